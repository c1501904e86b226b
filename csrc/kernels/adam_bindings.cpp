// pybind11 bindings of optim.hip's AdamW (module `_dgadam`): Adam with decoupled weight decay.
// Its own extension, imported only for optimizer=adamw.  dg_api.h declares dg_adamw and
// dg_adamw_tick; dg_bind.h says how they cross the boundary (the range table is the address of
// a host int64 array).
#include "dg_bind.h"

PYBIND11_MODULE(_dgadam, m) {
  m.doc() = "deep_go_amd AdamW: Adam with decoupled weight decay (gfx950)";
  m.def("adamw", [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t v, size_t n, uintptr_t lr,
                    uintptr_t rec, float beta1, float beta2, float eps, float wd,
                    uintptr_t ranges, int n_ranges, float gscale, uintptr_t gate,
                    uintptr_t stream) {
    check(dg_adamw(P<float>(p), P<float>(g), P<float>(mom), P<float>(v), n, P<double>(lr),
                   P<void>(rec), beta1, beta2, eps, wd, P<long long>(ranges), n_ranges, gscale,
                   P<float>(gate), nullptr, S(stream)),
          "adamw");
  }, "tick rec {t, c1, c2}; m, v moments; p *= 1 - lr wd [in ranges]; "
     "p -= lr c1 m / (sqrt(v) c2 + eps)");
  m.def("adamw_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t mom, uintptr_t v, size_t n,
                         uintptr_t lr, uintptr_t rec, float beta1, float beta2, float eps,
                         float wd, uintptr_t ranges, int n_ranges, float gscale, uintptr_t gate,
                         uintptr_t stream) {
    check(dg_adamw(P<float>(p), nullptr, P<float>(mom), P<float>(v), n, P<double>(lr),
                   P<void>(rec), beta1, beta2, eps, wd, P<long long>(ranges), n_ranges, gscale,
                   P<float>(gate), P<void>(g16), S(stream)),
          "adamw_bf16");
  }, "adamw reading the bf16 (wire-format) gradient");
  Bind<&dg_adamw_tick>::def(
      m, "adamw_tick",
      "the count's launch alone (adamw issues it itself): behind an open gate t += 1, c1, c2");
}
