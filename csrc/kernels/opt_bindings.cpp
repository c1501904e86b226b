// pybind11 bindings of optim.hip's momentum (module `_dgopt`): SGD with momentum, Nesterov and
// weight decay.  Its own extension, imported only for optimizer=momentum; its public names are
// pinned to the two below, so optim.hip's AdamW and LAMB are bound in modules of their own
// (adam_bindings.cpp, lamb_bindings.cpp).  dg_api.h declares dg_momentum; dg_bind.h says how it
// crosses the boundary (the range table is the address of a host int64 array).
#include "dg_bind.h"

PYBIND11_MODULE(_dgopt, m) {
  m.doc() = "deep_go_amd SGD with momentum / Nesterov / weight decay (gfx950)";
  m.def("momentum", [](uintptr_t p, uintptr_t g, uintptr_t v, size_t n, uintptr_t lr, float mu,
                       int nesterov, float wd, uintptr_t ranges, int n_ranges, float gscale,
                       uintptr_t gate, uintptr_t stream) {
    check(dg_momentum(P<float>(p), P<float>(g), P<float>(v), n, P<double>(lr), mu, nesterov, wd,
                      P<long long>(ranges), n_ranges, gscale, P<float>(gate), nullptr, S(stream)),
          "momentum");
  }, "v = mu v + (g gscale + wd p [in ranges]); p -= lr (nesterov ? gw + mu v : v)");
  m.def("momentum_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t v, size_t n, uintptr_t lr,
                            float mu, int nesterov, float wd, uintptr_t ranges, int n_ranges,
                            float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_momentum(P<float>(p), nullptr, P<float>(v), n, P<double>(lr), mu, nesterov, wd,
                      P<long long>(ranges), n_ranges, gscale, P<float>(gate), P<void>(g16),
                      S(stream)),
          "momentum_bf16");
  }, "momentum reading the bf16 (wire-format) gradient");
}
