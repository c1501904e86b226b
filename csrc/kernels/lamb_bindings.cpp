// pybind11 bindings of optim.hip's LAMB (module `_dglamb`): Adam's update rescaled per
// conv-weight tensor by a trust ratio.  Its own extension, imported only for optimizer=lamb.
// dg_api.h declares dg_lamb and dg_lamb_partials; dg_bind.h says how they cross the boundary
// (the range table is the address of a host int64 array).
#include "dg_bind.h"

PYBIND11_MODULE(_dglamb, m) {
  m.doc() = "deep_go_amd LAMB: layer-wise trust ratios on Adam (gfx950)";
  m.def("lamb", [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t v, uintptr_t u, size_t n,
                   uintptr_t lr, uintptr_t rec, uintptr_t part, long long part_n, uintptr_t tab,
                   float beta1, float beta2, float eps, float wd, uintptr_t ranges, int n_ranges,
                   float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_lamb(P<float>(p), P<float>(g), P<float>(mom), P<float>(v), P<float>(u), n,
                  P<double>(lr), P<void>(rec), P<float>(part), part_n, P<float>(tab), beta1,
                  beta2, eps, wd, P<long long>(ranges), n_ranges, gscale, P<float>(gate),
                  nullptr, S(stream)),
          "lamb");
  }, "tick rec {t, c1, c2}; m, v moments; u = c1 m / (sqrt(v) c2 + eps) [+ wd p in ranges]; "
     "tab[k] = {|p_k|, |u_k|, phi_k}; p -= lr phi u");
  m.def("lamb_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t mom, uintptr_t v, uintptr_t u,
                        size_t n, uintptr_t lr, uintptr_t rec, uintptr_t part, long long part_n,
                        uintptr_t tab, float beta1, float beta2, float eps, float wd,
                        uintptr_t ranges, int n_ranges, float gscale, uintptr_t gate,
                        uintptr_t stream) {
    check(dg_lamb(P<float>(p), nullptr, P<float>(mom), P<float>(v), P<float>(u), n,
                  P<double>(lr), P<void>(rec), P<float>(part), part_n, P<float>(tab), beta1,
                  beta2, eps, wd, P<long long>(ranges), n_ranges, gscale, P<float>(gate),
                  P<void>(g16), S(stream)),
          "lamb_bf16");
  }, "lamb reading the bf16 (wire-format) gradient");
  m.def("lamb_partials", [](size_t n, uintptr_t ranges, int n_ranges) {
    const long long need = dg_lamb_partials(n, P<long long>(ranges), n_ranges);
    if (need < 0) check(hipErrorInvalidValue, "lamb_partials");
    return need;
  }, "the floats the partial buffer needs for n elements and this range table");
}
