// pybind11 bindings of optim.hip's AdamW (module `_dgadam`): Adam with decoupled weight decay.
// Its own extension, imported only for optimizer=adamw: `_dghip` and `_dgopt` (whose tests pin
// their public names) stay as they are.  Built from the same optim.hip as `_dgopt`, so the
// decay ranges and the gradient loads exist once.  Conventions as in opt_bindings.cpp: tensors
// cross as raw device addresses, the range table as the address of a host int64 array, the
// stream as its handle; a launcher's error becomes RuntimeError("<name>: <hipGetErrorString>").
// dg_api.h declares dg_adamw and dg_adamw_tick.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "dg_api.h"

namespace py = pybind11;

namespace {

template <typename T>
T* P(uintptr_t v) {
  return reinterpret_cast<T*>(v);
}

void check(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

PYBIND11_MODULE(_dgadam, m) {
  m.doc() = "deep_go_amd AdamW: Adam with decoupled weight decay (gfx950)";
  m.def("adamw", [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t v, size_t n, uintptr_t lr,
                    uintptr_t rec, float beta1, float beta2, float eps, float wd,
                    uintptr_t ranges, int n_ranges, float gscale, uintptr_t gate,
                    uintptr_t stream) {
    check(dg_adamw(P<float>(p), P<float>(g), P<float>(mom), P<float>(v), n, P<double>(lr),
                   P<void>(rec), beta1, beta2, eps, wd, P<long long>(ranges), n_ranges, gscale,
                   P<float>(gate), nullptr, reinterpret_cast<hipStream_t>(stream)),
          "adamw");
  }, "tick rec {t, c1, c2}; m, v moments; p *= 1 - lr wd [in ranges]; "
     "p -= lr c1 m / (sqrt(v) c2 + eps)");
  m.def("adamw_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t mom, uintptr_t v, size_t n,
                         uintptr_t lr, uintptr_t rec, float beta1, float beta2, float eps,
                         float wd, uintptr_t ranges, int n_ranges, float gscale, uintptr_t gate,
                         uintptr_t stream) {
    check(dg_adamw(P<float>(p), nullptr, P<float>(mom), P<float>(v), n, P<double>(lr),
                   P<void>(rec), beta1, beta2, eps, wd, P<long long>(ranges), n_ranges, gscale,
                   P<float>(gate), P<void>(g16), reinterpret_cast<hipStream_t>(stream)),
          "adamw_bf16");
  }, "adamw reading the bf16 (wire-format) gradient");
  m.def("adamw_tick", [](uintptr_t rec, float beta1, float beta2, uintptr_t gate,
                         uintptr_t stream) {
    check(dg_adamw_tick(P<void>(rec), beta1, beta2, P<float>(gate),
                        reinterpret_cast<hipStream_t>(stream)),
          "adamw_tick");
  }, "the count's launch alone (adamw issues it itself): behind an open gate t += 1, c1, c2");
}
