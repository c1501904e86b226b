// pybind11 bindings of optim.hip (module `_dgopt`): SGD with momentum, Nesterov and weight
// decay.  Its own extension, imported only for optimizer=momentum, so the interface of `_dghip`
// stays as recorded.  Conventions as in bindings.cpp: tensors cross as raw device addresses,
// the range table as the address of a host int64 array, the stream as its handle; a launcher's
// error becomes RuntimeError("<name>: <hipGetErrorString>").  dg_api.h declares dg_momentum.
// optim.hip also holds AdamW (dg_adamw); that is bound in adam_bindings.cpp (module `_dgadam`),
// because this module's public names are pinned to the two below.
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

PYBIND11_MODULE(_dgopt, m) {
  m.doc() = "deep_go_amd SGD with momentum / Nesterov / weight decay (gfx950)";
  m.def("momentum", [](uintptr_t p, uintptr_t g, uintptr_t v, size_t n, uintptr_t lr, float mu,
                       int nesterov, float wd, uintptr_t ranges, int n_ranges, float gscale,
                       uintptr_t gate, uintptr_t stream) {
    check(dg_momentum(P<float>(p), P<float>(g), P<float>(v), n, P<double>(lr), mu, nesterov, wd,
                      P<long long>(ranges), n_ranges, gscale, P<float>(gate), nullptr,
                      reinterpret_cast<hipStream_t>(stream)),
          "momentum");
  }, "v = mu v + (g gscale + wd p [in ranges]); p -= lr (nesterov ? gw + mu v : v)");
  m.def("momentum_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t v, size_t n, uintptr_t lr,
                            float mu, int nesterov, float wd, uintptr_t ranges, int n_ranges,
                            float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_momentum(P<float>(p), nullptr, P<float>(v), n, P<double>(lr), mu, nesterov, wd,
                      P<long long>(ranges), n_ranges, gscale, P<float>(gate), P<void>(g16),
                      reinterpret_cast<hipStream_t>(stream)),
          "momentum_bf16");
  }, "momentum reading the bf16 (wire-format) gradient");
}
