// pybind11 bindings of ema.hip (module `_dgema`): the exponential moving average of the weights.
// Its own extension, imported only for ema_decay > 0: `_dghip`, `_dgopt`, `_dgadam` and
// `_dgclip` (whose tests pin their interfaces) stay as they are.  Conventions as in
// opt_bindings.cpp: tensors cross as raw device addresses, the stream as its handle; a
// launcher's error becomes RuntimeError("<name>: <hipGetErrorString>").  dg_api.h declares
// dg_ema_tick and dg_ema.
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

PYBIND11_MODULE(_dgema, m) {
  m.doc() = "deep_go_amd exponential moving average of the weights (gfx950)";
  m.def("ema", [](uintptr_t p, uintptr_t e, size_t n, uintptr_t rec, double decay,
                  uintptr_t gate, uintptr_t stream) {
    check(dg_ema(P<float>(p), P<float>(e), n, P<void>(rec), decay, P<float>(gate),
                 reinterpret_cast<hipStream_t>(stream)),
          "ema");
  }, "tick rec {int64 t; float omd; float pad}; e += omd (p - e), omd = 1 - min(decay, "
     "(1 + t) / (10 + t))");
  m.def("ema_tick", [](uintptr_t rec, double decay, uintptr_t gate, uintptr_t stream) {
    check(dg_ema_tick(P<void>(rec), decay, P<float>(gate),
                      reinterpret_cast<hipStream_t>(stream)),
          "ema_tick");
  }, "the count's launch alone (ema issues it itself): behind an open gate t += 1, omd");
}
