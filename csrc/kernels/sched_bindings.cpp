// pybind11 bindings of sched.hip (module `_dgsched`): the learning-rate schedule's launch.  Its
// own extension, imported only for lr_schedule != none: `_dghip`, `_dgopt`, `_dgadam`, `_dgclip`
// and `_dgema` (whose tests pin their interfaces) stay as they are.  Conventions as in
// opt_bindings.cpp: tensors cross as raw device addresses, the stream as its handle; a
// launcher's error becomes RuntimeError("<name>: <hipGetErrorString>").  dg_api.h declares
// dg_lr_sched.
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

PYBIND11_MODULE(_dgsched, m) {
  m.doc() = "deep_go_amd learning-rate schedule (gfx950)";
  m.def("lr_sched", [](uintptr_t rec, uintptr_t lr, int kind, long long W, long long T, double mn,
                       long long E, double g, double rate_decay, int advance, uintptr_t stream) {
    check(dg_lr_sched(P<void>(rec), P<double>(lr), kind, W, T, mn, E, g, rate_decay, advance,
                      reinterpret_cast<hipStream_t>(stream)),
          "lr_sched");
  }, "rec {double base; int64 s}; advance: base *= 1 - rate_decay, s += 1; lr = base * f(s), "
     "kind 0 constant | 1 linear | 2 cosine | 3 step");
}
