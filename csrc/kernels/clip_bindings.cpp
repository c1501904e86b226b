// pybind11 bindings of clip.hip (module `_dgclip`): global-norm gradient clipping.  Its own
// extension, imported only for grad_clip > 0: `_dghip`, `_dgopt` and `_dgadam` (whose tests pin
// their interfaces) stay as they are.  Conventions as in opt_bindings.cpp: tensors cross as raw
// device addresses, the stream as its handle; a launcher's error becomes
// RuntimeError("<name>: <hipGetErrorString>").  dg_api.h declares dg_grad_clip, dg_grad_norm
// and dg_clip_partials.
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

PYBIND11_MODULE(_dgclip, m) {
  m.doc() = "deep_go_amd gradient clipping by the global L2 norm (gfx950)";
  m.def("clip_partials", &dg_clip_partials, "floats the partial buffer must hold");
  m.def("grad_clip", [](uintptr_t g, size_t n, uintptr_t part, int part_n, uintptr_t rec,
                        float max_norm, float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_grad_clip(P<float>(g), nullptr, nullptr, n, P<float>(part), part_n, P<void>(rec),
                       max_norm, gscale, P<float>(gate), reinterpret_cast<hipStream_t>(stream)),
          "grad_clip");
  }, "norm = |gscale| sqrt(sum g^2); scale = min(1, max_norm / (norm + 1e-6)); g *= scale in "
     "place; rec {float norm; float scale; int64 clipped}");
  m.def("grad_clip_bf16", [](uintptr_t g16, uintptr_t out, size_t n, uintptr_t part, int part_n,
                             uintptr_t rec, float max_norm, float gscale, uintptr_t gate,
                             uintptr_t stream) {
    check(dg_grad_clip(nullptr, P<void>(g16), P<float>(out), n, P<float>(part), part_n,
                       P<void>(rec), max_norm, gscale, P<float>(gate),
                       reinterpret_cast<hipStream_t>(stream)),
          "grad_clip_bf16");
  }, "grad_clip reading the bf16 (wire-format) gradient: out = scale * float(g16), always "
     "written; g16 is not changed");
  m.def("grad_norm", [](uintptr_t g, size_t n, uintptr_t part, int part_n, uintptr_t gate,
                        uintptr_t stream) {
    check(dg_grad_norm(P<float>(g), nullptr, n, P<float>(part), part_n, P<float>(gate),
                       reinterpret_cast<hipStream_t>(stream)),
          "grad_norm");
  }, "the first launch alone (grad_clip issues it itself): the partials of sum g^2");
  m.def("grad_norm_bf16", [](uintptr_t g16, size_t n, uintptr_t part, int part_n, uintptr_t gate,
                             uintptr_t stream) {
    check(dg_grad_norm(nullptr, P<void>(g16), n, P<float>(part), part_n, P<float>(gate),
                       reinterpret_cast<hipStream_t>(stream)),
          "grad_norm_bf16");
  }, "grad_norm reading the bf16 (wire-format) gradient");
}
