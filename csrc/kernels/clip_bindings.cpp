// pybind11 bindings of clip.hip (module `_dgclip`): global-norm gradient clipping.  Its own
// extension, imported only for grad_clip > 0.  dg_api.h declares dg_grad_clip, dg_grad_norm and
// dg_clip_partials; dg_bind.h says how they cross the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dgclip, m) {
  m.doc() = "deep_go_amd gradient clipping by the global L2 norm (gfx950)";
  Bind<&dg_clip_partials>::def(m, "clip_partials", "floats the partial buffer must hold");
  m.def("grad_clip", [](uintptr_t g, size_t n, uintptr_t part, int part_n, uintptr_t rec,
                        float max_norm, float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_grad_clip(P<float>(g), nullptr, nullptr, n, P<float>(part), part_n, P<void>(rec),
                       max_norm, gscale, P<float>(gate), S(stream)),
          "grad_clip");
  }, "norm = |gscale| sqrt(sum g^2); scale = min(1, max_norm / (norm + 1e-6)); g *= scale in "
     "place; rec {float norm; float scale; int64 clipped}");
  m.def("grad_clip_bf16", [](uintptr_t g16, uintptr_t out, size_t n, uintptr_t part, int part_n,
                             uintptr_t rec, float max_norm, float gscale, uintptr_t gate,
                             uintptr_t stream) {
    check(dg_grad_clip(nullptr, P<void>(g16), P<float>(out), n, P<float>(part), part_n,
                       P<void>(rec), max_norm, gscale, P<float>(gate), S(stream)),
          "grad_clip_bf16");
  }, "grad_clip reading the bf16 (wire-format) gradient: out = scale * float(g16), always "
     "written; g16 is not changed");
  m.def("grad_norm", [](uintptr_t g, size_t n, uintptr_t part, int part_n, uintptr_t gate,
                        uintptr_t stream) {
    check(dg_grad_norm(P<float>(g), nullptr, n, P<float>(part), part_n, P<float>(gate),
                       S(stream)),
          "grad_norm");
  }, "the first launch alone (grad_clip issues it itself): the partials of sum g^2");
  m.def("grad_norm_bf16", [](uintptr_t g16, size_t n, uintptr_t part, int part_n, uintptr_t gate,
                             uintptr_t stream) {
    check(dg_grad_norm(nullptr, P<void>(g16), n, P<float>(part), part_n, P<float>(gate),
                       S(stream)),
          "grad_norm_bf16");
  }, "grad_norm reading the bf16 (wire-format) gradient");
}
