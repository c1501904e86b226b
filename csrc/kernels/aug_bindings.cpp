// pybind11 bindings of augment.hip (module `_dgaug`): the training-time symmetry augmentation.
// Its own extension, imported only when augmentation is requested, so the interface of `_dghip`
// stays as recorded.  Conventions as in bindings.cpp: tensors cross as raw device addresses,
// the stream as its handle; dg_api.h declares both functions.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "dg_api.h"

namespace py = pybind11;

PYBIND11_MODULE(_dgaug, m) {
  m.doc() = "deep_go_amd on-device D4 batch augmentation (gfx950)";
  m.def("augment_batch", [](uintptr_t planes, uintptr_t labels, int B, uintptr_t sym,
                            unsigned long long seed, unsigned long long seq,
                            unsigned long long board0, uintptr_t sym_out, uintptr_t stream) {
    const hipError_t e = dg_augment_batch(
        reinterpret_cast<uint8_t*>(planes), reinterpret_cast<int*>(labels), B,
        reinterpret_cast<const uint8_t*>(sym), seed, seq, board0,
        reinterpret_cast<uint8_t*>(sym_out), reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess)
      throw std::runtime_error(std::string("augment_batch: ") + hipGetErrorString(e));
  }, "move every board of a packed batch in place by a board symmetry: sym[i] & 7 (sym non-zero) "
     "or the hash of (seed, seq, board0 + i); sym_out (optional): the ids used");
  m.def("augment_symmetry", &dg_augment_symmetry,
        "the symmetry id 0..7 the kernel draws for (seed, seq, board): host twin of its hash");
}
