// pybind11 bindings of augment.hip (module `_dgaug`): the training-time symmetry augmentation.
// Its own extension, imported only when augmentation is requested.  dg_api.h declares both
// functions; dg_bind.h says how they cross the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dgaug, m) {
  m.doc() = "deep_go_amd on-device D4 batch augmentation (gfx950)";
  Bind<&dg_augment_batch>::def(
      m, "augment_batch",
      "move every board of a packed batch in place by a board symmetry: sym[i] & 7 (sym non-zero) "
      "or the hash of (seed, seq, board0 + i); sym_out (optional): the ids used");
  Bind<&dg_augment_symmetry>::def(
      m, "augment_symmetry",
      "the symmetry id 0..7 the kernel draws for (seed, seq, board): host twin of its hash");
}
