// pybind11 bindings of play.hip (module `_dgplay`): on-device move selection.  Its own
// extension, imported only when a selection is asked for.  dg_api.h declares both functions;
// dg_bind.h says how they cross the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dgplay, m) {
  m.doc() = "deep_go_amd on-device move selection (gfx950)";
  Bind<&dg_policy_select>::def(
      m, "policy_select",
      "one move per row of policy_ensemble's prob [n,361]: temperature, top_p nucleus, the draw "
      "select_uniform(seed, game[i], ply[i]); move [n], p_move [n] and kept [n] (both optional)");
  Bind<&dg_select_uniform>::def(
      m, "select_uniform",
      "the draw u in [0, 1) the kernel makes for (seed, game, ply): host twin of its hash");
}
