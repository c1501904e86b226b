// pybind11 bindings of ema.hip (module `_dgema`): the exponential moving average of the weights.
// Its own extension, imported only for ema_decay > 0.  dg_api.h declares dg_ema_tick and dg_ema;
// dg_bind.h says how they cross the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dgema, m) {
  m.doc() = "deep_go_amd exponential moving average of the weights (gfx950)";
  Bind<&dg_ema>::def(
      m, "ema",
      "tick rec {int64 t; float omd; float pad}; e += omd (p - e), omd = 1 - min(decay, "
      "(1 + t) / (10 + t))");
  Bind<&dg_ema_tick>::def(
      m, "ema_tick",
      "the count's launch alone (ema issues it itself): behind an open gate t += 1, omd");
}
