// pybind11 bindings of sched.hip (module `_dgsched`): the learning-rate schedule's launch.  Its
// own extension, imported only for lr_schedule != none.  dg_api.h declares dg_lr_sched;
// dg_bind.h says how it crosses the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dgsched, m) {
  m.doc() = "deep_go_amd learning-rate schedule (gfx950)";
  Bind<&dg_lr_sched>::def(
      m, "lr_sched",
      "rec {double base; int64 s}; advance: base *= 1 - rate_decay, s += 1; lr = base * f(s), "
      "kind 0 constant | 1 linear | 2 cosine | 3 step");
}
