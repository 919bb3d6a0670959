"""Parameters of the DWA baseline controller (include/mrca_env.h: mrca_dwa_params, mrca_dwa_actions).  The defaults are the
library's own (mrca_dwa_default_params): they are stated once, in C."""
import dataclasses

from . import _lib
from .params import ParamsMirror


@dataclasses.dataclass
class DwaParams(ParamsMirror):
    """Mirror of mrca_dwa_params; a field left ``None`` takes the library's default.  ``from_assignments``:
    ``["radius=0.4", "nw=31"]`` (the evaluator's --dwa-param) -> DwaParams."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.DwaParamsStruct, "mrca_dwa_default_params", "--dwa-param"
    radius: float = None                # disc the robot is treated as [m]
    horizon: float = None               # length of a rollout [s]
    obst_dist: float = None             # returns further away give no obstacle point [m], at most 6
    clear_cap: float = None             # clearance beyond this scores no better [m]
    max_speed: float = None             # at most 1
    max_omega: float = None             # at most 1
    acc_v: float = None                 # the window reaches v0 +- acc_v * 0.1 s
    acc_w: float = None                 # ... and w0 +- acc_w * 0.1 s
    w_goal: float = None                # weight of the progress towards the goal
    w_heading: float = None             # ... of the end heading pointing at the goal
    w_clear: float = None               # ... of the clearance
    w_speed: float = None               # ... of the forward speed
    steps: int = None                   # sub-steps of a rollout, 1..64
    nv: int = None                      # samples of v, 1..16
    nw: int = None                      # samples of omega, 1..64
