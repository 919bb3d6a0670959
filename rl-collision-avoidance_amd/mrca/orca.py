"""Parameters of the ORCA baseline controller (include/mrca_env.h: mrca_orca_params, mrca_orca_actions).  The defaults are the
library's own (mrca_orca_default_params): they are stated once, in C."""
import dataclasses

from . import _lib
from .params import ParamsMirror


@dataclasses.dataclass
class OrcaParams(ParamsMirror):
    """Mirror of mrca_orca_params; a field left ``None`` takes the library's default.  ``from_assignments``:
    ``["radius=0.4", "max_neighbors=12"]`` (the evaluator's --orca-param) -> OrcaParams."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.OrcaParamsStruct, "mrca_orca_default_params", "--orca-param"
    radius: float = None                # disc a robot is treated as [m]
    neighbor_dist: float = None         # robots further away give no constraint [m]
    time_horizon: float = None          # robot constraints look this far ahead [s]
    time_horizon_obst: float = None     # the lidar's static points: this far [s]
    obst_dist: float = None             # wall returns further away give no constraint [m], at most 6
    v_pref: float = None                # speed towards the goal [m/s]
    max_speed: float = None
    responsibility: float = None        # share of the avoidance a robot takes on (0.5: reciprocal, 1: the other does nothing)
    k_omega: float = None               # turn-rate gain of the mapping to (v, omega)
    jitter: float = None                # the preferred velocity is turned by a fixed per-robot angle of at most this [rad]
    max_neighbors: int = None           # 0..48
