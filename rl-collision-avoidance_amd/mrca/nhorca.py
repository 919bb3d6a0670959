"""Parameters of the NH-ORCA baseline controller (include/mrca_env.h: mrca_nhorca_params, mrca_nhorca_actions).  The defaults are
the library's own (mrca_nhorca_default_params): they are stated once, in C."""
import dataclasses

from . import _lib
from .params import ParamsMirror

MODES = ("track", "turn", "still", "evade")     # MRCA_NHORCA_*: what mode_dev holds


@dataclasses.dataclass
class NhOrcaParams(ParamsMirror):
    """Mirror of mrca_nhorca_params; a field left ``None`` takes the library's default.  ``from_assignments``:
    ``["track_error=0.1", "max_neighbors=12"]`` (the evaluator's --nh-orca-param) -> NhOrcaParams."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.NhOrcaParamsStruct, "mrca_nhorca_default_params", "--nh-orca-param"
    radius: float = None                # disc a robot is treated as [m], before it grows by track_error
    neighbor_dist: float = None         # robots further away give no constraint [m]
    time_horizon: float = None          # robot constraints look this far ahead [s]
    time_horizon_obst: float = None     # the lidar's static points: this far [s]
    obst_dist: float = None             # wall returns further away give no constraint [m], at most 6
    v_pref: float = None                # speed towards the goal [m/s]
    max_speed: float = None
    responsibility: float = None        # share of the avoidance a robot takes on (0.5: reciprocal, 1: the other does nothing)
    k_omega: float = None               # (ORCA's field, not used)
    jitter: float = None                # the preferred velocity is turned by a fixed per-robot angle of at most this [rad]
    max_neighbors: int = None           # 1..46
    track_error: float = None           # the unicycle stays this close to the velocity ORCA chose [m], in (0, 0.5]
    track_time: float = None            # ... over this long [s], in [0.1, 1.5]
