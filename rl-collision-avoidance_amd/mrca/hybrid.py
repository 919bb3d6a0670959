"""Parameters of the hybrid control wrapper (include/mrca_env.h: mrca_hybrid_params, mrca_hybrid_actions).  The defaults are the
library's own (mrca_hybrid_default_params): they are stated once, in C."""
import dataclasses

from . import _lib
from .params import ParamsMirror

MODE_NORMAL, MODE_SIMPLE, MODE_EMERGENT, MODE_AT_GOAL = 0, 1, 2, -2
MODE_NAMES = {MODE_NORMAL: "normal", MODE_SIMPLE: "simple", MODE_EMERGENT: "emergent", MODE_AT_GOAL: "at_goal"}


@dataclasses.dataclass
class HybridParams(ParamsMirror):
    """Mirror of mrca_hybrid_params; a field left ``None`` takes the library's default.  ``from_assignments``:
    ``["risk_dist=0.8", "look=3"]`` (the evaluator's --hybrid-param) -> HybridParams."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.HybridParamsStruct, "mrca_hybrid_default_params", "--hybrid-param"
    risk_dist: float = None             # a return nearer than this makes the robot careful (mode 2) [m], at most 6
    stop_dist: float = None             # the nearest return ahead at or below this: v = 0 [m], below risk_dist
    safe_scale: float = None            # the most of the incoming v that mode 2 lets through, 0..1
    corridor: float = None              # half width of the strip towards the goal that must be free for the PID law [m]
    look: float = None                  # its length at most [m], at most 6
    front_cos: float = None             # beams with cos >= this are "ahead"
    v_pid: float = None                 # speed of the PID law [m/s]
    k_omega: float = None               # its turn gain
    max_speed: float = None             # at most 1


@dataclasses.dataclass
class SafePolicyParams(ParamsMirror):
    """Mirror of mrca_safe_policy_params (hybrid control in the paper's form: mrca_hybrid_plan, mrca_hybrid_commit); a field
    left ``None`` takes the library's default.  ``from_assignments``: ``["scan_scale=0.7"]`` (the evaluator's
    --hybrid-safe-param) -> SafePolicyParams."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.SafePolicyParamsStruct, "mrca_safe_policy_default_params", "--hybrid-safe-param"
    scan_scale: float = None            # what a return's range is multiplied by in front of the network in mode 2, in (0, 1]
    v_cap: float = None                 # the most v that mode 2 lets through, in (0, 1]
