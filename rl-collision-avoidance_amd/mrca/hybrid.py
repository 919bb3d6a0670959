"""Parameters of the hybrid control wrapper (include/mrca_env.h: mrca_hybrid_params, mrca_hybrid_actions).  The defaults are the
library's own (mrca_hybrid_default_params): they are stated once, in C."""
import ctypes as C
import dataclasses

from . import _lib

_FIELDS = [name for name, _t in _lib.HybridParamsStruct._fields_]

MODE_NORMAL, MODE_SIMPLE, MODE_EMERGENT, MODE_AT_GOAL = 0, 1, 2, -2
MODE_NAMES = {MODE_NORMAL: "normal", MODE_SIMPLE: "simple", MODE_EMERGENT: "emergent", MODE_AT_GOAL: "at_goal"}


def _library_defaults():
    st = _lib.HybridParamsStruct()
    _lib.check(_lib.load().mrca_hybrid_default_params(C.byref(st)), "mrca_hybrid_default_params")
    return {k: getattr(st, k) for k in _FIELDS}


@dataclasses.dataclass
class HybridParams:
    """Mirror of mrca_hybrid_params; a field left ``None`` takes the library's default."""
    risk_dist: float = None             # a return nearer than this makes the robot careful (mode 2) [m], at most 6
    stop_dist: float = None             # the nearest return ahead at or below this: v = 0 [m], below risk_dist
    safe_scale: float = None            # the most of the incoming v that mode 2 lets through, 0..1
    corridor: float = None              # half width of the strip towards the goal that must be free for the PID law [m]
    look: float = None                  # its length at most [m], at most 6
    front_cos: float = None             # beams with cos >= this are "ahead"
    v_pid: float = None                 # speed of the PID law [m/s]
    k_omega: float = None               # its turn gain
    max_speed: float = None             # at most 1

    def __post_init__(self):
        for k, v in _library_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)

    def struct(self):
        return _lib.HybridParamsStruct(**{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_assignments(cls, items):
        """``["risk_dist=0.8", "look=3"]`` (the evaluator's --hybrid-param) -> HybridParams."""
        kw = {}
        for it in items or ():
            k, _eq, v = it.partition("=")
            if k not in _FIELDS or not _eq:
                raise ValueError(f"--hybrid-param {it!r}: expected name=value with name in {_FIELDS}")
            kw[k] = float(v)
        return cls(**kw)


_SAFE_FIELDS = [name for name, _t in _lib.SafePolicyParamsStruct._fields_]


def _library_safe_defaults():
    st = _lib.SafePolicyParamsStruct()
    _lib.check(_lib.load().mrca_safe_policy_default_params(C.byref(st)), "mrca_safe_policy_default_params")
    return {k: getattr(st, k) for k in _SAFE_FIELDS}


@dataclasses.dataclass
class SafePolicyParams:
    """Mirror of mrca_safe_policy_params (hybrid control in the paper's form: mrca_hybrid_plan, mrca_hybrid_commit); a field
    left ``None`` takes the library's default."""
    scan_scale: float = None            # what a return's range is multiplied by in front of the network in mode 2, in (0, 1]
    v_cap: float = None                 # the most v that mode 2 lets through, in (0, 1]

    def __post_init__(self):
        for k, v in _library_safe_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)

    def struct(self):
        return _lib.SafePolicyParamsStruct(**{k: getattr(self, k) for k in _SAFE_FIELDS})

    @classmethod
    def from_assignments(cls, items):
        """``["scan_scale=0.7"]`` (the evaluator's --hybrid-safe-param) -> SafePolicyParams."""
        kw = {}
        for it in items or ():
            k, _eq, v = it.partition("=")
            if k not in _SAFE_FIELDS or not _eq:
                raise ValueError(f"--hybrid-safe-param {it!r}: expected name=value with name in {_SAFE_FIELDS}")
            kw[k] = float(v)
        return cls(**kw)
