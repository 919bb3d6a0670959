"""Parameters of the DWA baseline controller (include/mrca_env.h: mrca_dwa_params, mrca_dwa_actions).  The defaults are the
library's own (mrca_dwa_default_params): they are stated once, in C."""
import ctypes as C
import dataclasses

from . import _lib

_FIELDS = [name for name, _t in _lib.DwaParamsStruct._fields_]
_INTS = ("steps", "nv", "nw")


def _library_defaults():
    st = _lib.DwaParamsStruct()
    _lib.check(_lib.load().mrca_dwa_default_params(C.byref(st)), "mrca_dwa_default_params")
    return {k: getattr(st, k) for k in _FIELDS}


@dataclasses.dataclass
class DwaParams:
    """Mirror of mrca_dwa_params; a field left ``None`` takes the library's default."""
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

    def __post_init__(self):
        for k, v in _library_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)
        for k in _INTS:
            setattr(self, k, int(getattr(self, k)))

    def struct(self):
        return _lib.DwaParamsStruct(**{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_assignments(cls, items):
        """``["radius=0.4", "nw=31"]`` (the evaluator's --dwa-param) -> DwaParams."""
        kw = {}
        for it in items or ():
            k, _eq, v = it.partition("=")
            if k not in _FIELDS or not _eq:
                raise ValueError(f"--dwa-param {it!r}: expected name=value with name in {_FIELDS}")
            kw[k] = int(v) if k in _INTS else float(v)
        return cls(**kw)
