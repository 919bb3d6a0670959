"""Parameters of the ORCA baseline controller (include/mrca_env.h: mrca_orca_params, mrca_orca_actions).  The defaults are the
library's own (mrca_orca_default_params): they are stated once, in C."""
import ctypes as C
import dataclasses

from . import _lib

_FIELDS = [name for name, _t in _lib.OrcaParamsStruct._fields_]


def _library_defaults():
    st = _lib.OrcaParamsStruct()
    _lib.check(_lib.load().mrca_orca_default_params(C.byref(st)), "mrca_orca_default_params")
    return {k: getattr(st, k) for k in _FIELDS}


@dataclasses.dataclass
class OrcaParams:
    """Mirror of mrca_orca_params; a field left ``None`` takes the library's default."""
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

    def __post_init__(self):
        for k, v in _library_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)
        self.max_neighbors = int(self.max_neighbors)

    def struct(self):
        return _lib.OrcaParamsStruct(**{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_assignments(cls, items):
        """``["radius=0.4", "max_neighbors=12"]`` (the evaluator's --orca-param) -> OrcaParams."""
        kw = {}
        for it in items or ():
            k, _eq, v = it.partition("=")
            if k not in _FIELDS or not _eq:
                raise ValueError(f"--orca-param {it!r}: expected name=value with name in {_FIELDS}")
            kw[k] = int(v) if k == "max_neighbors" else float(v)
        return cls(**kw)
