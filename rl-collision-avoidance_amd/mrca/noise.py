"""Parameters of the lidar noise model (include/mrca_env.h: mrca_scan_noise_params, mrca_scan_noise).  The defaults are the
library's own (mrca_scan_noise_default_params): they are stated once, in C."""
import ctypes as C
import dataclasses

from . import _lib

_FIELDS = [name for name, _t in _lib.ScanNoiseParamsStruct._fields_]
# the command line's short names (--lidar-noise const=0.02,prop=0.01,dropout=0.005,quantum=0.01)
_SHORT = {"const": "sigma_const", "prop": "sigma_prop"}


def _library_defaults():
    st = _lib.ScanNoiseParamsStruct()
    _lib.check(_lib.load().mrca_scan_noise_default_params(C.byref(st)), "mrca_scan_noise_default_params")
    return {k: getattr(st, k) for k in _FIELDS}


@dataclasses.dataclass
class ScanNoiseParams:
    """Mirror of mrca_scan_noise_params; a field left ``None`` takes the library's default."""
    sigma_const: float = None           # constant part of the range noise [m], at most 6
    sigma_prop: float = None            # ... and the part per metre of range, at most 1
    dropout: float = None               # probability that a returning beam reports nothing
    quantum: float = None               # read-out step [m], 0 = none, at most 1

    def __post_init__(self):
        for k, v in _library_defaults().items():
            if getattr(self, k) is None:
                setattr(self, k, v)

    def struct(self):
        return _lib.ScanNoiseParamsStruct(**{k: getattr(self, k) for k in _FIELDS})

    def as_dict(self):
        return {k: float(getattr(self, k)) for k in _FIELDS}

    @classmethod
    def from_assignments(cls, items):
        """``["const=0.02", "prop=0.01"]`` or ``"const=0.02,prop=0.01"`` (--lidar-noise) -> ScanNoiseParams.  A parameter that
        is not named is 0 -- what is asked for is what is applied; an empty list gives the library's defaults."""
        if isinstance(items, str):
            items = [it for it in items.split(",") if it]
        if not items or list(items) == ["default"]:
            return cls()
        kw = dict.fromkeys(_FIELDS, 0.0)
        for it in items:
            k, _eq, v = it.partition("=")
            k = _SHORT.get(k, k)
            if k not in _FIELDS or not _eq:
                raise ValueError(f"--lidar-noise {it!r}: expected name=value with name in {sorted(_SHORT) + _FIELDS}")
            kw[k] = float(v)
        return cls(**kw)
