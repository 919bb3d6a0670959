"""Parameters of the lidar noise model (include/mrca_env.h: mrca_scan_noise_params, mrca_scan_noise).  The defaults are the
library's own (mrca_scan_noise_default_params): they are stated once, in C."""
import dataclasses

from . import _lib
from .params import ParamsMirror


@dataclasses.dataclass
class ScanNoiseParams(ParamsMirror):
    """Mirror of mrca_scan_noise_params; a field left ``None`` takes the library's default."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.ScanNoiseParamsStruct, "mrca_scan_noise_default_params", "--lidar-noise"
    # the command line's short names (--lidar-noise const=0.02,prop=0.01,dropout=0.005,quantum=0.01)
    _SHORT = {"const": "sigma_const", "prop": "sigma_prop"}
    sigma_const: float = None           # constant part of the range noise [m], at most 6
    sigma_prop: float = None            # ... and the part per metre of range, at most 1
    dropout: float = None               # probability that a returning beam reports nothing
    quantum: float = None               # read-out step [m], 0 = none, at most 1

    @classmethod
    def from_assignments(cls, items):
        """``["const=0.02", "prop=0.01"]`` or ``"const=0.02,prop=0.01"`` (--lidar-noise) -> ScanNoiseParams.  A parameter that
        is not named is 0 -- what is asked for is what is applied; an empty list gives the library's defaults."""
        if isinstance(items, str):
            items = [it for it in items.split(",") if it]
        if not items or list(items) == ["default"]:
            return cls()
        return super().from_assignments(items, start=dict.fromkeys(cls._types(), 0.0))
