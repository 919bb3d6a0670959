"""Parameters and boxes of the scenario sampler (include/mrca_env.h: mrca_scatter_params, mrca_scatter).  The defaults are the
library's own (mrca_scatter_default_params): they are stated once, in C.  ``check_boxes`` is the PRODUCER of ``boxes_dev``: the
library does not validate device memory, so what it may rely on is guaranteed here."""
import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .params import ParamsMirror

COORD_MAX = 1.0e4       # |coordinate| of a box: a map cell index stays an exact integer in float32 on any map the env takes


@dataclasses.dataclass
class ScatterParams(ParamsMirror):
    """Mirror of mrca_scatter_params; a field left ``None`` takes the library's default."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.ScatterParamsStruct, "mrca_scatter_default_params", "--scatter-param"
    min_sep: float = None               # starts of one world: centre distance >= this [m], at least 0.6
    goal_sep: float = None              # goals of one world likewise (0: no test)
    goal_min: float = None              # goal_min <= |goal - own start| <= goal_max
    goal_max: float = None
    clear_cells: int = None             # Chebyshev distance to an occupied map cell > this (0..254)
    max_tries: int = None               # 1..65536 candidates per start and per goal
    draw: int = None                    # scenario number: another draw, another set of scenarios

    @classmethod
    def _types(cls):
        return {k: (float if t is C.c_float else int) for k, t in cls._STRUCT._fields_}

    @classmethod
    def from_assignments(cls, items, start=None):
        """``["min_sep=0.8", "max_tries=4096"]`` or ``"min_sep=0.8,max_tries=4096"`` (--scatter-param) on top of ``start`` (a
        dict of fields; default: the library's defaults) -> ScatterParams."""
        if isinstance(items, str):
            items = [it for it in items.split(",") if it]
        return super().from_assignments(items, start=start)


def check_boxes(boxes, R):
    """``boxes`` -> float32[R,8] (sx0, sy0, sx1, sy1, gx0, gy0, gx1, gy1 per local index), or ValueError: every value finite,
    x0 <= x1 and y0 <= y1 in both halves, |coordinate| <= 1e4 -- what mrca_scatter relies on without looking."""
    b = np.asarray(boxes, np.float64)
    if b.shape != (int(R), 8):
        raise ValueError(f"scatter boxes: expected shape ({int(R)}, 8), got {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError(f"scatter boxes: row {int(np.argwhere(~np.isfinite(b))[0, 0])} holds a value that is not finite")
    if (np.abs(b) > COORD_MAX).any():
        raise ValueError(f"scatter boxes: row {int(np.argwhere(np.abs(b) > COORD_MAX)[0, 0])} holds a coordinate beyond +-{COORD_MAX:g}")
    b32 = np.ascontiguousarray(b, np.float32)
    for lo, hi, what in ((0, 2, "sx0 > sx1"), (1, 3, "sy0 > sy1"), (4, 6, "gx0 > gx1"), (5, 7, "gy0 > gy1")):
        bad = np.flatnonzero(b32[:, lo] > b32[:, hi])
        if bad.size:
            raise ValueError(f"scatter boxes: row {int(bad[0])} has {what}")
    return b32
