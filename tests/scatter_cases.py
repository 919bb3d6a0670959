"""The cases of the scenario sampler's tests (tests/test_scatter_host.py: the g++ build of csrc/mrca_scatter_device.h;
tests/test_gpu_scatter.py: the library) and the restatement's answer to each, computed ONCE per process and handed out
read-only.  A case is (grid, seed, W, R, boxes f32[R,8], params); shapes are the smallest at which the kernel takes another
path: one lane's worth of robots, a full wave (64), the 256-lane block with a partial last wave (65, 130) and more rounds than
one (300 robots; the narrow bands), one world and three."""
import functools

import numpy as np

import scatter_ref as R
from util import S

f32 = np.float32
SEED = 0x5CA77E2012345678


def same_box(n, start, goal=None):
    return np.tile(np.asarray(list(start) + list(goal or start), f32), (n, 1))


def holes_grid():
    """4 m x 3 m of 0.1 m cells WITHOUT a border wall (so that cells at the map's edge have bytes of their own) and three blocks"""
    occ = np.zeros((30, 40), bool)
    occ[12:16, 5:8] = True          # near the left edge
    occ[27:30, 20:24] = True        # touching the top edge
    occ[2:4, 36:39] = True          # near the lower right corner
    return S.GridData.from_dense(occ, 0.1, -2.0, -1.5)


def edge_boxes():
    """eight robots whose x is PINNED on, beside and beyond the map's left and right edge (cells -2, -1, 0, 0, w-1, w, w, w+3)
    with y drawn from below the map to above it; the goals likewise with x and y free around the whole map"""
    xs = [-2.15, -2.05, -2.0, -1.95, 1.95, 2.0, 2.05, 2.35]
    b = np.zeros((8, 8), f32)
    for i, x in enumerate(xs):
        b[i] = (x, -2.2, x, 2.2, -2.6, -2.1, 2.6, 2.1)
    return b


def pinned_boxes():
    """table robots among random ones: 0 and 1 have start AND goal pinned to a point, 2 a pinned start x, 3 a pinned goal y"""
    b = same_box(6, (-6.0, -6.0, 6.0, 6.0))
    b[0] = (-3.0, 1.5, -3.0, 1.5, 4.0, -2.0, 4.0, -2.0)
    b[1] = (2.25, -4.0, 2.25, -4.0, -5.0, 5.0, -5.0, 5.0)
    b[2, [0, 2]] = -0.5
    b[3, [5, 7]] = 0.75
    return b


def _open():
    return S.empty_grid()


def _doorway():
    return S.doorway().grid


WIDE = (-10.0, -10.0, 10.0, 10.0)
ROOM = (-4.9, -3.9, 4.9, 3.9)          # the doorway's whole room, walls included
NARROW = dict(goal_min=4.0, goal_max=4.02, max_tries=16384)      # a ring of 0.5 m^2 in 400 m^2: some 800 candidates per goal

# name -> (grid maker, W, R, boxes maker, params); "gpu": also run against the library
CASES = {}
for _R in (1, 3, 64, 65, 130):
    for _W in (1, 3):
        CASES[f"open_R{_R}_W{_W}"] = (_open, _W, _R, functools.partial(same_box, _R, WIDE), R.params(goal_min=3.0))
for _c in (0, 4, 10):
    CASES[f"doorway_clear{_c}"] = (_doorway, 2, 6, functools.partial(same_box, 6, ROOM), R.params(clear_cells=_c, goal_min=2.0, min_sep=0.8))
CASES["off_map"] = (holes_grid, 3, 8, edge_boxes, R.params(clear_cells=2, min_sep=0.6, goal_sep=0.6, goal_min=0.5, max_tries=300))
CASES["pinned"] = (_open, 2, 6, pinned_boxes, R.params(goal_min=1.0))
for _t in (1, 100, 300):
    CASES[f"tries{_t}"] = (_open, 2, 12, functools.partial(same_box, 12, (0.0, 0.0, 4.0, 4.0)), R.params(max_tries=_t, goal_min=1.0))
CASES["narrow_R4"] = (_open, 1, 4, functools.partial(same_box, 4, WIDE), R.params(**NARROW))
CASES["narrow_R65"] = (_open, 1, 65, functools.partial(same_box, 65, WIDE), R.params(goal_sep=0.0, **NARROW))
CASES["infeasible"] = (_open, 1, 16, functools.partial(same_box, 16, (1.0, 1.0, 3.0, 3.0)), R.params(goal_min=0.0, max_tries=300))
CASES["open_R300_W1"] = (_open, 1, 300, functools.partial(same_box, 300, (-30.0, -30.0, 30.0, 30.0)), R.params(goal_min=3.0))

HOST_CASES = [k for k in CASES if k != "open_R300_W1"]
GPU_CASES = ["open_R1_W1", "open_R3_W3", "open_R64_W1", "open_R64_W3", "open_R65_W1", "open_R130_W3", "open_R300_W1", "doorway_clear4", "off_map",
             "pinned", "tries100", "tries300", "narrow_R4", "narrow_R65", "infeasible"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (grid, W, R, boxes, params, (poses, goals, tries) of the restatement); the arrays are read-only"""
    make_grid, W, Rn, make_boxes, p = CASES[name]
    grid, boxes = make_grid(), np.ascontiguousarray(make_boxes(), f32)
    want = R.scatter(p, grid, SEED, W, Rn, boxes)
    for a in want + (boxes,):
        a.setflags(write=False)
    return grid, W, Rn, boxes, dict(p), want
