"""Maps and poses the planner's host and GPU tests share (tests/test_planner_host.py, tests/test_gpu_planner.py)."""
import numpy as np

import planner_ref as R
import util as U
from util import S

f32 = np.float32


def serpentine_grid():
    """70 x 70 cells of 0.25 m (a tile border on both axes at stride 1) with horizontal walls that leave a gap at alternating
    ends: the shortest path from the bottom to the top crosses the tile border at column 64 once per band."""
    occ = np.zeros((70, 70), bool)
    for b, row in enumerate(range(6, 66, 6)):
        occ[row, :] = True
        if b % 2 == 0:
            occ[row, 66:69] = False
        else:
            occ[row, 1:4] = False
    return S.GridData.from_dense(occ, 0.25, -8.75, -8.75)


def odd_grid(seed=3):
    """131 x 67 cells: multiples of neither the tile nor stride 3; scattered blocks and two long walls."""
    rng = np.random.default_rng(seed)
    occ = rng.random((67, 131)) < 0.03
    occ[20, 10:100] = True
    occ[45, 30:131] = True
    occ[33, 50] = False
    return S.GridData.from_dense(occ, 0.1, -6.55, -3.35)


# the crafted map: 61 x 45 cells of 0.25 m (odd on both axes: the last planning cell of stride 2 is cut), NO border wall (a
# robot can stand off grid), a long wall with its gap at the top, a closed box (its inside is cut off), a block for a goal inside
# the inflation
CRAFTED_X0, CRAFTED_Y0, CRAFTED_CELL = -7.5, -5.5, 0.25


def crafted_grid():
    occ = np.zeros((45, 61), bool)
    occ[0:35, 30] = True                    # the wall: the way across is over its top
    occ[5:16, 40] = occ[5:16, 50] = True    # the box
    occ[5, 40:51] = occ[15, 40:51] = True
    occ[38:41, 8:11] = True                 # the block
    return S.GridData.from_dense(occ, CRAFTED_CELL, CRAFTED_X0, CRAFTED_Y0)


def centre(ix, iy):
    """the middle of map cell (ix, iy) of the crafted map"""
    return (CRAFTED_X0 + (ix + 0.5) * CRAFTED_CELL, CRAFTED_Y0 + (iy + 0.5) * CRAFTED_CELL)


CRAFTED_PARAMS = dict(stride=2, inflate=1, lookahead=6, max_rounds=0)
# goal points: 0 in the open right half, 1 in the open left half, 2 inside the block's inflation (a blocked seed), 3 off grid,
# 4 inside the box
CRAFTED_GOALS = np.array([centre(56, 30), centre(12, 12), centre(11, 39), (-9.0, 0.0), centre(45, 10)], f32)


def crafted_poses():
    """-> (names, pose f32[n, 3], slot i32[n]): robots that stand on the edges of the rule"""
    gx, gy = 56 // 2, 30 // 2                # goal 0's planning cell
    rows = [
        ("open_far", centre(4, 4) + (0.3,), 0),
        ("in_inflation", centre(29, 10) + (1.0,), 0),             # beside the wall: a blocked cell, the escape step
        ("in_wall", centre(30, 10) + (-2.0,), 1),
        ("in_pocket", centre(45, 10) + (0.5,), 0),                # inside the box: no path to goal 0
        ("in_pocket_own_goal", centre(46, 11) + (0.5,), 4),       # ... but to the goal inside it
        ("off_grid_left", (CRAFTED_X0 - 1.0, 0.0, 0.0), 0),
        ("off_grid_above", (0.0, CRAFTED_Y0 + 45 * CRAFTED_CELL + 0.01, 3.0), 1),
        ("on_cell_border", (CRAFTED_X0 + 20 * CRAFTED_CELL, CRAFTED_Y0 + 14 * CRAFTED_CELL, -1.0), 0),
        ("on_last_cut_cell", centre(60, 44) + (2.0,), 0),
        ("tie_straight_diagonal", centre(2 * (gx - 2), 2 * (gy - 1)) + (0.0,), 0),   # E then NE costs what NE then E does
        ("seed_within_lookahead", centre(2 * (gx - 3), 2 * gy) + (3.0,), 0),
        ("seed_at_lookahead", centre(2 * (gx - 6), 2 * gy) + (3.0,), 0),
        ("seed_beyond_lookahead", centre(2 * (gx - 7), 2 * gy) + (3.0,), 0),
        ("on_the_seed", tuple(CRAFTED_GOALS[1]) + (0.7,), 1),
        ("to_blocked_seed", centre(30, 38) + (0.0,), 2),
        ("to_off_grid_goal", centre(20, 20) + (0.0,), 3),
        ("no_slot", centre(20, 20) + (0.0,), -1),
        ("slot_too_large", centre(20, 20) + (0.0,), len(CRAFTED_GOALS)),
    ]
    names = [r[0] for r in rows]
    return names, np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], np.int32)


def random_poses(rng, n, grid):
    """poses over the map and a margin around it (some off grid), slots over the crafted goals and beyond"""
    w, h = grid.width * grid.cell, grid.height * grid.cell
    pose = np.stack([rng.uniform(grid.x0 - 0.5, grid.x0 + w + 0.5, n), rng.uniform(grid.y0 - 0.5, grid.y0 + h + 0.5, n),
                     rng.uniform(-np.pi, np.pi, n)], 1).astype(f32)
    slot = rng.integers(-1, len(CRAFTED_GOALS) + 1, n).astype(np.int32)
    return pose, slot


def head_of(pose):
    """(sine, cosine) of the headings as the env's head records hold them"""
    sn, cs = U.O.sincos(np.asarray(pose, f32)[:, 2], f32)
    return np.stack([sn, cs], 1).astype(f32)


def crafted_fields(p=None):
    """-> (grid, params, blocked, fields u32[G, PH, PW]) of the crafted map by the restatement"""
    g = crafted_grid()
    p = R.params(**CRAFTED_PARAMS) if p is None else p
    blocked = R.blocked_mask(g, p["stride"], p["inflate"])
    return g, p, blocked, np.stack([R.goal_field(g, p, goal, blocked) for goal in CRAFTED_GOALS])


def crafted_expectations(names, status, sub, dist, goals=CRAFTED_GOALS):
    """what the restatement must say about the crafted poses: the branch each one takes is asserted, not hoped for"""
    ix = {k: i for i, k in enumerate(names)}
    st = lambda k: int(status[ix[k]])
    assert st("open_far") == R.ON_PATH and np.isfinite(dist[ix["open_far"]])
    assert st("in_inflation") == R.ON_PATH and np.isinf(dist[ix["in_inflation"]])          # it escapes, its own cell is INF
    assert st("in_wall") == R.ON_PATH and np.isinf(dist[ix["in_wall"]])
    assert st("in_pocket") == R.NO_PATH and np.isinf(dist[ix["in_pocket"]])
    assert st("in_pocket_own_goal") == R.ON_GOAL
    assert st("off_grid_left") == R.NO_PATH and st("off_grid_above") == R.NO_PATH
    assert st("on_cell_border") == R.ON_PATH and st("on_last_cut_cell") == R.ON_PATH
    assert st("seed_within_lookahead") == R.ON_GOAL and st("seed_at_lookahead") == R.ON_GOAL
    assert st("seed_beyond_lookahead") == R.ON_PATH and st("on_the_seed") == R.ON_GOAL and dist[ix["on_the_seed"]] == 0.0
    assert st("to_blocked_seed") == R.ON_PATH and np.isfinite(dist[ix["to_blocked_seed"]])
    assert st("to_off_grid_goal") == R.NO_PATH and st("no_slot") == R.NO_SLOT and st("slot_too_large") == R.NO_SLOT
    for k in ("seed_within_lookahead", "on_the_seed"):
        assert np.array_equal(sub[ix[k]].view(np.uint32), goals[0 if k != "on_the_seed" else 1].view(np.uint32))
