"""The planner's line-of-sight rule (csrc/mrca_planner_device.h, LINE OF SIGHT; mrca_subgoals_los) restated in NumPy on top of
tests/planner_ref.py: the walk one step at a time with its cells kept, the supercover line in plain integers, the choice of m,
and the five outputs.  Nothing here is shared with the code under test."""
import numpy as np

import planner_ref as R

f32 = np.float32
LOS_FIELDS = ["reach"]
LOS_DEFAULTS = {"reach": 60}


def is_open(D, i, j):
    ph, pw = D.shape
    return 0 <= i < pw and 0 <= j < ph and int(D[j, i]) != R.INF


def visible(D, c0, c1):
    """the integer supercover line from cell c0 to cell c1 (McNeill's form): every cell entered is open, c0 is not tested, and
    where the line passes exactly through a lattice corner both side cells are open"""
    (i, j), (i1, j1) = c0, c1
    dx, dy = abs(i1 - i), abs(j1 - j)
    sx, sy = (1 if i1 > i else -1), (1 if j1 > j else -1)
    err = dx - dy
    dx, dy = 2 * dx, 2 * dy
    while (i, j) != (i1, j1):
        if err > 0:
            i, err = i + sx, err - dy
        elif err < 0:
            j, err = j + sy, err + dx
        else:
            if not (is_open(D, i + sx, j) and is_open(D, i, j + sy)):
                return False
            i, j, err = i + sx, j + sy, err + dx - dy
        if not is_open(D, i, j):
            return False
    return True


def walk_cells(D, blocked, seed, ci, cj, steps):
    """-> ([c_0 .. c_W], nocand): R.walk one step at a time"""
    cells = [(ci, cj)]
    for step in range(steps):
        ni, nj, nocand = R.walk(D, blocked, seed, cells[-1][0], cells[-1][1], 1)
        if nocand and step == 0:
            return cells, True
        if (ni, nj) == cells[-1]:
            break
        cells.append((ni, nj))
    return cells, False


def choose(D, cells, L):
    """-> (m, m_vis)"""
    W = len(cells) - 1
    m_vis = max([m for m in range(1, W + 1) if visible(D, cells[0], cells[m])], default=0)
    return max(m_vis, min(L, W)), m_vis


def subgoals_los(grid, p, reach, fields, goals, slot, pose, head_sc, env_goal, blocked=None):
    """the arguments of R.subgoals and the reach -> (local f32[N, 2], subgoal f32[N, 2], dist f32[N], status i32[N],
    ahead i32[N, 2] = (m, m_vis))"""
    s, L = p["stride"], p["lookahead"]
    blocked = R.blocked_mask(grid, s, p["inflate"]) if blocked is None else blocked
    N, G = len(pose), len(goals)
    local, sub = np.zeros((N, 2), f32), np.zeros((N, 2), f32)
    dist, status, ahead = np.zeros(N, f32), np.zeros(N, np.int32), np.zeros((N, 2), np.int32)
    unit = f32(f32(grid.cell) * f32(s))
    for n in range(N):
        x, y = f32(pose[n][0]), f32(pose[n][1])
        sl = int(slot[n])
        sub[n] = env_goal[n]
        dist[n] = np.inf
        c = R.plan_cell(grid, s, x, y)
        if not 0 <= sl < G:
            status[n] = R.NO_SLOT
        elif c is None:
            status[n] = R.NO_PATH
        else:
            D = fields[sl]
            seed = R.plan_cell(grid, s, goals[sl][0], goals[sl][1])
            d0 = int(D[c[1], c[0]])
            if d0 != R.INF:
                dist[n] = f32(d0) * f32(unit / f32(5.0))
            cells, nocand = walk_cells(D, blocked, seed, c[0], c[1], max(L, reach))
            if nocand:
                status[n] = R.NO_PATH
            else:
                m, m_vis = choose(D, cells, L)
                ahead[n] = (m, m_vis)
                ci, cj = cells[m]
                if int(D[cj, ci]) == 0:
                    status[n] = R.ON_GOAL
                    sub[n] = goals[sl]
                else:
                    status[n] = R.ON_PATH
                    sub[n] = (f32(grid.x0) + f32(f32(ci) + f32(0.5)) * unit, f32(grid.y0) + f32(f32(cj) + f32(0.5)) * unit)
        local[n] = R.local_of(sub[n][0], sub[n][1], x, y, head_sc[n][0], head_sc[n][1])
    return local, sub, dist, status, ahead
