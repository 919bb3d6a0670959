"""The global planner's rule (csrc/mrca_planner_device.h) restated in NumPy and heapq: the blocked mask from the occupancy grid
itself (no distance field), the goal field by Dijkstra with the 5 / 7 costs and the no-corner-cutting rule, the walk, and the four
outputs in float32 with the header's order of operations.  Nothing here is shared with the code under test."""
import heapq

import numpy as np

f32 = np.float32
INF = 0xFFFFFFFF
FIELDS = ["stride", "inflate", "lookahead", "max_rounds"]
DEFAULTS = {"stride": 2, "inflate": 7, "lookahead": 15, "max_rounds": 0}
# E, NE, N, NW, W, SW, S, SE (N is +y)
DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
COST = [5, 7, 5, 7, 5, 7, 5, 7]
ON_GOAL, ON_PATH, NO_SLOT, NO_PATH = 1, 0, -1, -2


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def grid_shape(grid, s):
    return -(-grid.width // s), -(-grid.height // s)            # PW, PH


def blocked_mask(grid, s, inflate):
    """bool[PH, PW]: a planning cell is blocked iff an occupied map cell lies within Chebyshev distance `inflate` of one of its
    map cells (cells beyond the map are free)."""
    occ = grid.dense()
    h, w = occ.shape
    pad = np.zeros((h + 2 * inflate, w + 2 * inflate), bool)
    pad[inflate:inflate + h, inflate:inflate + w] = occ
    near = np.zeros((h, w), bool)
    for dy in range(2 * inflate + 1):           # a box dilation, one axis after the other
        near |= pad[dy:dy + h, inflate:inflate + w]
    pad[:] = False
    pad[inflate:inflate + h, inflate:inflate + w] = near
    near = np.zeros((h, w), bool)
    for dx in range(2 * inflate + 1):
        near |= pad[inflate:inflate + h, dx:dx + w]
    pw, ph = grid_shape(grid, s)
    big = np.zeros((ph * s, pw * s), bool)
    big[:h, :w] = near
    return big.reshape(ph, s, pw, s).any(axis=(1, 3))


def map_cell(grid, x, y):
    """the env's rule in float32 -> (ix, iy) or None (off grid)"""
    fx = np.floor((f32(x) - f32(grid.x0)) * (f32(1.0) / f32(grid.cell)))
    fy = np.floor((f32(y) - f32(grid.y0)) * (f32(1.0) / f32(grid.cell)))
    if not (fx >= 0 and fx < grid.width and fy >= 0 and fy < grid.height):
        return None
    return int(fx), int(fy)


def plan_cell(grid, s, x, y):
    c = map_cell(grid, x, y)
    return None if c is None else (c[0] // s, c[1] // s)


def allowed(blocked, seed, ci, cj, k):
    """may a path step from (ci, cj) in direction k?  The seed counts as unblocked."""
    ph, pw = blocked.shape
    free = lambda i, j: 0 <= i < pw and 0 <= j < ph and (not blocked[j, i] or (i, j) == seed)
    dx, dy = DIRS[k]
    if not free(ci + dx, cj + dy):
        return False
    return True if not (k & 1) else free(ci + dx, cj) and free(ci, cj + dy)


def goal_field(grid, p, goal, blocked=None):
    """uint32[PH, PW]: Dijkstra from the goal's planning cell"""
    s = p["stride"]
    blocked = blocked_mask(grid, s, p["inflate"]) if blocked is None else blocked
    ph, pw = blocked.shape
    D = np.full((ph, pw), INF, np.uint64)
    seed = plan_cell(grid, s, goal[0], goal[1])
    if seed is None:
        return D.astype(np.uint32)
    D[seed[1], seed[0]] = 0
    heap = [(0, seed[0], seed[1])]
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > D[j, i]:
            continue
        for k in range(8):
            # the step n -> c of a path towards the seed, seen from c = (i, j): direction k out of c is allowed iff its reverse out
            # of n is (the two squeezed cells are the same)
            ni, nj = i + DIRS[k][0], j + DIRS[k][1]
            if not (0 <= ni < pw and 0 <= nj < ph) or (blocked[nj, ni] and (ni, nj) != seed):
                continue
            if not allowed(blocked, seed, ni, nj, (k + 4) & 7):
                continue
            nd = d + COST[k]
            if nd < D[nj, ni]:
                D[nj, ni] = nd
                heapq.heappush(heap, (nd, ni, nj))
    return D.astype(np.uint32)


def walk(D, blocked, seed, ci, cj, L):
    """-> (ci, cj, nocand): where the walk ends"""
    ph, pw = D.shape
    for step in range(L):
        dc = int(D[cj, ci])
        if dc == 0:
            break
        escape = dc == INF or (blocked[cj, ci] and (ci, cj) != seed)
        best = None
        for k in range(8):
            ni, nj = ci + DIRS[k][0], cj + DIRS[k][1]
            if not (0 <= ni < pw and 0 <= nj < ph) or int(D[nj, ni]) == INF:
                continue
            if not escape and not allowed(blocked, seed, ci, cj, k):
                continue
            key = (int(D[nj, ni]) + COST[k], k)
            if best is None or key < best:
                best = key
        if best is None:
            return ci, cj, step == 0
        k = best[1]
        if not best[0] - COST[k] < dc:
            break
        ci, cj = ci + DIRS[k][0], cj + DIRS[k][1]
    return ci, cj, False


def local_of(px, py, x, y, sn, cs):
    gx, gy = f32(px) - f32(x), f32(py) - f32(y)
    return f32(gx * f32(cs)) + f32(gy * f32(sn)), f32(gy * f32(cs)) - f32(gx * f32(sn))


def subgoals(grid, p, fields, goals, slot, pose, head_sc, env_goal, blocked=None):
    """fields uint32[G, PH, PW], goals f32[G, 2], slot int[N], pose f32[N, 3], head_sc f32[N, 2] (sine, cosine), env_goal
    f32[N, 2] -> (local f32[N, 2], subgoal f32[N, 2], dist f32[N], status i32[N])"""
    s, L = p["stride"], p["lookahead"]
    blocked = blocked_mask(grid, s, p["inflate"]) if blocked is None else blocked
    N, G = len(pose), len(goals)
    local, sub = np.zeros((N, 2), f32), np.zeros((N, 2), f32)
    dist, status = np.zeros(N, f32), np.zeros(N, np.int32)
    unit = f32(f32(grid.cell) * f32(s))
    for n in range(N):
        x, y = f32(pose[n][0]), f32(pose[n][1])
        sl = int(slot[n])
        sub[n] = env_goal[n]
        dist[n] = np.inf
        c = plan_cell(grid, s, x, y)
        if not 0 <= sl < G:
            status[n] = NO_SLOT
        elif c is None:
            status[n] = NO_PATH
        else:
            D = fields[sl]
            seed = plan_cell(grid, s, goals[sl][0], goals[sl][1])
            d0 = int(D[c[1], c[0]])
            if d0 != INF:
                dist[n] = f32(d0) * f32(unit / f32(5.0))
            ci, cj, nocand = walk(D, blocked, seed, c[0], c[1], L)
            if nocand:
                status[n] = NO_PATH
            elif int(D[cj, ci]) == 0:
                status[n] = ON_GOAL
                sub[n] = goals[sl]
            else:
                status[n] = ON_PATH
                sub[n] = (f32(grid.x0) + f32(f32(ci) + f32(0.5)) * unit, f32(grid.y0) + f32(f32(cj) + f32(0.5)) * unit)
        local[n] = local_of(sub[n][0], sub[n][1], x, y, head_sc[n][0], head_sc[n][1])
    return local, sub, dist, status
