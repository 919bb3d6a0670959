"""NumPy float32 / uint32 restatement of the scenario sampler's rule (csrc/mrca_scatter_device.h): the sequential definition as
plain loops over a world's robots, one separately rounded operation per line in the header's order, with the oracle's Philox,
u01 and wrap_angle -- and the cell field built from the dense map by brute-force dilation (nothing shared with the code under
test).  A robot's candidates are evaluated a chunk at a time; the least passing k of the first chunk that has one is the least
passing k."""
import numpy as np

import util as U

O = U.O
f32, u32 = np.float32, np.uint32
FIELDS = ("min_sep", "goal_sep", "goal_min", "goal_max", "clear_cells", "max_tries", "draw")
DEFAULTS = dict(min_sep=1.0, goal_sep=1.0, goal_min=5.0, goal_max=1.0e4, clear_cells=4, max_tries=1024, draw=0)    # mrca_scatter_default_params
STREAM_START, STREAM_GOAL = 3, 7
MAX_ROBOTS = 4096
CELL_LIMIT = f32(2.0 ** 30)
CHUNK = 96            # (no multiple of the kernel's 64 or 256 lanes, and none of them a multiple of it)


def params(**kw):
    """the library's defaults with ``kw`` set"""
    assert set(kw) <= set(FIELDS), kw
    return {**DEFAULTS, **kw}


def key_of(seed):
    return u32(seed & 0xFFFFFFFF), u32((seed >> 32) & 0xFFFFFFFF)


def cellfield(occ):
    """uint8[h, w]: per cell the Chebyshev distance to the nearest occupied cell, saturated at 255, cells beyond the map free"""
    occ = np.asarray(occ, bool)
    h, w = occ.shape
    out = np.full((h, w), 255, np.uint8)
    out[occ] = 0
    near = occ.copy()
    for d in range(1, 255):
        if near.all() or not near.any():
            break
        pad = np.zeros((h + 2, w + 2), bool)
        pad[1:-1, 1:-1] = near
        grown = np.zeros((h, w), bool)
        for dy in range(3):
            for dx in range(3):
                grown |= pad[dy:dy + h, dx:dx + w]
        out[grown & ~near] = d
        near = grown
    return out


def geometry(grid):
    """(x0, y0, inv_cell) as the env holds them"""
    return f32(grid.x0), f32(grid.y0), f32(1.0) / f32(grid.cell)


def candidates(box, gid, draw, ks, word, key):
    """candidates ``ks`` of robot ``gid`` in ``box`` (x0, y0, x1, y1) -> x, y, th float32[len(ks)]"""
    n = len(ks)
    w = O.philox4x32(np.full(n, gid, u32), np.full(n, draw, u32), np.asarray(ks, u32), np.full(n, word, u32), key[0], key[1])
    x0, y0, x1, y1 = (f32(v) for v in box)
    sx = x1 - x0
    sx = sx * O.u01(w[0], f32)
    x = x0 + sx
    sy = y1 - y0
    sy = sy * O.u01(w[1], f32)
    y = y0 + sy
    th = f32(2.0 * np.pi) * O.u01(w[2], f32)
    return x.astype(f32), y.astype(f32), O.wrap_angle(th, f32)


def clearance(cf, grid, x, y):
    """the clearance value per point (int64): the cell's byte; off the map the clamped cell's byte or the cell distance to it,
    whichever is more; 0 where the cell is no number"""
    h, w = cf.shape
    gx0, gy0, inv = geometry(grid)
    with np.errstate(all="ignore"):
        fx = x - gx0
        fx = np.floor(fx * inv)
        fy = y - gy0
        fy = np.floor(fy * inv)
        sane = (fx >= -CELL_LIMIT) & (fx <= CELL_LIMIT) & (fy >= -CELL_LIMIT) & (fy <= CELL_LIMIT)
    cx = np.where(sane, fx, 0).astype(np.int64)
    cy = np.where(sane, fy, 0).astype(np.int64)
    qx, qy = np.clip(cx, 0, w - 1), np.clip(cy, 0, h - 1)
    off = np.maximum(np.abs(cx - qx), np.abs(cy - qy))
    return np.where(sane, np.maximum(cf[qy, qx].astype(np.int64), off), 0)


def dist2(x, y, px, py):
    dx = x - f32(px)
    dy = y - f32(py)
    dx = dx * dx
    dy = dy * dy
    return dx + dy


def scatter_world(p, grid, cf, key, R, w, boxes):
    """world ``w`` -> poses f32[R,3], goals f32[R,2], tries i32[R,2]"""
    boxes = np.ascontiguousarray(boxes, f32).reshape(R, 8)
    min_sep, goal_sep, goal_min, goal_max = (f32(p[k]) for k in FIELDS[:4])
    clear_cells, max_tries, draw = int(p["clear_cells"]), int(p["max_tries"]), int(p["draw"])
    sep2 = (min_sep * min_sep, goal_sep * goal_sep)
    lo2, hi2 = goal_min * goal_min, goal_max * goal_max
    poses, goals, tries = np.zeros((R, 3), f32), np.zeros((R, 2), f32), np.zeros((R, 2), np.int32)
    for phase in (0, 1):
        placed = np.zeros((R, 2), f32)
        for i in range(R):
            gid = (w * R + i) & 0xFFFFFFFF
            box = boxes[i, 4 * phase: 4 * phase + 4]
            word = STREAM_GOAL if phase else STREAM_START
            found = -1
            for base in range(0, max_tries, CHUNK):
                ks = np.arange(base, min(base + CHUNK, max_tries))
                x, y, th = candidates(box, gid, draw, ks, word, key)
                ok = clearance(cf, grid, x, y) > clear_cells
                with np.errstate(all="ignore"):
                    if phase:
                        d2 = dist2(x, y, poses[i, 0], poses[i, 1])
                        ok &= (d2 >= lo2) & (d2 <= hi2)
                    if i:       # every j < i (elementwise float32: the same roundings as one j after the other)
                        ok &= ~(dist2(x[:, None], y[:, None], placed[None, :i, 0], placed[None, :i, 1]) < sep2[phase]).any(axis=1)
                if ok.any():
                    found = int(np.argmax(ok))
                    break
            at = found if found >= 0 else len(ks) - 1          # none: candidate max_tries - 1, the last of the last chunk
            placed[i] = x[at], y[at]
            if phase:
                goals[i] = x[at], y[at]
            else:
                poses[i] = x[at], y[at], th[at]
            tries[i, phase] = ks[found] + 1 if found >= 0 else -1
    return poses, goals, tries


def scatter(p, grid, seed, W, R, boxes, cf=None):
    """every world -> poses f32[W*R,3], goals f32[W*R,2], tries i32[W*R,2]"""
    cf = cellfield(grid.dense()) if cf is None else cf
    key = key_of(seed)
    parts = [scatter_world(p, grid, cf, key, R, w, boxes) for w in range(W)]
    return tuple(np.concatenate([q[k] for q in parts]) for k in range(3))
