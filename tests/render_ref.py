"""NumPy float32 GATHER restatement of the renderer's rules (csrc/mrca_render_device.h) for
tests/test_render_host.py and tests/test_gpu_render.py: for every pixel the maximum over the map, all goals and all robots --
the opposite loop order of the library's scatter (per robot, a pixel box), written from the rules' text with every step a
separately rounded float32 operation.  Also the documented palette as a table."""
import numpy as np

F32 = np.float32
HALF_LEN, HALF_WID, NOSE_U, GOAL_R2 = F32(0.22), F32(0.19), F32(0.11), F32(0.0625)
MAP, GOALS, BODIES, BEAMS = 1, 2, 4, 8
L_MAP, L_GOAL, L_BEAM_WALL, L_BEAM_ROBOT, L_BODY, L_NOSE = 1, 2, 3, 4, 5, 6

# DESIGN.md 5.11, the palette table
BACKGROUND, MAP_RGB, TRAIL_RGB = (255, 255, 255), (32, 32, 32), (200, 200, 200)
BEAM_WALL_RGB, BEAM_ROBOT_RGB, CRASHED_RGB, REACHED_RGB = (255, 165, 0), (211, 0, 211), (220, 0, 0), (0, 170, 0)
HUES = [(31, 119, 180), (255, 127, 14), (23, 90, 138), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127),
        (188, 189, 34), (23, 190, 207), (57, 74, 156), (140, 121, 49), (99, 158, 107), (123, 57, 148), (231, 181, 74),
        (148, 81, 165), (90, 132, 132)]


def frame(view, W, H):
    """view = (cx, cy, m_per_px) -> x of the left edge, y of the top edge, m, the pixel centres' x[W] and y[H]."""
    cx, cy, m = (F32(v) for v in view)
    x0 = cx - (F32(0.5) * F32(W)) * m
    y1 = cy + (F32(0.5) * F32(H)) * m
    wx = x0 + (np.arange(W, dtype=F32) + F32(0.5)) * m
    wy = y1 - (np.arange(H, dtype=F32) + F32(0.5)) * m
    return x0, y1, m, wx, wy


def pixel_of(view, W, H, x, y):
    """(col, row) of the pixel containing (x, y), or None outside the image."""
    x0, y1, m, _, _ = frame(view, W, H)
    with np.errstate(all="ignore"):
        fc = np.floor((F32(x) - x0) / m)
        fr = np.floor((y1 - F32(y)) / m)
    if fc >= 0 and fc < W and fr >= 0 and fr < H:
        return int(fc), int(fr)
    return None


def map_layer(view, W, H, grid):
    _, _, _, wx, wy = frame(view, W, H)
    inv_cell = F32(1.0) / F32(grid.cell)
    fx = np.floor((wx - F32(grid.x0)) * inv_cell)
    fy = np.floor((wy - F32(grid.y0)) * inv_cell)
    okx = (fx >= 0) & (fx < grid.width)
    oky = (fy >= 0) & (fy < grid.height)
    out = np.zeros((H, W), bool)
    out[np.ix_(oky, okx)] = grid.dense()[np.ix_(fy[oky].astype(int), fx[okx].astype(int))]
    return out


def gather_ids(view, W, H, layers, grid, pose_xy, sincos, goals):
    """uint32[H,W]: layer << 24 | index, the maximum over everything that covers the pixel's centre."""
    _, _, _, wx, wy = frame(view, W, H)
    WX, WY = np.meshgrid(wx, wy)
    ids = np.zeros((H, W), np.uint32)

    def put(mask, layer, i):
        ids[mask] = np.maximum(ids[mask], np.uint32(layer << 24 | i))

    def put_pixel(x, y, layer, i):
        p = pixel_of(view, W, H, x, y)
        if p is not None:
            ids[p[1], p[0]] = max(ids[p[1], p[0]], np.uint32(layer << 24 | i))

    if layers & MAP and grid is not None:
        put(map_layer(view, W, H, grid), L_MAP, 0)
    for i in range(len(pose_xy)):
        if layers & GOALS:
            dx, dy = WX - F32(goals[i][0]), WY - F32(goals[i][1])
            put(dx * dx + dy * dy <= GOAL_R2, L_GOAL, i)
            put_pixel(goals[i][0], goals[i][1], L_GOAL, i)
        if layers & BODIES:
            s, c = F32(sincos[i][0]), F32(sincos[i][1])
            dx, dy = WX - F32(pose_xy[i][0]), WY - F32(pose_xy[i][1])
            u = dx * c + dy * s
            v = dy * c - dx * s
            body = (np.abs(u) <= HALF_LEN) & (np.abs(v) <= HALF_WID)
            put(body, L_BODY, i)
            put(body & (u >= NOSE_U), L_NOSE, i)
            put_pixel(pose_xy[i][0], pose_xy[i][1], L_BODY, i)
    return ids


def trail_marks(view, W, H, pose_xy, trail=None):
    """max(trail, index + 1) at the pixel containing every robot's centre."""
    trail = np.zeros((H, W), np.uint32) if trail is None else trail.copy()
    for i, (x, y) in enumerate(pose_xy):
        p = pixel_of(view, W, H, x, y)
        if p is not None:
            trail[p[1], p[0]] = max(trail[p[1], p[0]], i + 1)
    return trail


def _tint(c):
    return tuple((v + 255) // 2 for v in c)


def _shade(c):
    return tuple(v // 2 for v in c)


def _dim(c):
    return tuple(v // 4 + 144 for v in c)


def colour(layer, index, trail=0, crashed=0, first_result=0, live=1):
    """One pixel of the documented palette."""
    if layer == 0:
        return TRAIL_RGB if trail else BACKGROUND
    if layer == L_MAP:
        return MAP_RGB
    if layer == L_GOAL:
        return _tint(HUES[index % 16])
    if layer == L_BEAM_WALL:
        return BEAM_WALL_RGB
    if layer == L_BEAM_ROBOT:
        return BEAM_ROBOT_RGB
    c = HUES[index % 16]
    if crashed:
        c = CRASHED_RGB
    elif first_result == 1:
        c = REACHED_RGB
    elif not live:
        c = _dim(c)
    return _shade(c) if layer == L_NOSE else c


def resolve(ids, trail, crashed, first_result, live):
    """uint8[H,W,3] of one view; crashed / first_result / live: the viewed world's robots, by local index."""
    H, W = ids.shape
    out = np.zeros((H, W, 3), np.uint8)
    trail = np.zeros_like(ids) if trail is None else trail
    keys = np.unique(np.stack([ids.ravel(), (trail.ravel() != 0).astype(np.uint32)], 1), axis=0)
    for k, t in keys:
        layer, i = int(k) >> 24, int(k) & 0xFFFFFF
        st = (crashed[i], first_result[i], live[i]) if layer >= L_BODY else (0, 0, 1)
        out[(ids == k) & ((trail != 0) == bool(t))] = colour(layer, i, int(t), *st)
    return out
