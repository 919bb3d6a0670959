"""NumPy float32 restatement of the DWA baseline controller's rule (csrc/mrca_dwa_device.h): arrays of
np.float32 over robots, candidates and obstacle points, every + - * / sqrt rounded on its own and in the header's order, so the
result can be compared with the host build and the gfx950 kernel for EQUALITY.  (A minimum over points is taken with np.fmin:
the minimum of a set of non-negative numbers does not depend on the order, and like the header's ``d < m ? d : m`` it passes
over a NaN.)  Beside command, choice and score it returns diagnostics per robot: the obstacle points and the beams they came
from, and per candidate its admissibility, clearance and score.

Everything is in the robot's frame: x ahead, y to the left."""
import numpy as np

import util as U  # noqa: F401  (puts the oracle on the path)
import mrca_oracle as O

f = np.float32
DT = f(0.1)
GOAL_RADIUS = f(0.5)
RANGE_MAX = f(6.0)
SECTORS = 64
BLOCKED, AT_GOAL = -1, -2
ZERO, ONE = f(0.0), f(1.0)
INF = f(np.inf)

FIELDS = ["radius", "horizon", "obst_dist", "clear_cap", "max_speed", "max_omega", "acc_v", "acc_w", "w_goal", "w_heading", "w_clear",
          "w_speed", "steps", "nv", "nw"]
INTS = ("steps", "nv", "nw")
DEFAULTS = dict(radius=0.35, horizon=2.0, obst_dist=3.0, clear_cap=1.0, max_speed=1.0, max_omega=1.0, acc_v=10.0, acc_w=20.0,
                w_goal=1.0, w_heading=0.0, w_clear=0.2, w_speed=0.3, steps=10, nv=5, nw=21)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: (int(v) if k in INTS else f(v)) for k, v in p.items()}


def points(rows, bc, bs, obst_dist):
    """rows[N,B] -> (px[N,64], py[N,64], beam[N,64]): a sector's nearest return below min(obst_dist, 6), the lowest beam among
    equals; a sector without one has beam -1 and the point (+inf, 0)."""
    rows = np.asarray(rows, f)
    N, B = rows.shape
    per = B // SECTORS
    cut = obst_dist if obst_dist < RANGE_MAX else RANGE_MAX
    r = rows.reshape(N, SECTORS, per)
    counts = r < cut
    k = np.argmin(np.where(counts, r, INF), axis=2)                      # (the first of equal minima; -0.0 equals 0.0)
    valid = counts.any(axis=2)
    beam = np.where(valid, np.arange(SECTORS)[None, :] * per + k, -1)
    br = np.take_along_axis(r, k[..., None], 2)[..., 0] + ZERO          # (+ 0: a range of -0.0 is a 0)
    b = np.where(valid, beam, 0)
    px = np.where(valid, br * bc[b], INF).astype(f)
    py = np.where(valid, br * bs[b], ZERO).astype(f)
    return px, py, beam.astype(np.int32)


def clamp(x, lo, hi):
    """x into [lo, hi]; a NaN becomes lo"""
    return np.where(~(x > lo), lo, np.where(x < hi, x, hi)).astype(f)


def window(p, v0, w0):
    av, aw = p["acc_v"] * DT, p["acc_w"] * DT
    vhi = clamp(v0 + av, ZERO, p["max_speed"])
    vlo = clamp(v0 - av, ZERO, vhi)
    whi = clamp(w0 + aw, -p["max_omega"], p["max_omega"])
    wlo = clamp(w0 - aw, -p["max_omega"], whi)
    return vlo, vhi, wlo, whi


def sample(lo, hi, i, n):
    """lo, hi [N], i [C] -> [N,C]: sample i of n over [lo, hi], the lower half counted from lo, the upper half from hi"""
    lo, hi = lo[:, None], hi[:, None]
    if n == 1:
        return np.broadcast_to(hi, (hi.shape[0], len(i))).astype(f)
    span = hi - lo
    den = f(n - 1)
    lower = lo + span * (i.astype(f) / den)[None, :]
    upper = hi - span * ((n - 1 - i).astype(f) / den)[None, :]
    return np.where((2 * i < n - 1)[None, :], lower, upper).astype(f)


def ordered_bits(score):
    b = np.ascontiguousarray(score, f).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def env_actions(p, local_goal, speed, rows, robots=None):
    """Every robot of an env from host copies of its fields: local_goal[N,2], speed[N,2], rows[N,B] = the newest scan row.
    -> (actions f32[N,2], choice i32[N], score f32[N], diag); rows of robots not in ``robots`` (default: all) are NaN / 0 / NaN.
    diag: px, py [N,64], beam [N,64], and per candidate v, w, clear, score, admissible [N,C]."""
    local_goal, speed, rows = (np.ascontiguousarray(t, f) for t in (local_goal, speed, rows))
    N, B = rows.shape
    bc, bs = (np.asarray(t, f) for t in O.beam_table(f, B))
    steps, nv, nw = p["steps"], p["nv"], p["nw"]
    C = nv * nw
    with np.errstate(all="ignore"):
        px, py, beam = points(rows, bc, bs, p["obst_dist"])
        any_point = (beam >= 0).any(axis=1)
        gx, gy = local_goal[:, 0], local_goal[:, 1]
        gl = np.sqrt(gx * gx + gy * gy)
        at_goal = gl <= GOAL_RADIUS
        vlo, vhi, wlo, whi = window(p, speed[:, 0], speed[:, 1])
        dt = p["horizon"] / f(steps)
        c = np.arange(C)
        v = sample(vlo, vhi, c // nw, nv)
        w = sample(wlo, whi, c % nw, nw)
        x, y, th = np.zeros((N, C), f), np.zeros((N, C), f), np.zeros((N, C), f)
        s, co = np.zeros((N, C), f), np.ones((N, C), f)
        m = np.full((N, C), INF, f)
        for _ in range(steps):
            d = v * dt
            x = x + d * co
            y = y + d * s
            th = O.wrap_angle(th + w * dt, f)
            s, co = O.sincos(th, f)
            dx = x[:, :, None] - px[:, None, :]
            dy = y[:, :, None] - py[:, None, :]
            m = np.fmin(m, np.fmin.reduce(dx * dx + dy * dy, axis=2))
        clear = np.where(any_point[:, None], np.sqrt(m) - p["radius"], p["clear_cap"]).astype(f)
        ex, ey = gx[:, None] - x, gy[:, None] - y
        el = np.sqrt(ex * ex + ey * ey)
        progress = (gl[:, None] - el) / (p["max_speed"] * p["horizon"])
        align = np.where(el == ZERO, ONE, (co * ex + s * ey) / el).astype(f)
        cl = np.where(clear < p["clear_cap"], clear, p["clear_cap"]).astype(f)
        score = ((((p["w_goal"] * progress + p["w_heading"] * align) + p["w_clear"] * (cl / p["clear_cap"])) +
                  p["w_speed"] * (v / p["max_speed"])) + ZERO).astype(f)
        adm = (clear >= ZERO) & (score == score)
    key = np.where(adm, (ordered_bits(score).astype(np.uint64) << np.uint64(32)) | (~c.astype(np.uint32)).astype(np.uint64)[None, :],
                   np.uint64(0))
    best = key.argmax(axis=1)
    none = ~adm.any(axis=1)
    rows_ = np.arange(N)
    act = np.stack([v[rows_, best], w[rows_, best]], 1).astype(f)
    choice = best.astype(np.int32)
    sc = score[rows_, best].astype(f)
    turn = np.where(gy >= ZERO, p["max_omega"], -p["max_omega"]).astype(f)
    act[none] = np.stack([np.zeros(N, f), turn], 1)[none]
    choice[none], sc[none] = BLOCKED, ZERO
    act[at_goal], choice[at_goal], sc[at_goal] = ZERO, AT_GOAL, ZERO
    if robots is not None:
        skip = np.ones(N, bool)
        skip[list(robots)] = False
        act[skip], choice[skip], sc[skip] = np.nan, 0, np.nan
    diag = dict(px=px, py=py, beam=beam, v=v, w=w, clear=clear, score=score, admissible=adm, at_goal=at_goal, any_point=any_point)
    return act, choice, sc, diag
