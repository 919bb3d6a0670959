"""NumPy float32 restatement of the NH-ORCA baseline controller's rule (csrc/mrca_nhorca_device.h): per robot,
with np.float32 scalars -- every + - * / sqrt rounded on its own, in the header's order, so the result can be compared with the
host build and the gfx950 kernel for EQUALITY.  The constraints, the linear programs, the neighbour selection and the preferred
velocity are tests/orca_ref.py's; restated here: atan2_approx, the derived values, the heading lines, the two solves, the command
and the modes."""
import numpy as np

import orca_ref as R
import util as U  # noqa: F401  (puts the oracle on the path)
import mrca_oracle as O

f = np.float32
ZERO, ONE, HALF = f(0.0), f(1.0), f(0.5)
PI = f(3.14159265358979323846)
W_MAX = f(1.0)
STRAIGHT = f(1e-3)
HEADING_LINES = 2
MAX_NEIGHBORS = 46
TRACK, TURN, STILL, EVADE = 0, 1, 2, 3

FIELDS = R.FIELDS + ["track_error", "track_time"]
DEFAULTS = dict(R.DEFAULTS, jitter=0.3, track_error=0.05, track_time=0.3)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: (int(v) if k == "max_neighbors" else f(v)) for k, v in p.items()}


def sincos(a):
    s, c = O.sincos(f(a), f)
    return f(s), f(c)


def atan2_approx(y, x):
    y, x = f(y), f(x)
    ax, ay = abs(x), abs(y)
    mx, mn = (ax, ay) if ax > ay else (ay, ax)
    a = mn / mx if mx > ZERO else ZERO
    z = a * a
    r = ((f(-0.0464964749) * z + f(0.15931422)) * z - f(0.327622764)) * z * a + a
    r = f(1.57079637) - r if ay > ax else r
    r = f(3.14159274) - r if x < ZERO else r
    return -r if y < ZERO else r


def derive(p):
    """-> (sm, cm, u_cap, Rr)"""
    tw = p["track_time"] * W_MAX
    th_max = tw if tw < HALF * PI else HALF * PI
    sm, cm = sincos(th_max)
    sh, _ch = sincos(HALF * th_max)
    cap = p["track_error"] / (p["track_time"] * sh)
    return sm, cm, (p["max_speed"] if p["max_speed"] < cap else cap), p["radius"] + p["track_error"]


def heading_lines(s, c, sm, cm):
    """(left, right): through the origin"""
    return (ZERO, ZERO, -(c * cm - s * sm), -(s * cm + c * sm)), (ZERO, ZERO, c * cm + s * sm, s * cm - c * sm)


def inside(x, y, n, s, c, cm):
    return bool(c * x + s * y >= cm * n)


def side(x, y, s, c):
    return ONE if c * y - s * x >= ZERO else -ONE


def aim(s1x, s1y, ox, oy, s, c, cm):
    """-> (track, turn)"""
    n1 = np.sqrt(R.dot(s1x, s1y, s1x, s1y))
    if n1 >= R.STILL:
        if inside(s1x, s1y, n1, s, c, cm):
            return True, ZERO
        return False, side(s1x, s1y, s, c)
    no = np.sqrt(R.dot(ox, oy, ox, oy))
    if no > ZERO and not inside(ox, oy, no, s, c, cm):
        return False, side(ox, oy, s, c)
    return False, ZERO


def command(s2x, s2y, s, c, track, turn, ms, T):
    """-> ((v, omega), mode)"""
    s2x, s2y, s, c, turn, ms, T = (f(v) for v in (s2x, s2y, s, c, turn, ms, T))
    u = np.sqrt(R.dot(s2x, s2y, s2x, s2y))
    if u < R.STILL:
        return (ZERO, turn), (TURN if turn != ZERO else STILL)
    fwd = c * s2x + s * s2y
    lat = c * s2y - s * s2x
    th = atan2_approx(lat, fwd)
    om = th / T
    w = -W_MAX if om < -W_MAX else (W_MAX if om > W_MAX else om)
    arc = u if abs(th) < STRAIGHT else ((u * (HALF * th)) * (u + fwd)) / lat
    v = (ms if arc > ms else arc) if arc > ZERO else ZERO
    return (v, w), (TRACK if track else EVADE)


def solve(p, lines, n_static, s, c, ox, oy, s1=None):
    """lines = the static ones, then the robots' (WITHOUT the heading lines), built with the grown radius; s1: the free solve's
    velocity where the caller has it.  -> (cmd, S2, mode, diag)"""
    sm, cm, u_cap, _rr = derive(p)
    if s1 is None:
        s1, _d = R.solve(lines, n_static, p["max_speed"], ox, oy)
    with np.errstate(all="ignore"):
        track, turn = aim(s1[0], s1[1], ox, oy, s, c, cm)
    all_lines = list(heading_lines(s, c, sm, cm)) + list(lines)
    qx, qy = (ox, oy) if track else (ZERO, ZERO)
    (rx, ry), diag = R.solve(all_lines, HEADING_LINES + n_static, u_cap, qx, qy)
    with np.errstate(all="ignore"):
        cmd, mode = command(rx, ry, s, c, track, turn, p["max_speed"], p["track_time"])
    diag.update(s1=s1, track=track, turn=turn, lines=all_lines, n_static=n_static)
    return cmd, (rx, ry), mode, diag


def robot(p, local, gid, k0, k1, pose, sincos_rows, speed_gt, goal, ranges, hit_robot, bc, bs):
    """The whole rule for robot ``local`` of one world (orca_ref.robot's arguments).  -> (cmd, S2, mode, diag)"""
    _sm, _cm, _cap, rr = derive(p)
    grown = dict(p, radius=rr)
    # plain ORCA with the grown radius: its lines are this rule's, and its velocity is the free solve's
    _cmd, s1, d = R.robot(grown, local, gid, k0, k1, pose, sincos_rows, speed_gt, goal, ranges, hit_robot, bc, bs)
    with np.errstate(all="ignore"):
        ox, oy = R.pref_velocity(p, gid, k0, k1, f(pose[local][0]), f(pose[local][1]), goal[0], goal[1])
    s, c = f(sincos_rows[local][0]), f(sincos_rows[local][1])
    cmd, v, mode, diag = solve(p, d["lines"], d["n_static"], s, c, ox, oy, s1=s1)
    diag.update(branches=d["branches"], free=d, o=(ox, oy))
    return cmd, v, mode, diag


def env_actions(p, Rn, seed, pose, speed_gt, goal, rows, hit_robot, robots=None):
    """Every robot of an env from host copies of its fields (orca_ref.env_actions' arguments).
    -> (actions f32[N,2], vel f32[N,2], mode i32[N], {n: diag}); ``robots``: only these (other rows stay NaN / -1)."""
    N, B = rows.shape
    bc, bs = O.beam_table(f, B)
    s, c = O.sincos(pose[:, 2], f)
    sc = np.stack([s, c], 1).astype(f)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    act = np.full((N, 2), np.nan, f)
    vel = np.full((N, 2), np.nan, f)
    mode = np.full(N, -1, np.int32)
    diags = {}
    for n in (range(N) if robots is None else robots):
        w = n // Rn
        sl = slice(w * Rn, (w + 1) * Rn)
        cmd, v, m, d = robot(p, n - w * Rn, n, k0, k1, pose[sl], sc[sl], speed_gt[sl], goal[n], rows[n], hit_robot[n], bc, bs)
        act[n], vel[n], mode[n] = cmd, v, m
        diags[n] = d
    return act, vel, mode, diags
