"""NumPy float32 restatement of the ORCA baseline controller's rule (csrc/mrca_orca_device.h): per robot, with
plain sequential loops over np.float32 scalars -- every + - * / sqrt rounded on its own, in the header's order, so the result
can be compared with the host build and the gfx950 kernel for EQUALITY.  Beside the command and the velocity it returns
diagnostics: which branch each constraint took, whether LP2 fell short, whether LP3 changed the result.

A line is a tuple (px, py, dx, dy) of np.float32: the directed line through p along d; v satisfies it when
det(d, p - v) <= 0."""
import numpy as np

import util as U  # noqa: F401  (puts the oracle on the path)
import mrca_oracle as O

f = np.float32
EPS = f(1e-5)
STILL = f(1e-4)
DT = f(0.1)
GOAL_RADIUS = f(0.5)
SECTORS = 16
STREAM_ORCA = 2
CIRCLE, LEG_LEFT, LEG_RIGHT, OVERLAP = 0, 1, 2, 3
ZERO, ONE, TWO = f(0.0), f(1.0), f(2.0)

FIELDS = ["radius", "neighbor_dist", "time_horizon", "time_horizon_obst", "obst_dist", "v_pref", "max_speed", "responsibility",
          "k_omega", "jitter", "max_neighbors"]
DEFAULTS = dict(radius=0.35, neighbor_dist=6.0, time_horizon=2.0, time_horizon_obst=1.5, obst_dist=3.0, v_pref=1.0, max_speed=1.0,
                responsibility=0.5, k_omega=6.0, jitter=0.0, max_neighbors=10)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: (int(v) if k == "max_neighbors" else f(v)) for k, v in p.items()}


def det(ax, ay, bx, by):
    return ax * by - ay * bx


def dot(ax, ay, bx, by):
    return ax * bx + ay * by


def violation(line, vx, vy):
    px, py, dx, dy = line
    return det(dx, dy, px - vx, py - vy)


def constraint(rpx, rpy, rvx, rvy, vx, vy, R, inv_t, resp):
    """-> (line, branch)"""
    rpx, rpy, rvx, rvy, vx, vy, R, inv_t, resp = (f(v) for v in (rpx, rpy, rvx, rvy, vx, vy, R, inv_t, resp))
    dist2 = dot(rpx, rpy, rpx, rpy)
    R2 = R * R
    it = inv_t
    if dist2 <= R2:
        it = ONE / DT
        branch, circle = OVERLAP, True
        wx, wy = rvx - it * rpx, rvy - it * rpy
        w2 = dot(wx, wy, wx, wy)
    else:
        wx, wy = rvx - it * rpx, rvy - it * rpy
        w2 = dot(wx, wy, wx, wy)
        d1 = dot(wx, wy, rpx, rpy)
        circle = bool(d1 < ZERO and d1 * d1 > R2 * w2)
        branch = CIRCLE
    if circle:
        wl = np.sqrt(w2)
        nx, ny = (ONE, ZERO) if wl == ZERO else (wx / wl, wy / wl)
        dx, dy = ny, -nx
        m = R * it - wl
        ux, uy = m * nx, m * ny
    else:
        leg = np.sqrt(dist2 - R2)
        if det(rpx, rpy, wx, wy) > ZERO:
            dx = (rpx * leg - rpy * R) / dist2
            dy = (rpx * R + rpy * leg) / dist2
            branch = LEG_LEFT
        else:
            dx = -((rpx * leg + rpy * R) / dist2)
            dy = -((-rpx * R + rpy * leg) / dist2)
            branch = LEG_RIGHT
        d2 = dot(rvx, rvy, dx, dy)
        ux, uy = d2 * dx - rvx, d2 * dy - rvy
    return (vx + resp * ux, vy + resp * uy, dx, dy), branch


def lp1(lines, k, ms, ox, oy, dir_opt):
    """-> (ok, (rx, ry) or None, failed by the parallel-line rule)"""
    px, py, dx, dy = lines[k]
    d = dot(px, py, dx, dy)
    disc = (d * d + ms * ms) - dot(px, py, px, py)
    if disc < ZERO:
        return False, None, False
    sq = np.sqrt(disc)
    tl, tr = -d - sq, -d + sq
    for j in range(k):
        jpx, jpy, jdx, jdy = lines[j]
        den = det(dx, dy, jdx, jdy)
        num = det(jdx, jdy, px - jpx, py - jpy)
        if abs(den) <= EPS:
            if num < ZERO:
                return False, None, True
            continue
        t = num / den
        if den >= ZERO:
            tr = t if t < tr else tr
        else:
            tl = t if t > tl else tl
    tl, tr = tl + ZERO, tr + ZERO
    if tl > tr:
        return False, None, False
    if dir_opt:
        t = tr if dot(ox, oy, dx, dy) > ZERO else tl
    else:
        t = dot(dx, dy, ox - px, oy - py)
        t = tl if t < tl else (tr if t > tr else t)
    return True, (px + t * dx, py + t * dy), False


def lp2(lines, ms, ox, oy, dir_opt, diag=None):
    """-> (k, (rx, ry)): k = len(lines) when every line holds"""
    if dir_opt:
        rx, ry = ox * ms, oy * ms
    else:
        o2 = dot(ox, oy, ox, oy)
        if o2 > ms * ms:
            ol = np.sqrt(o2)
            rx, ry = (ox * ms) / ol, (oy * ms) / ol
        else:
            rx, ry = ox, oy
    for k in range(len(lines)):
        if violation(lines[k], rx, ry) > ZERO:
            ok, res, par = lp1(lines, k, ms, ox, oy, dir_opt)
            if diag is not None and par:
                diag["parallel_fail"] = diag.get("parallel_fail", 0) + 1
            if not ok:
                return k, (rx, ry)
            rx, ry = res
    return len(lines), (rx, ry)


def project(li, lj):
    ipx, ipy, idx, idy = li
    jpx, jpy, jdx, jdy = lj
    D = det(idx, idy, jdx, jdy)
    if abs(D) <= EPS:
        if dot(idx, idy, jdx, jdy) > ZERO:
            return None
        px, py = (ipx + jpx) / TWO, (ipy + jpy) / TWO
    else:
        t = det(jdx, jdy, ipx - jpx, ipy - jpy) / D
        px, py = ipx + t * idx, ipy + t * idy
    ex, ey = jdx - idx, jdy - idy
    el = np.sqrt(dot(ex, ey, ex, ey))
    return (px, py, ex / el, ey / el)


def lp3(lines, n_static, begin, ms, rx, ry):
    distance = ZERO
    for i in range(begin, len(lines)):
        if violation(lines[i], rx, ry) > distance:
            proj = list(lines[:n_static])
            for j in range(n_static, i):
                p = project(lines[i], lines[j])
                if p is not None:
                    proj.append(p)
            k, res = lp2(proj, ms, -lines[i][3], lines[i][2], True)
            if k == len(proj):
                rx, ry = res
            distance = violation(lines[i], rx, ry)
    return rx, ry


def solve(lines, n_static, ms, ox, oy):
    """-> ((rx, ry), diag)"""
    diag = {"parallel_fail": 0}
    ms, ox, oy = f(ms), f(ox), f(oy)
    with np.errstate(all="ignore"):
        k, (rx, ry) = lp2(lines, ms, ox, oy, False, diag)
        diag["lp2_short"] = k < len(lines)
        bx, by = rx, ry
        if k < len(lines):
            rx, ry = lp3(lines, n_static, k, ms, rx, ry)
        diag["lp3_changed"] = bool(k < len(lines) and (bx != rx or by != ry))
    return (rx, ry), diag


def sectors(ranges, hit_robot, obst_dist):
    """-> [(range, beam)] per sector, beam -1 where the sector gives no constraint"""
    per = len(ranges) // SECTORS
    out = []
    for s in range(SECTORS):
        best, bb = f(np.inf), -1
        for b in range(s * per, (s + 1) * per):
            if (not hit_robot[b]) and ranges[b] < obst_dist and ranges[b] < best:
                best, bb = f(ranges[b]), b
        out.append((best, bb))
    return out


def neighbours(xy, local, neighbor_dist, max_neighbors):
    """indices of the kept neighbours, nearest first, ties by index"""
    nd2 = f(neighbor_dist) * f(neighbor_dist)
    keys = []
    for j in range(len(xy)):
        dx, dy = f(xy[j][0]) - f(xy[local][0]), f(xy[j][1]) - f(xy[local][1])
        d2 = dot(dx, dy, dx, dy)
        if j != local and d2 < nd2:
            keys.append((d2, j))
    keys.sort()
    return [j for _d, j in keys[:max_neighbors]]


def pref_velocity(p, gid, k0, k1, px, py, gx, gy):
    dx, dy = f(gx) - f(px), f(gy) - f(py)
    dist = np.sqrt(dot(dx, dy, dx, dy))
    if dist <= GOAL_RADIUS:
        return ZERO, ZERO
    x, y = (p["v_pref"] * dx) / dist, (p["v_pref"] * dy) / dist
    if p["jitter"] != ZERO:
        r = O.philox4x32(gid, 0, 0, STREAM_ORCA, k0, k1)[0]
        a = p["jitter"] * (TWO * f(O.u01(r, f)) - ONE)
        sa, ca = (f(v) for v in O.sincos(a, f))
        x, y = ca * x - sa * y, sa * x + ca * y
    return x, y


def command(vx, vy, s, c, ms, k_omega):
    vx, vy, s, c, ms, k_omega = (f(v) for v in (vx, vy, s, c, ms, k_omega))
    sp = np.sqrt(dot(vx, vy, vx, vy))
    if sp < STILL:
        return ZERO, ZERO
    fwd = c * vx + s * vy
    lat = c * vy - s * vx
    v = (ms if fwd > ms else fwd) if fwd > ZERO else ZERO
    turn = k_omega * (lat / sp if fwd > ZERO else (ONE if lat >= ZERO else -ONE))
    w = -ONE if turn < -ONE else (ONE if turn > ONE else turn)
    return v, w


def robot(p, local, gid, k0, k1, pose, sincos, speed_gt, goal, ranges, hit_robot, bc, bs):
    """The whole rule for robot ``local`` of one world (pose[R,3], sincos[R,2] = (sin, cos), speed_gt[R,2]; goal, ranges,
    hit_robot: this robot's).  -> (cmd (v, w), vel (vx, vy), diag)"""
    with np.errstate(all="ignore"):
        px, py = f(pose[local][0]), f(pose[local][1])
        s, c = f(sincos[local][0]), f(sincos[local][1])
        sp = f(speed_gt[local][0])
        vx, vy = sp * c, sp * s
        ox, oy = pref_velocity(p, gid, k0, k1, px, py, goal[0], goal[1])
        lines, branches = [], []
        inv_to = ONE / p["time_horizon_obst"]
        for r, b in sectors(ranges, hit_robot, p["obst_dist"]):
            if b < 0:
                continue
            rx = r * (c * f(bc[b]) - s * f(bs[b]))
            ry = r * (s * f(bc[b]) + c * f(bs[b]))
            line, br = constraint(rx, ry, vx, vy, vx, vy, p["radius"], inv_to, ONE)
            lines.append(line)
            branches.append(br)
        n_static = len(lines)
        inv_t = ONE / p["time_horizon"]
        for j in neighbours(pose[:, :2], local, p["neighbor_dist"], p["max_neighbors"]):
            sj = f(speed_gt[j][0])
            vjx, vjy = sj * f(sincos[j][1]), sj * f(sincos[j][0])
            line, br = constraint(f(pose[j][0]) - px, f(pose[j][1]) - py, vx - vjx, vy - vjy, vx, vy, TWO * p["radius"], inv_t,
                                  p["responsibility"])
            lines.append(line)
            branches.append(br)
    (rx, ry), diag = solve(lines, n_static, p["max_speed"], ox, oy)
    with np.errstate(all="ignore"):
        cmd = command(rx, ry, s, c, p["max_speed"], p["k_omega"])
    diag.update(branches=branches, n_static=n_static, lines=lines)
    return cmd, (rx, ry), diag


def env_actions(p, R, seed, pose, speed_gt, goal, rows, hit_robot, robots=None):
    """Every robot of an env from host copies of its fields: pose[N,3], speed_gt[N,2], goal[N,2], rows[N,B] = the newest scan
    of every robot, hit_robot[N,B] (bool).  The head record is sincos_det of the stored heading.
    -> (actions f32[N,2], vel f32[N,2], [diag]); ``robots``: only these indices (the other rows stay NaN)."""
    N, B = rows.shape
    bc, bs = O.beam_table(f, B)
    s, c = O.sincos(pose[:, 2], f)
    sincos = np.stack([s, c], 1).astype(f)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    act = np.full((N, 2), np.nan, f)
    vel = np.full((N, 2), np.nan, f)
    diags = {}
    for n in (range(N) if robots is None else robots):
        w = n // R
        sl = slice(w * R, (w + 1) * R)
        cmd, v, d = robot(p, n - w * R, n, k0, k1, pose[sl], sincos[sl], speed_gt[sl], goal[n], rows[n], hit_robot[n], bc, bs)
        act[n], vel[n] = cmd, v
        diags[n] = d
    return act, vel, diags
