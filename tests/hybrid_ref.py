"""NumPy float32 restatement of the hybrid control rule (csrc/mrca_hybrid_device.h), one robot at a time: every
+ - * / sqrt rounded on its own and in the header's order, so the result can be compared with the host build and the gfx950
kernel for EQUALITY.  It is written from the rule's text and shares no code with the header (the conversion of the PID
velocity to (v, omega) is restated here too).  The minima are np.min over float32 arrays without a NaN or a -0.0 (every range
has had + 0 added): they do not depend on the order of the beams, and neither does the count.

Everything is in the robot's frame: x ahead, y to the left."""
import numpy as np

import util as U  # noqa: F401  (puts the oracle on the path)
import mrca_oracle as O

f = np.float32
GOAL_RADIUS = f(0.5)
RANGE_MAX = f(6.0)
STILL = f(1e-4)
ZERO, ONE = f(0.0), f(1.0)
NORMAL, SIMPLE, EMERGENT, AT_GOAL = 0, 1, 2, -2

FIELDS = ["risk_dist", "stop_dist", "safe_scale", "corridor", "look", "front_cos", "v_pid", "k_omega", "max_speed"]
DEFAULTS = dict(risk_dist=0.6, stop_dist=0.3, safe_scale=0.75, corridor=1.0, look=6.0, front_cos=0.5, v_pid=1.0, k_omega=6.0,
                max_speed=1.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: f(v) for k, v in p.items()}


def pid_command(vx, vy, ms, k_omega):
    """the holonomic velocity (vx, vy) as (v, omega) of a forward-only differential drive whose heading is the x axis"""
    sp = np.sqrt(vx * vx + vy * vy)
    if sp < STILL:
        return ZERO, ZERO
    fwd = ONE * vx + ZERO * vy
    lat = ONE * vy - ZERO * vx
    v = (ms if fwd > ms else fwd) if fwd > ZERO else ZERO
    turn = k_omega * (lat / sp if fwd > ZERO else (ONE if lat >= ZERO else -ONE))
    w = -ONE if turn < -ONE else (ONE if turn > ONE else turn)
    return f(v), f(w)


def robot(p, goal, policy, row, bc, bs):
    """-> (cmd float32[2], mode, clear float32[3] = (d_min, d_front, d_block), n_block)"""
    with np.errstate(all="ignore"):
        gx, gy = f(goal[0]), f(goal[1])
        policy = np.asarray(policy, f)
        r = np.asarray(row, f) + ZERO
        bc, bs = np.asarray(bc, f), np.asarray(bs, f)
        d_min = r.min()
        front = bc >= p["front_cos"]
        d_front = min(r[front].min(), RANGE_MAX) if front.any() else RANGE_MAX
        gl = np.sqrt(gx * gx + gy * gy)
        if gl <= GOAL_RADIUS:
            return np.zeros(2, f), AT_GOAL, np.array([d_min, d_front, RANGE_MAX], f), 0
        ux, uy = gx / gl, gy / gl
        reach = gl if gl < p["look"] else p["look"]
        px, py = r * bc, r * bs
        t = px * ux + py * uy
        lat = px * uy - py * ux
        block = (r < RANGE_MAX) & (t >= ZERO) & (t <= reach) & (np.abs(lat) < p["corridor"])
        n_block = int(block.sum())
        d_block = r[block].min() if n_block else RANGE_MAX
        clear = np.array([d_min, d_front, d_block], f)
        if d_min < p["risk_dist"]:
            x = (d_front - p["stop_dist"]) / (p["risk_dist"] - p["stop_dist"])
            s = ZERO if not (x > ZERO) else (x if x < p["safe_scale"] else p["safe_scale"])
            cmd = policy.copy()
            cmd[0] = policy[0] * s
            return cmd, EMERGENT, clear, n_block
        if n_block == 0:
            v, w = pid_command(p["v_pid"] * ux, p["v_pid"] * uy, p["max_speed"], p["k_omega"])
            return np.array([v, w], f), SIMPLE, clear, n_block
        return policy.copy(), NORMAL, clear, n_block


def env_actions(p, goals, policy, rows, bc=None, bs=None):
    """every robot of an env from host copies of its fields -> (actions f32[N,2], mode i32[N], clear f32[N,3], n_block i32[N])"""
    rows = np.asarray(rows, f)
    N, B = rows.shape
    if bc is None:
        bc, bs = (np.ascontiguousarray(t, f) for t in O.beam_table(f, B))
    act, mode, clear, nb = np.zeros((N, 2), f), np.zeros(N, np.int32), np.zeros((N, 3), f), np.zeros(N, np.int32)
    for n in range(N):
        act[n], mode[n], clear[n], nb[n] = robot(p, goals[n], policy[n], rows[n], bc, bs)
    return act, mode, clear, nb
