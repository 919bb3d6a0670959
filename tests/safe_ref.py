"""NumPy float32 restatement of hybrid control in the paper's form (csrc/mrca_safe_device.h): the plan, the
commit and the scan the safe policy sees.  Written from the rule's text: the plan asks tests/hybrid_ref.py (the restatement of
the rule it stands on) with a ZERO command for the mode, the clearances and the PID command; nothing comes from the new
header.  Every step is a comparison, a copy or one float32 multiply, so the results can be compared for EQUALITY."""
import numpy as np

import hybrid_ref as R

f = np.float32
RANGE_MAX = f(6.0)
ZERO, ONE = f(0.0), f(1.0)

FIELDS = ["scan_scale", "v_cap"]
DEFAULTS = dict(scan_scale=0.3, v_cap=0.75)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: f(v) for k, v in p.items()}


def plan_robot(p, sp, goal, row, bc, bs):
    """-> (mode, scale float32, pid float32[2], clear float32[3])"""
    cmd, mode, clear, _nb = R.robot(p, goal, np.zeros(2, f), row, bc, bs)
    scale = sp["scan_scale"] if mode == R.EMERGENT else ONE
    pid = cmd.astype(f) if mode == R.SIMPLE else np.zeros(2, f)
    return mode, f(scale), pid, clear


def plan(p, sp, goals, rows, bc=None, bs=None):
    """every robot of an env from host copies of its fields -> (mode i32[N], scale f32[N], pid f32[N,2], clear f32[N,3])"""
    rows = np.asarray(rows, f)
    N, B = rows.shape
    if bc is None:
        bc, bs = (np.ascontiguousarray(t, f) for t in R.O.beam_table(f, B))
    mode, scale, pid, clear = np.zeros(N, np.int32), np.zeros(N, f), np.zeros((N, 2), f), np.zeros((N, 3), f)
    for n in range(N):
        mode[n], scale[n], pid[n], clear[n] = plan_robot(p, sp, goals[n], rows[n], bc, bs)
    return mode, scale, pid, clear


def commit(sp, mode, pid, policy):
    """-> actions f32[N,2]; bits are copied (a NaN or a -0.0 coming in stays what it is)"""
    policy = np.ascontiguousarray(policy, f)
    pid = np.ascontiguousarray(pid, f)
    out = policy.copy()
    for n, m in enumerate(np.asarray(mode).tolist()):
        if m in (R.SIMPLE, R.AT_GOAL):
            out[n] = pid[n]
        elif m == R.EMERGENT:
            if policy[n, 0] > sp["v_cap"]:          # (false for a NaN: it stays)
                out[n, 0] = sp["v_cap"]
    return out


def scaled_range(x, s):
    """the range the safe policy sees in place of x = |raw| under the factor s, elementwise float32"""
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        return np.where(x < RANGE_MAX, (x * f(s)).astype(f), x).astype(f)


def scaled_ring(ring, scale):
    """ring f32[N,F,B] of raw ranges, scale f32[N] -> the ring the UNSCALED front end has to be fed with to see what the scaled
    one sees: |x| (the front end folds the sign first), every return times its robot's factor in all frames, 6.0 kept."""
    ring = np.abs(np.asarray(ring, f))
    s = np.asarray(scale, f).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        return np.where(ring < RANGE_MAX, (ring * s).astype(f), ring).astype(f)
