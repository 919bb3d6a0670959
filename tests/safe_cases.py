"""Crafted inputs of hybrid control in the paper's form (csrc/mrca_safe_device.h) that the host test (tests/test_safe_host.py)
and the GPU test (tests/test_gpu_safe_policy.py) share -- data only -- and the ``*_expectations`` that assert, from the rule's
text, what each is made for:

* the commit under NaN, Inf and -0.0 commands, and with v exactly at the cap and one ulp either side, in every mode and in two
  that are none;
* the plan on the rows of tests/hybrid_cases.py (the host set on its hand-made beam table, the device set on the env's own):
  the mode of each edge, the scan scale on the edges of the risk rule, the PID command;
* the edges of the scale rule the safe policy's scan is seen through.

The commit's cases and the plan's device set go onto the device as they stand (tests/test_gpu_safe_policy.py); the plan's host
set does not (tests/hybrid_cases.py says why and what stands in for it).  The edges of the scale rule are the host test's alone:
they are single values for the header's safe_scan_range, among them values beyond the sensor's range that no ring holds; on the
device the scaled front ends meet 0.0, -0.0, 6.0 and the last float below 6 in ``deep_ring`` of tests/test_gpu_safe_policy.py,
and the plan's scale output is held to the edges of the risk rule by ``plan_expectations``."""
import numpy as np

import hybrid_cases as HK
import hybrid_ref as R

f32 = np.float32
bits, same_bits, below, above = HK.bits, HK.same_bits, HK.below, HK.above

# ------------------------------------------------------------------------------------------------ the commit
COMMIT_SAFE = dict(scan_scale=0.7, v_cap=0.3)
COMMIT_MODES = [R.NORMAL, R.SIMPLE, R.EMERGENT, R.AT_GOAL, 7, -1]        # (7, -1: no mode of the rule -- the command is copied)
COMMIT_PID = (0.625, -0.125)


def commit_commands(cap):
    cap = f32(cap)
    return [(np.nan, 0.5), (np.inf, -np.inf), (-np.inf, np.inf), (-0.0, -0.0), (0.5, np.nan), (float(cap), 0.25),
            (float(below(cap)), 0.25), (float(above(cap)), 0.25), (0.0, 0.0), (1.0, -1.0)]


def commit_cases():
    """-> (mode i32[n], pid f32[n,2], policy f32[n,2]): every command of ``commit_commands`` in every mode of COMMIT_MODES"""
    cmds = commit_commands(COMMIT_SAFE["v_cap"])
    mode = np.repeat(np.array(COMMIT_MODES, np.int32), len(cmds))
    policy = np.tile(np.array(cmds, f32), (len(COMMIT_MODES), 1))
    pid = np.tile(np.array([COMMIT_PID], f32), (len(mode), 1))
    pid[len(cmds) + 3] = (-0.0, np.nan)                                   # whatever pid holds is what modes 1 and -2 give
    return mode, pid, policy


def commit_expectations(got, pid, policy):
    """stated from the rule, not from the restatement; ``got``: the commit of ``commit_cases()`` under COMMIT_SAFE"""
    cap = f32(COMMIT_SAFE["v_cap"])
    n_modes, n_cmds = len(COMMIT_MODES), len(commit_commands(cap))
    got = np.asarray(got, f32).reshape(n_modes, n_cmds, 2)
    pol = np.asarray(policy, f32).reshape(n_modes, n_cmds, 2)
    for i in (0, 4, 5):                                                   # copied bit for bit
        assert np.array_equal(bits(got[i]), bits(pol[i]))
    for i in (1, 3):                                                      # the pid, whatever comes in
        assert np.array_equal(bits(got[i]), bits(np.asarray(pid, f32).reshape(n_modes, n_cmds, 2)[i]))
    e = got[2]
    assert np.array_equal(bits(e[:, 1]), bits(pol[2][:, 1]))              # omega is kept in mode 2, a NaN included
    assert np.isnan(e[0, 0]) and same_bits(e[1, 0], cap) and np.isneginf(e[2, 0]) and same_bits(e[3, 0], -0.0)
    assert same_bits(e[5, 0], cap) and same_bits(e[6, 0], below(cap)) and same_bits(e[7, 0], cap)      # at, below, above the cap
    assert same_bits(e[9, 0], cap) and same_bits(e[8, 0], 0.0)


# ------------------------------------------------------------------------------------------------ the plan
PLAN_SAFE = dict(scan_scale=0.7, v_cap=0.3)


def plan_expectations(names, sp, mode, scale, pid, clear, hybrid):
    """The plan of the rows of hybrid_cases (``names`` in front) under R.params(**HK.PARAMS) and ``sp``: the mode, the
    clearances and mode 1's command are the ones ``hybrid`` = (act, mode, clear) of the command-scaling rule reports on the same
    rows (which ``HK.expectations`` holds to their edges); the scan scale follows the risk rule on its edges."""
    n = len(names)
    ix = {k: i for i, k in enumerate(names)}
    hact, hmode, hclear = hybrid
    assert np.array_equal(mode[:n], hmode[:n]) and same_bits(clear[:n], hclear[:n])
    assert same_bits(scale[:n], np.where(mode[:n] == R.EMERGENT, sp["scan_scale"], f32(1.0)))
    assert not bits(pid[:n][mode[:n] != R.SIMPLE]).any()                 # (+0.0, +0.0) outside mode 1
    simple = mode[:n] == R.SIMPLE
    assert simple.any() and same_bits(pid[:n][simple], hact[:n][simple])
    # exactly risk_dist is no risk: the scan is seen as it is; one ulp below it is seen through scan_scale
    edge = [k for k in names if k.startswith("d_min_is_risk")]
    under = [k for k in names if k.startswith("d_min_below_risk")]
    assert edge and len(edge) == len(under)
    assert all(same_bits(scale[ix[k]], 1.0) for k in edge) and all(same_bits(scale[ix[k]], sp["scan_scale"]) for k in under)
    for k in ("d_front_at_stop", "range_minus_0", "risk_beside_front_open"):
        assert mode[ix[k]] == R.EMERGENT and same_bits(scale[ix[k]], sp["scan_scale"])


# ------------------------------------------------------------------------------------------------ the scale rule
SIX = f32(6.0)
SCALE_EDGES = np.array([0.0, -0.0, 6.0, np.nextafter(SIX, f32(0.0)), np.nextafter(SIX, f32(7.0)), 1.0, 0.1, 5.999, 3.0000002, 2.0 ** -126,
                        np.inf, 7.5], f32)
SCALE_FACTORS = (0.7, 0.8, 0.5, 1.0, 2.0 ** -20, float(np.nextafter(f32(1.0), f32(0.0))))


def scale_expectations(x, s, out):
    """``out``: the rule on ``x`` (SCALE_EDGES in front) under the factor ``s``"""
    assert same_bits(out[0], 0.0) and same_bits(out[2], 6.0)         # 0 stays 0; "nothing" stays nothing
    assert same_bits(out[1], -0.0)                                    # (the front ends fold the sign BEFORE the rule: |x|)
    assert same_bits(out[3], f32(x[3]) * f32(s)) and out[3] < SIX   # the last float below 6 is a return: scaled, below 6
    assert same_bits(out[4], x[4]) and same_bits(out[10], np.inf) and same_bits(out[11], 7.5)      # beyond the range: kept
    if s == 1.0:
        assert np.array_equal(bits(out), bits(x))                     # ones are the identity
