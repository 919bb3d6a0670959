"""Hybrid control in the paper's form (csrc/mrca_safe_device.h) compiled for the host with g++ -ffp-contract=off: the very
functions the gfx950 kernels call, held EQUAL bit for bit to the NumPy float32 restatement of tests/safe_ref.py -- the plan on
random rows under several parameter sets (every mode asserted to occur; mode and clearances also equal to what the EXISTING
header's hybrid_robot returns), the commit under NaN, Inf and -0.0 commands in each mode and with v exactly at the cap and one
ulp either side, the scale rule on its edges -- and the library's validation table of the four new calls.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hybrid_cases as HK
import hybrid_ref as R
import safe_cases as K
import safe_ref as SR
import util as U
from test_hybrid_host import PARAM_SETS, Params, beam_table, bits, cparams, random_inputs, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include "mrca_safe_device.h"
using namespace mrca;
extern "C" void shim_plan(const HybridParams* q, const SafeParams* sp, int N, const float* goal, const float* rows, int beams,
                          const float* bc, const float* bs, int* mode, float* scale, float* pid, float* clear) {
    for (int n = 0; n < N; ++n)
        safe_plan_robot(*q, *sp, goal + 2 * n, rows + (size_t)n * beams, beams, bc, bs, mode + n, scale + n, pid + 2 * n, clear + 3 * n);
}
// act may be policy itself
extern "C" void shim_commit(const SafeParams* sp, int N, const int* mode, const float* pid, const float* policy, float* act) {
    for (int n = 0; n < N; ++n) {
        float v, w;
        safe_commit(*sp, mode[n], policy[2 * n], policy[2 * n + 1], pid[2 * n], pid[2 * n + 1], &v, &w);
        act[2 * n] = v;
        act[2 * n + 1] = w;
    }
}
extern "C" void shim_scale(int n, const float* x, float s, float* out) {
    for (int i = 0; i < n; ++i) out[i] = safe_scan_range(x[i], s);
}
// the EXISTING rule on the same inputs (mrca_hybrid_device.h: hybrid_robot)
extern "C" void shim_hybrid(const HybridParams* q, int N, const float* goal, const float* policy, const float* rows, int beams,
                            const float* bc, const float* bs, float* act, int* mode, float* clear) {
    for (int n = 0; n < N; ++n)
        hybrid_robot(*q, goal + 2 * n, policy + 2 * n, rows + (size_t)n * beams, beams, bc, bs, act + 2 * n, mode + n, clear + 3 * n);
}
"""


class SafeParams(C.Structure):
    _fields_ = [(k, C.c_float) for k in SR.FIELDS]


def csafe(sp):
    return SafeParams(**{k: float(v) for k, v in sp.items()})


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("safe_host")
    src, so = d / "shim.cpp", d / "libsafe_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.shim_plan.argtypes = [C.POINTER(Params), C.POINTER(SafeParams), C.c_int, fp, fp, C.c_int, fp, fp, ip, fp, fp, fp]
    lib.shim_commit.argtypes = [C.POINTER(SafeParams), C.c_int, ip, fp, fp, fp]
    lib.shim_scale.argtypes = [C.c_int, fp, C.c_float, fp]
    lib.shim_hybrid.argtypes = [C.POINTER(Params), C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, ip, fp]
    return lib


SAFE_SETS = [SR.params(), SR.params(scan_scale=0.7, v_cap=0.3), SR.params(scan_scale=1.0, v_cap=1.0), SR.params(scan_scale=2.0 ** -20, v_cap=0.05)]


def host_plan(shim, p, sp, goal, rows, bc, bs):
    goal, rows = np.ascontiguousarray(goal, f32), np.ascontiguousarray(rows, f32)
    N, B = rows.shape
    mode, scale, pid, clear = np.zeros(N, np.int32), np.zeros(N, f32), np.full((N, 2), 7.0, f32), np.zeros((N, 3), f32)
    q, s = cparams(p), csafe(sp)
    shim.shim_plan(C.byref(q), C.byref(s), N, _fp(goal), _fp(rows), B, _fp(bc), _fp(bs), _ip(mode), _fp(scale), _fp(pid), _fp(clear))
    return mode, scale, pid, clear


def host_commit(shim, sp, mode, pid, policy, in_place=False):
    mode, pid, policy = np.ascontiguousarray(mode, np.int32), np.ascontiguousarray(pid, f32), np.ascontiguousarray(policy, f32)
    act = policy.copy() if in_place else np.full_like(policy, 7.0)
    s = csafe(sp)
    shim.shim_commit(C.byref(s), len(mode), _ip(mode), _fp(pid), _fp(act) if in_place else _fp(policy), _fp(act))
    return act


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_plan_on_random_rows_equals_the_reference_and_the_existing_rule(shim, beams):
    rng = np.random.default_rng(beams + 1)
    goal, policy, rows = random_inputs(rng, 32, beams)
    bc, bs = beam_table(beams)
    seen = set()
    for i, p in enumerate(PARAM_SETS):
        sp = SAFE_SETS[i % len(SAFE_SETS)]
        mode, scale, pid, clear = host_plan(shim, p, sp, goal, rows, bc, bs)
        wmode, wscale, wpid, wclear = SR.plan(p, sp, goal, rows, bc, bs)
        assert np.array_equal(mode, wmode), (mode, wmode)
        assert same_bits(scale, wscale) and same_bits(pid, wpid) and same_bits(clear, wclear)
        # what the plan promises of its outputs
        assert same_bits(scale, np.where(mode == R.EMERGENT, sp["scan_scale"], f32(1.0)))
        assert not bits(pid[mode != R.SIMPLE]).any()                     # (+0.0, +0.0) outside mode 1
        # the EXISTING header on the same inputs, with a real command: same mode, same clearances, and its mode-1 command is the pid
        act, hmode, hclear = np.zeros((32, 2), f32), np.zeros(32, np.int32), np.zeros((32, 3), f32)
        q = cparams(p)
        shim.shim_hybrid(C.byref(q), 32, _fp(np.ascontiguousarray(goal, f32)), _fp(np.ascontiguousarray(policy, f32)),
                         _fp(np.ascontiguousarray(rows, f32)), beams, _fp(bc), _fp(bs), _fp(act), _ip(hmode), _fp(hclear))
        assert np.array_equal(mode, hmode) and same_bits(clear, hclear)
        assert same_bits(pid[mode == R.SIMPLE], act[mode == R.SIMPLE])
        seen |= set(mode.tolist())
        # ... and the commit of a command under this plan
        for in_place in (False, True):
            got = host_commit(shim, sp, mode, pid, policy, in_place)
            assert same_bits(got, SR.commit(sp, mode, pid, policy))
    assert seen == {R.AT_GOAL, R.NORMAL, R.SIMPLE, R.EMERGENT}


# ------------------------------------------------------------------------------------------------ the plan on the crafted rows
@pytest.mark.parametrize("which,beams", [("host", 64), ("device", 64), ("device", 192), ("device", 1024)])
def test_plan_on_the_crafted_rows(shim, which, beams):
    """tests/hybrid_cases.py through the plan: the host set on its hand-made beam table, the device set (which
    tests/test_gpu_safe_policy.py writes into an env) on the env's own"""
    names, goal, policy, rows = HK.crafted(beams) if which == "host" else HK.device_cases(beams)
    bc, bs = HK.crafted_table(beams) if which == "host" else beam_table(beams)
    p, sp = R.params(**HK.PARAMS), SR.params(**K.PLAN_SAFE)
    mode, scale, pid, clear = host_plan(shim, p, sp, goal, rows, bc, bs)
    wmode, wscale, wpid, wclear = SR.plan(p, sp, goal, rows, bc, bs)
    assert np.array_equal(mode, wmode) and same_bits(scale, wscale) and same_bits(pid, wpid) and same_bits(clear, wclear)
    hact, hmode, hclear, nb = R.env_actions(p, goal, policy, rows, bc, bs)
    HK.expectations(names, p, policy, rows, hact, hmode, hclear, nb)
    K.plan_expectations(names, sp, wmode, wscale, wpid, wclear, (hact, hmode, hclear))


# ------------------------------------------------------------------------------------------------ the commit
def test_commit_under_special_commands_in_every_mode(shim):
    sp = SR.params(**K.COMMIT_SAFE)
    mode, pid, policy = K.commit_cases()
    want = SR.commit(sp, mode, pid, policy)
    for in_place in (False, True):
        got = host_commit(shim, sp, mode, pid, policy, in_place)
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    K.commit_expectations(got, pid, policy)


# ------------------------------------------------------------------------------------------------ the scale rule
def test_the_scale_rule_on_its_edges(shim):
    rng = np.random.default_rng(4)
    x = np.concatenate([K.SCALE_EDGES, rng.uniform(0.0, 6.0, 4096).astype(f32)])
    for s in K.SCALE_FACTORS:
        out = np.zeros_like(x)
        shim.shim_scale(len(x), _fp(x), f32(s), _fp(out))
        want = SR.scaled_range(x, s)
        assert np.array_equal(bits(out), bits(want)), (s, np.argwhere(bits(out) != bits(want))[:5])
        K.scale_expectations(x, s, out)
    # 0.7 is no dyadic rational: the product is rounded, once, as float32 rounds it
    assert same_bits(SR.scaled_range(f32(0.1), 0.7), f32(0.1) * f32(0.7)) and float(f32(0.1) * f32(0.7)) != float(f32(0.1)) * float(f32(0.7))
    # the ring form: |x| first, all three frames by the robot's factor
    ring = np.array([[[1.0, -2.0, 6.0, -0.0], [3.0, 6.0, 0.5, 5.0], [-6.0, 4.0, 0.0, 1.5]],
                     [[1.0, -2.0, 6.0, -0.0], [3.0, 6.0, 0.5, 5.0], [-6.0, 4.0, 0.0, 1.5]]], f32)
    got = SR.scaled_ring(ring, np.array([0.5, 1.0], f32))
    assert same_bits(got[0], [[0.5, 1.0, 6.0, 0.0], [1.5, 6.0, 0.25, 2.5], [6.0, 2.0, 0.0, 0.75]])
    assert same_bits(got[1], np.abs(ring[1]))


# ------------------------------------------------------------------------------------------------ the library's validation table
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.hybrid import SafePolicyParams
    assert built_lib.mrca_safe_policy_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.SafePolicyParamsStruct()
    assert built_lib.mrca_safe_policy_default_params(C.byref(st)) == 0
    assert {k: getattr(st, k) for k in SR.FIELDS} == {k: float(f32(v)) for k, v in SR.DEFAULTS.items()}
    assert [n for n, _t in _lib.SafePolicyParamsStruct._fields_] == SR.FIELDS and C.sizeof(st) == 8
    p = SafePolicyParams(scan_scale=0.7)
    assert p.scan_scale == 0.7 and p.v_cap == float(f32(SR.DEFAULTS["v_cap"])) and abs(p.struct().scan_scale - 0.7) < 1e-7
    assert SafePolicyParams.from_assignments(["v_cap=0.25"]).v_cap == 0.25
    with pytest.raises(ValueError):
        SafePolicyParams.from_assignments(["nonsense=1"])
    # a rejected call touches nothing: `out` stands where the device buffers would (host memory -- no call gets as far as a launch)
    out = np.full(64, 7.0, f32)
    ptr = C.c_void_p(out.ctypes.data)
    off4 = C.c_void_p(out.ctypes.data + 4)
    assert out.ctypes.data % 16 == 0
    err = built_lib.mrca_last_error

    def plan(hp=None, sp=None, mode=ptr, scale=ptr, pid=ptr, clear=None):
        return built_lib.mrca_hybrid_plan(None, None if hp is None else C.byref(hp), None if sp is None else C.byref(sp), None, mode,
                                          scale, pid, clear, None)

    def commit(sp=None, n=4, mode=ptr, pid=ptr, policy=ptr, actions=ptr):
        return built_lib.mrca_hybrid_commit(n, None if sp is None else C.byref(sp), None, mode, pid, policy, actions, None)
    # what can be judged without an env is judged before the env is looked at
    assert plan() == -1 and b"env is NULL" in err()
    for kw, what in (({"mode": None}, b"mode_dev is NULL"), ({"scale": None}, b"scale_dev is NULL"), ({"pid": None}, b"pid_dev is NULL"),
                     ({"pid": off4}, b"8-byte aligned"), ({"mode": C.c_void_p(out.ctypes.data + 2)}, b"4-byte aligned")):
        assert plan(**kw) == -1 and what in err(), (kw, err())
    for kw, what in (({"mode": None}, b"mode_dev is NULL"), ({"pid": None}, b"pid_dev is NULL"), ({"policy": None}, b"policy_dev is NULL"),
                     ({"actions": None}, b"actions_dev is NULL"), ({"actions": off4}, b"8-byte aligned"), ({"pid": off4}, b"8-byte aligned"),
                     ({"n": 0}, b"n_robots")):
        assert commit(**kw) == -1 and what in err(), (kw, err())
    bad = [("scan_scale", 0.0), ("scan_scale", -0.5), ("scan_scale", 1.5), ("v_cap", 0.0), ("v_cap", -1.0), ("v_cap", 1.01)]
    bad += [(k, v) for k in SR.FIELDS for v in (float("nan"), float("inf"), float("-inf"))]
    for k, v in bad:
        st = _lib.SafePolicyParamsStruct()
        built_lib.mrca_safe_policy_default_params(C.byref(st))
        setattr(st, k, v)
        for call in (plan, commit):
            e = err() if call(sp=st) == -1 else b"accepted"
            assert k.encode() in e and b"env is NULL" not in e, (k, v, e)
    # the hybrid params go through the table of mrca_hybrid_actions
    for k, v in [("stop_dist", 0.7), ("risk_dist", 6.5), ("corridor", 0.0), ("look", float("nan")), ("max_speed", 1.5)]:
        st = _lib.HybridParamsStruct()
        built_lib.mrca_hybrid_default_params(C.byref(st))
        setattr(st, k, v)
        e = err() if plan(hp=st) == -1 else b"accepted"
        assert (k.encode() in e or (k == "stop_dist" and b"risk_dist" in e)) and b"mrca_hybrid_plan" in e and b"env is NULL" not in e, (k, v, e)
    # the edges of the table are inside it: these get as far as the env
    for k, v in [("scan_scale", 1.0), ("v_cap", 1.0), ("scan_scale", 2.0 ** -20), ("v_cap", 1e-3)]:
        st = _lib.SafePolicyParamsStruct()
        built_lib.mrca_safe_policy_default_params(C.byref(st))
        setattr(st, k, v)
        assert plan(sp=st) == -1 and b"env is NULL" in err(), (k, v, err())
    # the two scaled front ends: raw ring form only, 3 x 512 only -- judged before the first HIP call
    for name in ("mrca_lidar_features_scaled", "mrca_lidar_features_bf16_scaled"):
        fn = getattr(built_lib, name)

        def fe(head=ptr, scale=ptr, frames=3, beams=512, n=4, obs=ptr):
            return fn(obs, head, scale, n, frames, beams, ptr, ptr, ptr, ptr, ptr, None)
        assert fe(head=None) == -1 and b"obs_head_dev is NULL" in err() and name.encode() in err()
        assert fe(scale=None) == -1 and b"scale_dev is NULL" in err()
        assert fe(scale=C.c_void_p(out.ctypes.data + 2)) == -1 and b"4-byte aligned" in err()
        assert fe(obs=None) == -1 and b"NULL pointer" in err()
        assert fe(frames=2) == -4 and fe(beams=256) == -4 and fe(n=0) == -4
    assert built_lib.mrca_lidar_features_bf16_scaled(off4, ptr, ptr, 4, 3, 512, ptr, ptr, ptr, ptr, ptr, None) == -1
    assert b"16-byte aligned" in err()
    assert (out == 7.0).all()
