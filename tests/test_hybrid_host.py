"""The hybrid control rule (csrc/mrca_hybrid_device.h) compiled for the host with g++ -ffp-contract=off: the very functions the
gfx950 kernel calls, held EQUAL bit for bit to the NumPy float32 restatement of tests/hybrid_ref.py -- on random rows, on
crafted rows that stand exactly on each of the rule's edges (with the branch each one takes asserted from the restatement, not
hoped for), under a permutation of the beams -- and the library's validation table.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hybrid_ref as R
import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include "mrca_hybrid_device.h"
using namespace mrca;
// every robot from host copies of its fields; act may be policy itself
extern "C" void shim_env(const HybridParams* q, int N, const float* goal, const float* policy, const float* rows, int beams,
                         const float* bc, const float* bs, float* act, int* mode, float* clear) {
    for (int n = 0; n < N; ++n)
        hybrid_robot(*q, goal + 2 * n, policy + 2 * n, rows + (size_t)n * beams, beams, bc, bs, act + 2 * n, mode + n, clear + 3 * n);
}
// the pieces the kernel puts together: the beams dealt to `lanes` partial results as the kernel deals them, merged pairwise
extern "C" void shim_dealt(const HybridParams* q, const float* goal, const float* policy, const float* row, int beams, const float* bc,
                           const float* bs, int lanes, float* act, int* mode, float* clear) {
    const HybridRobot rb = hybrid_robot_begin(*q, goal[0], goal[1]);
    HybridAcc acc[64];
    for (int l = 0; l < lanes; ++l) {
        acc[l] = hybrid_acc_empty();
        for (int b = l; b < beams; b += lanes) hybrid_beam(*q, rb, row[b], bc[b], bs[b], &acc[l]);
    }
    for (int o = lanes / 2; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) acc[l] = hybrid_acc_merge(acc[l], acc[l + o]);
    hybrid_result(*q, rb, acc[0], policy[0], policy[1], &act[0], &act[1], mode);
    clear[0] = acc[0].d_min; clear[1] = acc[0].d_front; clear[2] = acc[0].d_block;
}
"""


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in R.FIELDS]


def cparams(p):
    return Params(**{k: float(v) for k, v in p.items()})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("hybrid_host")
    src, so = d / "shim.cpp", d / "libhybrid_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.shim_env.argtypes = [C.POINTER(Params), C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, ip, fp]
    lib.shim_dealt.argtypes = [C.POINTER(Params), fp, fp, fp, C.c_int, fp, fp, C.c_int, fp, ip, fp]
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, f32)), bits(np.asarray(b, f32)))


def beam_table(B):
    return tuple(np.ascontiguousarray(t, f32) for t in U.O.beam_table(f32, B))


def host_env_actions(shim, p, goal, policy, rows, bc=None, bs=None, in_place=False):
    """The host build of the rule on every robot -> (actions, mode, clear)"""
    goal, policy, rows = (np.ascontiguousarray(t, f32) for t in (goal, policy, rows))
    N, B = rows.shape
    if bc is None:
        bc, bs = beam_table(B)
    act = policy.copy() if in_place else np.full((N, 2), 7.0, f32)
    mode, clear = np.zeros(N, np.int32), np.zeros((N, 3), f32)
    q = cparams(p)
    shim.shim_env(C.byref(q), N, _fp(goal), _fp(act) if in_place else _fp(policy), _fp(rows), B, _fp(bc), _fp(bs), _fp(act), _ip(mode),
                  _fp(clear))
    return act, mode, clear


def assert_equal_to_ref(shim, p, goal, policy, rows, bc=None, bs=None):
    """host build == restatement on every output, out of place and in place -> (the restatement's outputs)"""
    want = R.env_actions(p, goal, policy, rows, bc, bs)
    for in_place in (False, True):
        act, mode, clear = host_env_actions(shim, p, goal, policy, rows, bc, bs, in_place)
        assert np.array_equal(want[1], mode), (want[1], mode)
        assert same_bits(want[2], clear), np.argwhere(bits(want[2]) != bits(clear))[:5]
        assert same_bits(want[0], act), np.argwhere(bits(want[0]) != bits(act))[:5]
    return want


# ------------------------------------------------------------------------------------------------ equality with hybrid_ref
def random_inputs(rng, N, B):
    rows = rng.uniform(0.05, 6.0, (N, B)).astype(f32)
    rows[rng.random((N, B)) < 0.5] = 6.0                 # half the beams see nothing
    rows[: N // 2] = np.maximum(rows[: N // 2], f32(1.2))                # half the robots have room around them
    rows[: N // 4][rng.random((N // 4, B)) < 0.9] = 6.0                  # ... and half of those nearly open space
    th = rng.uniform(-np.pi, np.pi, N)
    dist = rng.uniform(0.0, 8.0, N)
    dist[::5] = rng.uniform(0.0, 0.7, len(dist[::5]))                    # near and inside the goal radius
    goal = np.stack([dist * np.cos(th), dist * np.sin(th)], 1).astype(f32)
    policy = np.stack([rng.uniform(0, 1, N), rng.uniform(-1, 1, N)], 1).astype(f32)
    return goal, policy, rows


PARAM_SETS = [
    R.params(),
    R.params(risk_dist=6.0, stop_dist=0.0, safe_scale=1.0),              # the widest the table allows
    R.params(corridor=0.01, look=0.5),
    R.params(corridor=3.0, look=6.0, risk_dist=0.2, stop_dist=0.1),
    R.params(front_cos=-1.0),
    R.params(front_cos=1.0, safe_scale=0.0),                             # no beam is ahead; mode 2 stops
    R.params(v_pid=0.3, max_speed=0.2, k_omega=0.0),
    R.params(v_pid=1e-5),                                                # slower than ORCA's "still": the PID law says (0, 0)
]


@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_random_inputs_equal_the_reference(shim, beams):
    rng = np.random.default_rng(beams)
    goal, policy, rows = random_inputs(rng, 32, beams)
    seen = set()
    for p in PARAM_SETS:
        _a, mode, _c, _n = assert_equal_to_ref(shim, p, goal, policy, rows)
        seen |= set(mode.tolist())
    assert seen == {R.AT_GOAL, R.NORMAL, R.SIMPLE, R.EMERGENT}


def crafted_table(B=64):
    """beam directions with three exact ones: beam 0 = (0, 1) (left), beam 1 = (1, 0) (ahead), beam 2 = (0, -1) (right); the rest
    the env's own"""
    bc, bs = beam_table(B)
    bc, bs = bc.copy(), bs.copy()
    bc[:3] = [0.0, 1.0, 0.0]
    bs[:3] = [1.0, 0.0, -1.0]
    return bc, bs


def below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def above(x):
    return np.nextafter(f32(x), f32(np.inf))


def test_crafted_inputs_stand_on_every_edge(shim):
    B = 64
    bc, bs = crafted_table(B)
    open_row = np.full(B, 6.0, f32)
    names, goals, cmds, rows = [], [], [], []

    def add(name, goal, row, cmd=(0.75, -0.25)):
        names.append(name)
        goals.append(goal)
        cmds.append(cmd)
        rows.append(row)

    def lone(beam, r):
        row = open_row.copy()
        row[beam] = f32(r)
        return row
    # (its own corridor, look and scale; risk_dist 0.4 so that a return on the corridor's edge, 0.45 m away, is not a risk)
    p = R.params(risk_dist=0.4, stop_dist=0.3, safe_scale=0.5, corridor=0.45, look=4.0)
    cor, risk, stop = p["corridor"], p["risk_dist"], p["stop_dist"]
    add("goal_half_a_metre_ahead", (0.5, 0.0), lone(1, 0.2))
    add("goal_just_outside", (float(above(0.5)), 0.0), open_row.copy())
    add("all_ranges_6", (3.0, 1.0), open_row.copy())
    add("edge_of_corridor_t0", (4.0, 0.0), lone(0, cor))                 # t = 0, |l| = corridor exactly: does not block
    add("inside_corridor_t0", (4.0, 0.0), lone(0, below(cor)))           # t = 0, one ulp inside: blocks
    add("inside_corridor_right_t0", (4.0, 0.0), lone(2, below(cor)))
    add("at_reach", (2.0, 0.0), lone(1, 2.0))                            # t = reach = gl exactly: blocks
    add("beyond_reach", (2.0, 0.0), lone(1, above(2.0)))
    add("at_look", (5.5, 0.0), lone(1, 4.0))                             # t = reach = look exactly: blocks
    add("beyond_look", (5.5, 0.0), lone(1, above(4.0)))
    add("d_min_is_risk", (0.0, 3.0), lone(2, risk))                      # exactly risk_dist: not emergent
    add("d_min_below_risk", (0.0, 3.0), lone(2, below(risk)))
    add("d_front_at_stop", (3.0, 0.0), lone(1, stop))                    # s = 0
    add("d_front_below_stop", (3.0, 0.0), lone(1, 0.1))                  # s would be negative: 0
    add("d_front_between", (3.0, 0.0), lone(1, 0.325))                   # s = 0.25 (about)
    add("risk_beside_front_open", (3.0, 0.0), lone(0, 0.35))             # d_front 6: s = safe_scale
    row = open_row.copy()
    row[1], row[5] = f32(-0.0), f32(0.0)
    add("range_minus_0", (3.0, 0.0), row)
    add("goal_straight_behind", (-3.0, 0.0), open_row.copy())
    add("goal_behind_left", (-3.0, 1.0), open_row.copy())
    add("goal_behind_right", (-3.0, -1.0), open_row.copy())
    add("goal_ahead_left", (1.0, 0.05), open_row.copy())
    blocked = lone(1, 1.0)
    for k, cmd in (("nan", (np.nan, 0.5)), ("inf", (np.inf, -np.inf)), ("minus_0", (-0.0, -0.0)), ("nan_w", (0.5, np.nan))):
        add("normal_" + k, (3.0, 0.0), blocked, cmd)
        add("simple_" + k, (3.0, 0.0), open_row.copy(), cmd)
        add("emergent_" + k, (3.0, 0.0), lone(1, 0.35), cmd)
        add("at_goal_" + k, (0.1, 0.1), open_row.copy(), cmd)
    goal, policy, rows = np.array(goals, f32), np.array(cmds, f32), np.stack(rows)
    ix = {k: i for i, k in enumerate(names)}
    act, mode, clear, nb = assert_equal_to_ref(shim, p, goal, policy, rows, bc, bs)

    def m(k):
        return int(mode[ix[k]])
    # 0.5 m is AT the goal (<=): (0, 0) whatever is near; the next float is not
    assert m("goal_half_a_metre_ahead") == R.AT_GOAL and same_bits(act[ix["goal_half_a_metre_ahead"]], [0.0, 0.0])
    assert same_bits(clear[ix["goal_half_a_metre_ahead"]], [0.2, 0.2, 6.0])
    assert m("goal_just_outside") == R.SIMPLE
    # nothing anywhere: the PID law, and every clearance is 6
    i = ix["all_ranges_6"]
    assert m("all_ranges_6") == R.SIMPLE and same_bits(clear[i], [6.0, 6.0, 6.0]) and act[i][0] > 0.9 and act[i][1] == 1.0
    # the corridor's edge is outside it (strict), one ulp inside blocks; t = 0 is inside (>=)
    assert nb[ix["edge_of_corridor_t0"]] == 0 and m("edge_of_corridor_t0") == R.SIMPLE
    for k in ("inside_corridor_t0", "inside_corridor_right_t0"):
        assert nb[ix[k]] == 1 and m(k) == R.NORMAL and same_bits(act[ix[k]], policy[ix[k]]) and clear[ix[k]][2] == below(cor)
    # t = reach is inside (<=), whether the goal's distance or `look` ends the corridor
    assert nb[ix["at_reach"]] == 1 and m("at_reach") == R.NORMAL and nb[ix["beyond_reach"]] == 0 and m("beyond_reach") == R.SIMPLE
    assert nb[ix["at_look"]] == 1 and m("at_look") == R.NORMAL and nb[ix["beyond_look"]] == 0 and m("beyond_look") == R.SIMPLE
    # d_min == risk_dist is not a risk (strict)
    assert m("d_min_is_risk") == R.SIMPLE and m("d_min_below_risk") == R.EMERGENT
    # the scale: 0 at and below stop_dist, in between in between, safe_scale where nothing is ahead; omega goes through
    for k in ("d_front_at_stop", "d_front_below_stop"):
        assert m(k) == R.EMERGENT and same_bits(act[ix[k]], [0.0, -0.25])
    i = ix["d_front_between"]
    assert m("d_front_between") == R.EMERGENT and 0.0 < act[i][0] < 0.75 * 0.5 and same_bits(act[i][1], -0.25)
    i = ix["risk_beside_front_open"]
    assert m("risk_beside_front_open") == R.EMERGENT and same_bits(act[i], [0.75 * 0.5, -0.25]) and same_bits(clear[i], [0.35, 6.0, 0.35])
    # -0.0 is a 0: d_min is +0, the robot is in danger and stops
    i = ix["range_minus_0"]
    assert m("range_minus_0") == R.EMERGENT and same_bits(clear[i], [0.0, 0.0, 0.0]) and same_bits(act[i], [0.0, -0.25])
    # a goal behind (fwd <= 0): stand and turn at full rate, to the left when the goal is straight behind or to the left
    assert same_bits(act[ix["goal_straight_behind"]], [0.0, 1.0]) and same_bits(act[ix["goal_behind_left"]], [0.0, 1.0])
    assert same_bits(act[ix["goal_behind_right"]], [0.0, -1.0])
    assert all(m(k) == R.SIMPLE for k in ("goal_straight_behind", "goal_behind_left", "goal_behind_right", "goal_ahead_left"))
    i = ix["goal_ahead_left"]
    assert 0.99 < act[i][0] < 1.0 and 0.29 < act[i][1] < 0.31           # k_omega * uy = 6 * 0.05 (about)
    # a NaN, an Inf or a -0.0 coming in: normal copies the bits, simple and at-goal do not look at them, emergent scales v
    for k in ("nan", "inf", "minus_0", "nan_w"):
        i = ix["normal_" + k]
        assert m("normal_" + k) == R.NORMAL and np.array_equal(bits(act[i]), bits(policy[i]))
        assert m("simple_" + k) == R.SIMPLE and same_bits(act[ix["simple_" + k]], [1.0, 0.0])
        assert m("at_goal_" + k) == R.AT_GOAL and same_bits(act[ix["at_goal_" + k]], [0.0, 0.0])
        i = ix["emergent_" + k]
        assert m("emergent_" + k) == R.EMERGENT and np.array_equal(bits(act[i][1]), bits(policy[i][1]))
    assert np.isnan(act[ix["emergent_nan"]][0]) and np.isinf(act[ix["emergent_inf"]][0])
    assert same_bits(act[ix["emergent_minus_0"]], [-0.0, -0.0])


def test_a_permutation_of_the_beams_changes_no_bit(shim):
    """The minima and the count do not depend on the order: the beams of a row shuffled WITH their directions, and the beams
    dealt to 64 partial results that are merged pairwise (what the kernel does), give every output bit of the plain loop."""
    rng = np.random.default_rng(5)
    B = 192
    goal, policy, rows = random_inputs(rng, 24, B)
    rows[3, 7] = rows[3, 100] = rows[3].min()            # equal minima
    rows[4, :] = 6.0
    bc, bs = beam_table(B)
    for p in (R.params(), R.params(risk_dist=0.2, stop_dist=0.1, corridor=1.0)):
        want = assert_equal_to_ref(shim, p, goal, policy, rows)
        for _ in range(3):
            perm = rng.permutation(B)
            got = assert_equal_to_ref(shim, p, goal, policy, rows[:, perm], np.ascontiguousarray(bc[perm]), np.ascontiguousarray(bs[perm]))
            assert same_bits(want[0], got[0]) and np.array_equal(want[1], got[1]) and same_bits(want[2], got[2])
            assert np.array_equal(want[3], got[3])
        q = cparams(p)
        for n in range(len(goal)):
            for lanes in (64, 4):
                act, mode, clear = np.zeros(2, f32), np.zeros(1, np.int32), np.zeros(3, f32)
                shim.shim_dealt(C.byref(q), _fp(goal[n]), _fp(policy[n]), _fp(rows[n]), B, _fp(bc), _fp(bs), lanes, _fp(act), _ip(mode),
                                _fp(clear))
                assert same_bits(act, want[0][n]) and mode[0] == want[1][n] and same_bits(clear, want[2][n])


# ------------------------------------------------------------------------------------------------ the library's own defaults
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.hybrid import HybridParams
    assert built_lib.mrca_hybrid_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.HybridParamsStruct()
    assert built_lib.mrca_hybrid_default_params(C.byref(st)) == 0
    got = {k: getattr(st, k) for k in R.FIELDS}
    assert got == {k: float(f32(v)) for k, v in R.DEFAULTS.items()}
    assert [n for n, _t in _lib.HybridParamsStruct._fields_] == R.FIELDS and C.sizeof(st) == 36
    p = HybridParams(risk_dist=0.8)
    assert p.risk_dist == 0.8 and p.look == 6.0 and p.struct().corridor == 1.0
    assert HybridParams.from_assignments(["look=3.5", "v_pid=0.5"]).look == 3.5
    with pytest.raises(ValueError):
        HybridParams.from_assignments(["nonsense=1"])
    # a rejected call touches nothing: `out` stands where the device buffers would (host memory -- no call gets as far as a launch)
    out = np.full(64, 7.0, f32)
    ptr = C.c_void_p(out.ctypes.data)
    assert out.ctypes.data % 8 == 0

    def call(params=None, policy=ptr, actions=ptr):
        return built_lib.mrca_hybrid_actions(None, None if params is None else C.byref(params), None, policy, actions, None, None, None)
    # what can be judged without an env is judged before the env is looked at
    assert call() == -1 and b"env is NULL" in built_lib.mrca_last_error()
    assert call(actions=None) == -1 and b"actions_dev is NULL" in built_lib.mrca_last_error()
    assert call(policy=None) == -1 and b"policy_dev is NULL" in built_lib.mrca_last_error()
    assert call(actions=C.c_void_p(out.ctypes.data + 4)) == -1 and b"8-byte aligned" in built_lib.mrca_last_error()
    bad = [("stop_dist", -0.1), ("stop_dist", 0.6), ("stop_dist", 0.7), ("risk_dist", 6.5), ("risk_dist", 0.3), ("safe_scale", -0.1),
           ("safe_scale", 1.1), ("corridor", 0.0), ("corridor", -1.0), ("look", 0.0), ("look", 6.5), ("front_cos", -1.1),
           ("front_cos", 1.1), ("v_pid", 0.0), ("v_pid", -1.0), ("max_speed", 0.0), ("max_speed", 1.5), ("k_omega", -1.0)]
    bad += [(k, v) for k in R.FIELDS for v in (float("nan"), float("inf"), float("-inf"))]
    for k, v in bad:
        st = _lib.HybridParamsStruct()
        built_lib.mrca_hybrid_default_params(C.byref(st))
        setattr(st, k, v)
        err = built_lib.mrca_last_error() if call(st) == -1 else b"accepted"
        assert (k.encode() in err or (k == "stop_dist" and b"risk_dist" in err)) and b"env is NULL" not in err, (k, v, err)
    # the edges of the table are inside it: these get as far as the env
    for k, v in [("stop_dist", 0.0), ("risk_dist", 6.0), ("safe_scale", 0.0), ("safe_scale", 1.0), ("look", 6.0), ("front_cos", -1.0),
                 ("front_cos", 1.0), ("max_speed", 1.0), ("k_omega", 0.0), ("v_pid", 5.0)]:
        st = _lib.HybridParamsStruct()
        built_lib.mrca_hybrid_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(st) == -1 and b"env is NULL" in built_lib.mrca_last_error(), (k, v, built_lib.mrca_last_error())
    assert (out == 7.0).all()
