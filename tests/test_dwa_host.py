"""The DWA baseline controller's rule (csrc/mrca_dwa_device.h) compiled for the host with g++ -ffp-contract=off: the very
functions the gfx950 kernel calls, held EQUAL bit for bit to the NumPy float32 restatement of tests/dwa_ref.py (sector
reduction, window, rollout, clearance, score, choice -- with the coverage of the branches asserted from the restatement's
diagnostics, not hoped for), the choice checked against a brute-force argmax, the rule driven in closed loop on the C oracle's
env (the behaviour gates of the controller's defaults), and the library's validation table.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dwa_cases as K
import dwa_ref as R
import util as U
from dwa_cases import crafted  # noqa: F401  (the crafted rows live in tests/dwa_cases.py; tests/test_gpu_dwa.py runs them too)
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include "mrca_dwa_device.h"
using namespace mrca;
// every robot from host copies of its fields; pts[N][64][2], beam[N][64], adm / clear / scores [N][nv * nw]
extern "C" void shim_env(const DwaParams* q, int N, const float* goal, const float* speed, const float* rows, int beams,
                         const float* bc, const float* bs, float* act, int* choice, float* score, float* pts, int* beam,
                         uint8_t* adm, float* clear, float* scores) {
    const int C = q->nv * q->nw;
    for (int n = 0; n < N; ++n)
        dwa_robot(*q, goal + 2 * n, speed + 2 * n, rows + (size_t)n * beams, beams, bc, bs, act + 2 * n, choice + n, score + n,
                  pts ? pts + (size_t)n * 2 * kDwaSectors : nullptr, beam ? beam + (size_t)n * kDwaSectors : nullptr,
                  adm ? adm + (size_t)n * C : nullptr, clear ? clear + (size_t)n * C : nullptr, scores ? scores + (size_t)n * C : nullptr);
}
extern "C" float shim_sample(float lo, float hi, int i, int n) { return dwa_sample(lo, hi, i, n); }
extern "C" float shim_score_roundtrip(float s) { return dwa_ordered_score(dwa_ordered_bits(s)); }
extern "C" uint32_t shim_ordered_bits(float s) { return dwa_ordered_bits(s); }
"""


class Params(C.Structure):
    _fields_ = [(k, C.c_int32 if k in R.INTS else C.c_float) for k in R.FIELDS]


def cparams(p):
    return Params(**{k: (int(v) if k in R.INTS else float(v)) for k, v in p.items()})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("dwa_host")
    src, so = d / "shim.cpp", d / "libdwa_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    lib.shim_env.argtypes = [C.POINTER(Params), C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, ip, fp, fp, ip, vp, fp, fp]
    lib.shim_sample.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int]
    lib.shim_sample.restype = C.c_float
    lib.shim_score_roundtrip.argtypes = [C.c_float]
    lib.shim_score_roundtrip.restype = C.c_float
    lib.shim_ordered_bits.argtypes = [C.c_float]
    lib.shim_ordered_bits.restype = C.c_uint32
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, f32)), bits(np.asarray(b, f32)))


def host_env_actions(shim, p, local_goal, speed, rows, want_diag=False):
    """The host build of the rule on every robot -> (actions, choice, score, diag or None)"""
    local_goal, speed, rows = (np.ascontiguousarray(t, f32) for t in (local_goal, speed, rows))
    N, B = rows.shape
    bc, bs = (np.ascontiguousarray(t, f32) for t in U.O.beam_table(f32, B))
    Cn = p["nv"] * p["nw"]
    act, choice, score = np.zeros((N, 2), f32), np.zeros(N, np.int32), np.zeros(N, f32)
    diag = None
    if want_diag:
        diag = dict(pts=np.zeros((N, 64, 2), f32), beam=np.zeros((N, 64), np.int32), admissible=np.zeros((N, Cn), np.uint8),
                    clear=np.zeros((N, Cn), f32), score=np.zeros((N, Cn), f32))
    q = cparams(p)
    shim.shim_env(C.byref(q), N, _fp(local_goal), _fp(speed), _fp(rows), B, _fp(bc), _fp(bs), _fp(act), _ip(choice), _fp(score),
                  None if diag is None else _fp(diag["pts"]), None if diag is None else _ip(diag["beam"]),
                  None if diag is None else diag["admissible"].ctypes.data, None if diag is None else _fp(diag["clear"]),
                  None if diag is None else _fp(diag["score"]))
    return act, choice, score, diag


def assert_equal_to_ref(shim, p, goal, speed, rows):
    """host build == restatement on every output and every diagnostic -> (the restatement's outputs and diagnostics)"""
    act, choice, score, d = host_env_actions(shim, p, goal, speed, rows, want_diag=True)
    wact, wchoice, wscore, wd = R.env_actions(p, goal, speed, rows)
    assert np.array_equal(wd["beam"], d["beam"]), np.argwhere(wd["beam"] != d["beam"])[:5]
    assert same_bits(wd["px"], d["pts"][..., 0]) and same_bits(wd["py"], d["pts"][..., 1])
    assert same_bits(wd["clear"], d["clear"]), np.argwhere(bits(wd["clear"]) != bits(d["clear"]))[:5]
    assert same_bits(wd["score"], d["score"]), np.argwhere(bits(wd["score"]) != bits(d["score"]))[:5]
    assert np.array_equal(wd["admissible"], d["admissible"].astype(bool))
    assert np.array_equal(wchoice, choice), (wchoice, choice)
    assert same_bits(wact, act) and same_bits(wscore, score)
    return wact, wchoice, wscore, wd


# ------------------------------------------------------------------------------------------------ equality with dwa_ref
def random_inputs(rng, N, B):
    rows = rng.uniform(0.05, 6.0, (N, B)).astype(f32)
    rows[rng.random((N, B)) < 0.5] = 6.0                 # half the beams see nothing
    rows[: N // 3] = np.maximum(rows[: N // 3], f32(1.2))                # a third of the robots have room around them
    th = rng.uniform(-np.pi, np.pi, N)
    dist = rng.uniform(0.0, 8.0, N)
    dist[::5] = rng.uniform(0.0, 0.7, len(dist[::5]))                    # near and inside the goal radius
    goal = np.stack([dist * np.cos(th), dist * np.sin(th)], 1).astype(f32)
    speed = np.stack([rng.uniform(0, 1, N), rng.uniform(-1, 1, N)], 1).astype(f32)
    return goal, speed, rows


PARAM_SETS = [
    R.params(),
    R.params(acc_v=1.0, acc_w=2.0, obst_dist=6.0),                       # a window that is a part of the range
    R.params(nv=1, nw=1, steps=1),
    R.params(nv=16, nw=64, steps=3, horizon=0.7, clear_cap=0.4, radius=0.3),
    R.params(nv=3, nw=4, steps=64, max_speed=0.6, max_omega=0.5, w_goal=0.0, w_speed=2.0),
    R.params(obst_dist=0.0),                                             # nothing counts: no point anywhere
    R.params(acc_v=0.0, acc_w=0.0, nv=2, nw=2),                          # a window that is one point
]


@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_random_inputs_equal_the_reference(shim, beams):
    rng = np.random.default_rng(beams)
    goal, speed, rows = random_inputs(rng, 24, beams)
    seen = set()
    for p in PARAM_SETS:
        _a, choice, _s, _d = assert_equal_to_ref(shim, p, goal, speed, rows)
        seen |= {"blocked" if c == R.BLOCKED else "at_goal" if c == R.AT_GOAL else "chosen" for c in choice.tolist()}
    assert seen == {"blocked", "at_goal", "chosen"}


def test_crafted_inputs_take_every_branch(shim):
    """tests/dwa_cases.py: ``crafted`` and what each of its rows is made for"""
    B = 192
    names, goal, speed, rows = crafted(B)
    p = R.params()
    act, choice, score, d = assert_equal_to_ref(shim, p, goal, speed, rows)
    K.expectations(names, p, B, act, choice, score, d)


def test_a_tie_goes_to_the_lower_candidate(shim):
    """Goal dead ahead in the open with two candidates, (1, -1) and (1, +1): mirror arcs, EQUAL scores -- c = 0 wins.  And with
    only the clearance weighted, all 105 candidates of the default grid tie (no point: every clearance is the cap), as do the
    1024 of the largest grid."""
    _names, goal, speed, rows = crafted(64)
    sel = [K.TIE_ROW]
    for name, grid in K.TIE_GRIDS.items():
        act, choice, score, d = assert_equal_to_ref(shim, R.params(**grid), goal[sel], speed[sel], rows[sel])
        K.tie_expectations(name, act, choice, d)


@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_sector_counts_special_values_and_winner_places(shim, beams):
    """The rest of tests/dwa_cases.py, which the GPU test puts into an env: rows with 0 ... 64 occupied sectors, goals and speeds
    that are no numbers, and the params under which the winner sits in each place of the kernel's deal."""
    p = R.params()
    rows = K.sector_rows(beams)
    n = len(rows)
    _a, _c, _s, d = assert_equal_to_ref(shim, p, np.tile(f32(K.SECTOR_GOAL), (n, 1)), np.tile(f32([0.5, 0.0]), (n, 1)), rows)
    K.sector_expectations(d)
    _names, goal, speed, rows = K.special(beams)
    act, choice, _s, d = assert_equal_to_ref(shim, p, goal, speed, rows)
    K.special_expectations(p, act, choice, d)
    kinds = set()
    for grid, g in K.WINNER_SETS:
        q = R.params(**grid)
        _a, choice, _s, _d = assert_equal_to_ref(shim, q, f32([g]), f32([[0.5, 0.0]]), np.full((1, beams), 6.0, f32))
        kinds |= K.winner_kinds(q, int(choice[0]))
    assert kinds == K.WINNER_KINDS, kinds


def test_choice_is_the_brute_force_argmax(shim):
    rng = np.random.default_rng(11)
    goal, speed, rows = random_inputs(rng, 40, 128)
    names, cg, cs, cr = crafted(128)
    goal, speed, rows = np.concatenate([goal, cg]), np.concatenate([speed, cs]), np.concatenate([rows, cr])
    for p in (R.params(), R.params(w_goal=0.0, w_heading=0.0, w_speed=0.0), R.params(nv=16, nw=64, steps=2)):
        act, choice, score, d = host_env_actions(shim, p, goal, speed, rows, want_diag=True)
        _wa, wchoice, _ws, wd = R.env_actions(p, goal, speed, rows)
        for n in range(len(goal)):
            best, best_s = R.BLOCKED, None
            for c in range(p["nv"] * p["nw"]):
                s = wd["score"][n, c]
                if wd["admissible"][n, c] and (best_s is None or s > best_s):      # strictly greater: the lowest c among equals
                    best, best_s = c, s
            if wd["at_goal"][n]:
                best = R.AT_GOAL
            assert choice[n] == best == wchoice[n], (n, choice[n], best)
            if best >= 0:
                assert same_bits(score[n], best_s)
                assert same_bits(act[n], [wd["v"][n, best], wd["w"][n, best]])


def test_samples_and_the_score_key(shim):
    for n in (1, 2, 3, 5, 16, 21, 64):
        got = [shim.shim_sample(-1.0, 1.0, i, n) for i in range(n)]
        want = R.sample(np.array([-1.0], f32), np.array([1.0], f32), np.arange(n), n)[0]
        assert same_bits(got, want)
        assert got[-1] == 1.0 and (n == 1 or got[0] == -1.0)
        assert got == [-v for v in got[::-1]] or n == 1                  # a symmetric window gives symmetric samples
        assert all(a < b for a, b in zip(got, got[1:]))
    lo, hi = f32(0.123), f32(0.877)
    for n in (2, 5, 16):
        got = [shim.shim_sample(lo, hi, i, n) for i in range(n)]
        assert same_bits(got, R.sample(np.array([lo]), np.array([hi]), np.arange(n), n)[0]) and got[0] == lo and got[-1] == hi
    vals = np.array([-np.inf, -3.5, -1e-30, 0.0, 1e-30, 0.25, 7.0, np.inf], f32)
    keys = [shim.shim_ordered_bits(float(v)) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert keys == R.ordered_bits(vals).tolist()
    assert all(same_bits(shim.shim_score_roundtrip(float(v)), v) for v in vals)


# ------------------------------------------------------------------------------------------------ closed loop on the C oracle
TICKS_BLOCK = 74            # measured: the block gate with the defaults
BUDGET_BLOCK = 111          # 1.5 x


def closed_loop(shim, sc, p, ticks, poses=None, goals=None):
    """-> (env, ticks run, the commands of every tick)"""
    env = U.COracleEnv(sc)
    env.reset(None, poses, goals)
    cmds = []
    for k in range(ticks):
        act, _c, _s, _d = host_env_actions(shim, p, env.local_goal, env.speed, env.scan)
        cmds.append(act)
        env.step(act)
        if (env.first_result != 0).all():
            break
    return env, k + 1, np.stack(cmds)


def test_gate_goal_behind_a_block(shim):
    """A lone robot drives along y = 0.4 at a 1 m wide block (y in [-0.5, 0.5]) with its goal 3 m behind it: the way round is
    shorter on the left.  Measured with the defaults: the goal is reached after TICKS_BLOCK = 74 ticks without a crash (75 to 80 from y = 0.2, 0 and -0.3); the budget is
    1.5 x that (the C oracle is deterministic: the margin only covers a later retuning of the defaults)."""
    grid = U.small_grid(blocks=[(0.0, -0.5, 0.5, 0.5)])
    sc = S.circle_n(1, 4.0, grid=grid)
    env, ticks, _cmds = closed_loop(shim, sc, R.params(), BUDGET_BLOCK, np.array([[-3.0, 0.4, 0.0]], f32), np.array([[3.5, 0.4]], f32))
    print("goal behind a block: result", env.first_result, "ticks", ticks)
    assert env.first_result[0] == 1 and not env.crashed.any(), (env.first_result, env.pose, ticks)


def test_gate_wall_with_the_goal_behind_it(shim):
    """A robot 1.5 m from the arena's wall, facing it, with its goal behind the wall: it can never arrive, and it must not
    crash in 300 ticks."""
    grid = U.small_grid()
    sc = S.circle_n(1, 4.0, grid=grid)
    env, ticks, cmds = closed_loop(shim, sc, R.params(), 300, np.array([[8.3, 0.0, 0.0]], f32), np.array([[12.0, 0.0]], f32))
    print("wall with the goal behind it: result", env.first_result, "ticks", ticks, "pose", env.pose)
    assert ticks == 300 and not env.crashed.any() and env.first_result[0] == 0, (env.first_result, env.pose)
    assert np.isfinite(cmds).all()


def test_gate_a_perturbed_circle_is_reported(shim):
    """Ten robots across a circle of 4 m radius, every start 0.2 m / 0.1 rad off (seed 0).  REPORTED, not gated on the outcome
    (a sensor-level rule that takes moving robots for standing obstacles is not expected to solve this): the gate is that no
    command is a NaN and every command lies inside its bounds."""
    sc = S.circle_n(10, 4.0, grid=S.empty_grid())
    rng = np.random.default_rng(0)
    poses = np.asarray(sc.init_table, f32).copy()
    poses[:, :2] += rng.uniform(-0.2, 0.2, (10, 2)).astype(f32)
    poses[:, 2] += rng.uniform(-0.1, 0.1, 10).astype(f32)
    p = R.params()
    env, ticks, cmds = closed_loop(shim, sc, p, 400, poses, np.asarray(sc.goal_table, f32))
    fr = env.first_result
    print("perturbed 10-robot circle: SR", float((fr == 1).mean()), "crashes", int((fr == 2).sum()), "unfinished", int((fr == 0).sum()),
          "ticks", ticks)
    assert np.isfinite(cmds).all()
    assert (cmds[..., 0] >= 0).all() and (cmds[..., 0] <= p["max_speed"]).all() and (np.abs(cmds[..., 1]) <= p["max_omega"]).all()



# ------------------------------------------------------------------------------------------------ the library's own defaults
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.dwa import DwaParams
    assert built_lib.mrca_dwa_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.DwaParamsStruct()
    assert built_lib.mrca_dwa_default_params(C.byref(st)) == 0
    got = {k: getattr(st, k) for k in R.FIELDS}
    assert got == {k: (v if k in R.INTS else float(f32(v))) for k, v in R.DEFAULTS.items()}
    assert [n for n, _t in _lib.DwaParamsStruct._fields_] == R.FIELDS and C.sizeof(st) == 60
    p = DwaParams(radius=0.4)
    assert p.radius == 0.4 and p.nw == 21 and p.struct().horizon == 2.0
    assert DwaParams.from_assignments(["horizon=1.5", "nw=31"]).nw == 31
    with pytest.raises(ValueError):
        DwaParams.from_assignments(["nonsense=1"])
    # a rejected call touches nothing: `out` stands where the device buffers would (host memory -- no call gets as far as a launch)
    out = np.full(64, 7.0, f32)
    ptr = C.c_void_p(out.ctypes.data)
    assert out.ctypes.data % 8 == 0

    def call(params=None, actions=ptr, choice=None, score=None):
        return built_lib.mrca_dwa_actions(None, None if params is None else C.byref(params), None, actions, choice, score, None)
    # what can be judged without an env is judged before the env is looked at
    assert call() == -1 and b"env is NULL" in built_lib.mrca_last_error()
    assert call(actions=None) == -1 and b"actions_dev is NULL" in built_lib.mrca_last_error()
    assert call(actions=C.c_void_p(out.ctypes.data + 4)) == -1 and b"8-byte aligned" in built_lib.mrca_last_error()
    bad = [("radius", 0.0), ("radius", -1.0), ("horizon", 0.0), ("clear_cap", 0.0), ("max_speed", 0.0), ("max_omega", 0.0),
           ("max_speed", 1.5), ("max_omega", 1.0001), ("obst_dist", -0.1), ("obst_dist", 6.5), ("acc_v", -1.0), ("acc_w", -0.5),
           ("w_goal", -1.0), ("w_heading", -1.0), ("w_clear", -1.0), ("w_speed", -1.0), ("steps", 0), ("steps", 65), ("nv", 0),
           ("nv", 17), ("nw", 0), ("nw", 65)]
    bad += [(k, v) for k in R.FIELDS if k not in R.INTS for v in (float("nan"), float("inf"), float("-inf"))]
    for k, v in bad:
        st = _lib.DwaParamsStruct()
        built_lib.mrca_dwa_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(st) == -1 and k.encode() in built_lib.mrca_last_error() and b"env is NULL" not in built_lib.mrca_last_error(), \
            (k, v, built_lib.mrca_last_error())
    # the edges of the table are inside it: these get as far as the env
    for k, v in [("obst_dist", 0.0), ("obst_dist", 6.0), ("max_speed", 1.0), ("acc_v", 0.0), ("w_clear", 0.0), ("steps", 64), ("nv", 16),
                 ("nw", 64), ("steps", 1), ("nv", 1), ("nw", 1)]:
        st = _lib.DwaParamsStruct()
        built_lib.mrca_dwa_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(st) == -1 and b"env is NULL" in built_lib.mrca_last_error(), (k, v, built_lib.mrca_last_error())
    assert (out == 7.0).all()
