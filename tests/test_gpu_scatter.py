"""GPU: mrca_scatter -- poses, goals and tries EQUAL (the floats bit for bit) to the NumPy float32 restatement of
tests/scatter_ref.py on the cases of tests/scatter_cases.py: one lane's worth of robots, a full wave, the 256-lane block with a
partial last wave, 300 robots, one world and three, more rounds than one, max_tries that are no multiple of the block, boxes
that leave the map, an infeasible box.  The call is valid before the first reset, writes its three buffers and nothing else,
replays from a captured graph, and hands mrca_reset a start state no robot crashes in; a closed loop from it equals the C
oracle's; every refusal with its whole text; ``mrca.evaluate --scenario swap``."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scatter_cases as SC
import scatter_ref as R
import util as U
from util import S

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
NAN_BITS = 0x7FC0BEEF


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def scenario_of(grid, W, Rn, seed=SC.SEED):
    """W worlds of Rn table robots on ``grid``, nothing resets; the smallest scans the env takes (the sampler reads none)"""
    mode = np.full(Rn, S.RESET_TABLE, np.int32)
    return S.Scenario("scatter_case", W, Rn, grid, timeout=1000, w_thresh=0.7, pre_dist_zero=True, auto_reset=S.AUTO_NONE, seed=seed,
                      beams=64, frames=1, reset_mode=mode, goal_mode=mode.copy())


def params_of(p):
    from mrca.scatter import ScatterParams
    return ScatterParams(**p)


def poisoned(env):
    """(poses, goals, tries) filled with what no call writes"""
    return (torch.full((env.N, 3), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32),
            torch.full((env.N, 2), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32),
            torch.full((env.N, 2), -7, dtype=torch.int32, device=env.device))


def bits(t):
    return t.detach().cpu().numpy().view(u32)


def assert_same(got, want, what):
    torch.cuda.synchronize()
    for g, w, name in zip(got[:2], want[:2], ("poses", "goals")):
        assert np.array_equal(bits(g), w.view(u32)), (what, name, np.argwhere(bits(g) != w.view(u32))[:5])
    assert np.array_equal(got[2].cpu().numpy(), want[2]), (what, "tries", np.argwhere(got[2].cpu().numpy() != want[2])[:5])


# ------------------------------------------------------------------------------------------------ equality with scatter_ref
@pytest.mark.parametrize("name", SC.GPU_CASES)
def test_the_library_equals_the_restatement(hip, name):
    grid, W, Rn, boxes, p, want = SC.case(name)
    env = hip.VecStageWorld(scenario_of(grid, W, Rn))
    out = poisoned(env)
    got = env.scatter(boxes, params_of(p), out=out)          # BEFORE the first reset: it reads the map, the geometry and the key
    assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2]
    assert_same(got, want, name)
    # tries_dev = NULL: the same poses and goals
    again = poisoned(env)
    st = params_of(p).struct()
    rc = env.lib.mrca_scatter(env._h, C.byref(st), C.c_void_p(env._scatter_boxes[1].data_ptr()), C.c_void_p(again[0].data_ptr()),
                              C.c_void_p(again[1].data_ptr()), None, env._stream())
    assert rc == 0, env.lib.mrca_last_error()
    torch.cuda.synchronize()
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))
    env.check()
    env.close()


def test_the_scenarios_own_boxes_and_overrides(hip):
    """boxes and params default to the scenario's; the uploaded boxes are kept until other boxes come"""
    sc = S.random_box(robots=6, num_worlds=2, seed=11)
    env = hip.VecStageWorld(sc)
    poses, goals, tries = env.scatter()
    kept = env._scatter_boxes[1]
    want = R.scatter(R.params(**sc.scatter), sc.grid, sc.seed, 2, 6, sc.boxes)
    assert_same((poses, goals, tries), want, "random_box")
    assert (want[2] > 0).all()
    env.scatter()
    assert env._scatter_boxes[1] is kept
    other = sc.boxes * 0.5
    got = env.scatter(other, params_of(R.params(draw=4, **sc.scatter)))
    assert env._scatter_boxes[1] is not kept
    assert_same(got, R.scatter(R.params(draw=4, **sc.scatter), sc.grid, sc.seed, 2, 6, other), "half boxes, draw 4")
    with pytest.raises(ValueError, match="row 0 has sx0 > sx1"):
        env.scatter(sc.boxes[:, [2, 1, 0, 3, 4, 5, 6, 7]])
    bare = hip.VecStageWorld(scenario_of(S.empty_grid(), 1, 2))
    with pytest.raises(ValueError, match="no boxes"):
        bare.scatter()
    bare.close()
    env.close()


# ------------------------------------------------------------------------------------------------ what the call writes
def test_the_call_writes_its_three_buffers_only(hip):
    """every env field and every other byte of the arena as they were -- before the first reset and behind ticks -- and the
    bytes around the three outputs, which stand in ONE allocation between guard words"""
    grid, W, Rn, boxes, p, want = SC.case("doorway_clear4")
    sc = scenario_of(grid, W, Rn)
    sc.beams, sc.frames = 512, 3
    env = hip.VecStageWorld(sc, lazy_obs=False)
    N, pad = env.N, 64
    flat = torch.full((pad + 3 * N + pad + 2 * N + pad + 2 * N + pad,), 0x5A5A5A5A, dtype=torch.int32, device=env.device)
    o1 = pad
    o2 = o1 + 3 * N + pad
    o3 = o2 + 2 * N + pad
    out = (flat[o1:o1 + 3 * N].view(torch.float32).view(N, 3), flat[o2:o2 + 2 * N].view(torch.float32).view(N, 2), flat[o3:o3 + 2 * N].view(N, 2))
    guard = torch.ones_like(flat, dtype=torch.bool)
    for o, n in ((o1, 3 * N), (o2, 2 * N), (o3, 2 * N)):
        guard[o:o + n] = False
    names = U.STATE_FIELDS + ["scan_ring", "ring_head", "hit_bits", "fresh"]
    rng = np.random.default_rng(8)
    for stage in ("before the first reset", "behind three ticks"):
        if stage != "before the first reset":
            env.reset()
            for _ in range(3):
                env.step(torch.from_numpy(U.random_actions(rng, N)).cuda())
        torch.cuda.synchronize()
        fields = {k: getattr(env, k).clone() for k in names}
        arena = env.arena.clone()
        flat.fill_(0x5A5A5A5A)
        env.scatter(boxes, params_of(p), out=out)
        assert_same(out, want, stage)
        for k in names:
            assert torch.equal(fields[k], getattr(env, k)), (stage, k)
        assert torch.equal(arena, env.arena), stage              # not a byte of the env's memory
        assert bool((flat[guard] == 0x5A5A5A5A).all()), stage    # ... nor one beside an output
        assert not bool((flat[~guard] == 0x5A5A5A5A).any())      # ... and every word of the outputs
    env.check()
    env.close()


def test_a_captured_call_replays_as_the_eager_call(hip):
    grid, W, Rn, boxes, p, want = SC.case("open_R130_W3")
    env = hip.VecStageWorld(scenario_of(grid, W, Rn))
    q = params_of(p)
    eager = env.scatter(boxes, q, out=poisoned(env))
    out = poisoned(env)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.scatter(boxes, q, out=out)                       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        env.scatter(boxes, q, out=out)
    for _ in range(2):
        for t, fill in zip(out, (float("nan"), float("nan"), -7)):
            t.fill_(fill)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_same(out, want, "replay")
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ what mrca_reset makes of it
@pytest.mark.parametrize("name", ["doorway_clear4", "open_R65_W1"])
def test_reset_takes_the_outputs_and_nobody_crashes(hip, name):
    from mrca import _lib
    grid, W, Rn, boxes, p, want = SC.case(name)
    assert (want[2] > 0).all()                               # a feasible case
    env = hip.VecStageWorld(scenario_of(grid, W, Rn))
    poses, goals, _tries = env.scatter(boxes, params_of(p))
    env.reset(None, poses, goals)
    torch.cuda.synchronize()
    assert [n for n, _d, _s in _lib.FIELDS][:4] == ["pose", "speed", "speed_gt", "goal"]       # MRCA_F_POSE, MRCA_F_GOAL
    assert np.array_equal(bits(env.pose), want[0].view(u32)) and np.array_equal(bits(env.goal), want[1].view(u32))
    assert np.array_equal(bits(env.init_pose), want[0].view(u32))
    assert not bool(env.crashed.any()) and not bool(env.done.any())
    env.step(torch.zeros((env.N, 2), device=env.device))
    torch.cuda.synchronize()
    assert not bool(env.crashed.any()) and bool((env.result != 2).all()) and bool((env.first_result != 2).all())
    assert np.array_equal(bits(env.pose[:, :2]), want[0][:, :2].view(u32))      # nobody moved
    env.check()
    env.close()


def test_forty_closed_loop_ticks_equal_the_oracle(hip):
    """random_box(robots=6), two worlds, the go-to-goal stand-in: the device and the C oracle from the same (poses, goals)"""
    from mrca.evaluate import go_to_goal_policy
    sc = S.random_box(robots=6, num_worlds=2, seed=7)
    env = hip.VecStageWorld(sc)
    ora = U.COracleEnv(sc)
    poses, goals, tries = env.scatter()
    torch.cuda.synchronize()
    assert bool((tries > 0).all())
    env.reset(None, poses, goals)
    ora.reset(None, poses.cpu().numpy(), goals.cpu().numpy())
    U.assert_state_equal(U.HostView(env), ora, what="reset")
    moved = 0.0
    for k in range(40):
        a = go_to_goal_policy(env.obs, env.local_goal, env.speed).float().contiguous()
        env.step(a)
        ora.step(a.cpu().numpy())
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
        U.assert_hits_equal(env, ora, what=f"tick {k}")
        moved += float(a[:, 0].sum())
    assert moved > 10.0                                       # they drive
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(hip):
    """every refusal with the whole text of mrca_last_error(); a refused call launches nothing and writes nothing"""
    from mrca import _lib
    env = hip.VecStageWorld(scenario_of(S.empty_grid(), 2, 3))
    lib, h, st_ = env.lib, env._h, env._stream()
    boxes = torch.from_numpy(SC.same_box(3, SC.WIDE)).to(env.device)
    out = poisoned(env)
    before = [t.clone() for t in out]

    def call(over=None, boxes=boxes.data_ptr(), poses=out[0].data_ptr(), goals=out[1].data_ptr(), tries=out[2].data_ptr(), handle=h):
        st = _lib.ScatterParamsStruct()
        assert lib.mrca_scatter_default_params(C.byref(st)) == 0
        for k, v in (over or {}).items():
            setattr(st, k, v)
        rc = lib.mrca_scatter(handle, C.byref(st), *[None if a is None else C.c_void_p(a) for a in (boxes, poses, goals, tries)], st_)
        return rc, lib.mrca_last_error().decode()

    for k in R.FIELDS[:4]:
        for v in (float("nan"), float("inf"), float("-inf")):
            assert call({k: v}) == (-1, f"mrca_scatter: {k} is not finite")
    assert call({"min_sep": float(np.nextafter(f32(0.6), f32(0)))}) == (-1, "mrca_scatter: min_sep must be >= 0.6")
    assert call({"min_sep": 0.1}) == (-1, "mrca_scatter: min_sep must be >= 0.6")
    assert call({"goal_sep": -0.01}) == (-1, "mrca_scatter: goal_sep must be >= 0")
    assert call({"goal_min": -1.0}) == (-1, "mrca_scatter: goal_min must be >= 0")
    assert call({"goal_min": 7.0, "goal_max": 6.0}) == (-1, "mrca_scatter: goal_max must be >= goal_min")
    assert call({"clear_cells": -1}) == (-1, "mrca_scatter: clear_cells -1 outside 0..254")
    assert call({"clear_cells": 255}) == (-1, "mrca_scatter: clear_cells 255 outside 0..254")
    assert call({"max_tries": 0}) == (-1, "mrca_scatter: max_tries 0 outside 1..65536")
    assert call({"max_tries": 65537}) == (-1, "mrca_scatter: max_tries 65537 outside 1..65536")
    assert call(boxes=None) == (-1, "mrca_scatter: boxes_dev is NULL")
    assert call(poses=None) == (-1, "mrca_scatter: poses_dev is NULL")
    assert call(goals=None) == (-1, "mrca_scatter: goals_dev is NULL")
    assert call(poses=out[0].data_ptr() + 2) == (-1, "mrca_scatter: poses_dev must be 4-byte aligned")
    assert call(goals=out[1].data_ptr() + 4) == (-1, "mrca_scatter: goals_dev must be 8-byte aligned")
    assert call(tries=out[2].data_ptr() + 2) == (-1, "mrca_scatter: tries_dev must be 4-byte aligned")
    assert call(handle=None) == (-1, "env is NULL")
    torch.cuda.synchronize()
    for a, b in zip(out, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the edges of the table are inside it
    assert call({"min_sep": float(f32(0.6)), "goal_sep": 0.0, "goal_min": 0.0, "goal_max": 0.0, "clear_cells": 254, "max_tries": 1})[0] == 0
    env.check()
    env.close()
    # a world of more robots than the placed points have room for in LDS
    big = S.circle_big(4097)
    big.beams, big.frames = 64, 1
    env = hip.VecStageWorld(big)
    boxes = torch.from_numpy(SC.same_box(4097, (-300.0, -300.0, 300.0, 300.0))).to(env.device)
    out = poisoned(env)
    st = _lib.ScatterParamsStruct()
    lib.mrca_scatter_default_params(C.byref(st))
    rc = lib.mrca_scatter(env._h, C.byref(st), C.c_void_p(boxes.data_ptr()), C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                          C.c_void_p(out[2].data_ptr()), env._stream())
    assert (rc, lib.mrca_last_error().decode()) == \
        (-4, "mrca_scatter: robots_per_world 4097 > 4096 (a world's placed points are held in 32 KB of LDS)")
    with pytest.raises(RuntimeError, match="robots_per_world 4097 > 4096"):
        env.scatter(boxes.cpu().numpy())
    torch.cuda.synchronize()
    assert bool((out[2] == -7).all())
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ the command line
def _evaluate(args):
    cmd = [sys.executable, "-m", "mrca.evaluate"] + args
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), os.environ.get("PYTHONPATH", "")]))
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)


SWAP = ["--scenario", "swap", "--circles", "2", "--robots", "8", "--max-ticks", "60"]


def test_cli_swap(hip):
    run = _evaluate(SWAP)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout)
    assert {"scenario", "scatter_params", "scatter_draw", "scatter_max_tries_used"} <= set(out)
    assert out["scenario"] == "swap" and out["robots"] == 16 and out["scatter_draw"] == 0 == out["scatter_params"]["draw"]
    assert out["scatter_params"] == dict(R.DEFAULTS, min_sep=1.0) and 1 <= out["scatter_max_tries_used"] <= 1024
    assert {"success_rate", "crash_rate", "unfinished_rate"} <= set(out) and out["ticks_run"] == 60
    sc = S.group_swap(robots=8, num_worlds=2, seed=0, timeout=60)
    want = R.scatter(R.params(**sc.scatter), sc.grid, 0, 2, 8, sc.boxes)
    assert out["scatter_max_tries_used"] == int(want[2].max())


def test_cli_refuses_a_min_sep_below_the_footprints(hip):
    run = _evaluate(SWAP + ["--scatter-param", "min_sep=0.1"])
    assert run.returncode == 2 and run.stdout == ""
    assert "mrca_scatter: min_sep must be >= 0.6" in run.stderr


def test_cli_refuses_more_robots_than_the_boxes_take(hip):
    run = _evaluate(["--scenario", "swap", "--circles", "2", "--robots", "40", "--max-ticks", "60"])
    assert run.returncode == 2 and run.stdout == ""
    assert "group_swap: 20 robots in a box of 40 m^2" in run.stderr and "more than 30 %" in run.stderr
