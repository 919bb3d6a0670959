"""GPU: the planner's per-tick call with line of sight (mrca_subgoals_los) and the three controllers steered at the caller's rows
(mrca_dwa_actions_goal, mrca_hybrid_actions_goal, mrca_hybrid_plan_goal).  The kernel's five outputs EQUAL, bit for bit, to the
restatement of tests/planner_los_ref.py fed with the fields mrca_goal_fields planned on the device: the host test's crafted poses
and random finite cells, 1 / 37 / 300 robots, a world of 80, masks, default and explicit slots, the list of reaches, a captured
call; equality with mrca_subgoals for reach <= lookahead; the _goal entries equal to their siblings on a copy of
MRCA_F_LOCAL_GOAL and on NULL, and to their NumPy restatements on the line-of-sight subgoals; the closed loop on the doorway
scenario against the CPU closed loop; and the evaluator's --planner-los."""
import ctypes as C

import numpy as np
import pytest
import torch

import dwa_ref
import hybrid_ref
import planner_cases as PC
import planner_los_ref as LR
import planner_ref as R
import safe_ref
import util as U
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 12345
NAN_BITS = 0x7FC12345


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def planner_params(p):
    from mrca.planner import PlannerParams
    return PlannerParams(**{k: int(p[k]) for k in R.FIELDS})


def los_params(reach):
    from mrca.planner import LosParams
    return LosParams(reach=int(reach))


def sentinels(env):
    nanf = lambda *shape: torch.full(shape, NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)
    return (nanf(env.N, 2), nanf(env.N, 2), nanf(env.N), torch.full((env.N,), SENTINEL, dtype=torch.int32, device=env.device),
            torch.full((env.N, 2), SENTINEL, dtype=torch.int32, device=env.device))


def crafted_env(hip, worlds, robots, rng, **kw):
    """the crafted map, the host test's crafted poses first and random ones behind, the fields planned ON THE DEVICE
    -> (env, fields, names, (grid, p, blocked, the fields read back))"""
    from test_planner_los_host import crafted_case
    grid, p, blocked, want, names, pose, slot, _g = crafted_case(rng)
    env = hip.VecStageWorld(S.stage1(num_worlds=worlds, robots_per_world=robots, grid=grid, seed=5), **kw)
    N = env.N
    if N > len(pose):
        rp, rs = PC.random_poses(rng, N - len(pose), grid)
        pose, slot = np.concatenate([pose, rp]), np.concatenate([slot, rs])
    pose, slot = pose[:N], slot[:N]
    goals = np.where(((slot >= 0) & (slot < len(PC.CRAFTED_GOALS)))[:, None], PC.CRAFTED_GOALS[np.clip(slot, 0, len(PC.CRAFTED_GOALS) - 1)],
                     rng.uniform(-4, 4, (N, 2)).astype(f32)).astype(f32)
    env.reset(None, dev(pose), dev(goals))
    fields = env.plan_goals(dev(PC.CRAFTED_GOALS), planner_params(p))
    fields.slot = dev(slot)
    torch.cuda.synchronize()
    back = fields.field.cpu().numpy().view(np.uint32)
    assert np.array_equal(back, want)
    return env, fields, names[:N], (grid, p, blocked, back)


def check_los(env, fields, case, reach, mask=None, goals=PC.CRAFTED_GOALS, want=None):
    """one call compared with the restatement on the fields read back, every robot and all five outputs -> the restatement's"""
    grid, p, blocked, back = case
    torch.cuda.synchronize()
    pose, goal, lg = env.pose.cpu().numpy(), env.goal.cpu().numpy(), env.local_goal.cpu().numpy()
    slot = (np.arange(env.N) % env.R).astype(np.int32) if fields.slot is None else fields.slot.cpu().numpy()
    if want is None:
        want = LR.subgoals_los(grid, p, reach, back, goals, slot, pose, PC.head_of(pose), goal, blocked)
    out = sentinels(env)
    m = None if mask is None else dev(np.ascontiguousarray(mask, np.uint8))
    got = env.subgoals_los(fields, los_params(reach), mask=m, out=out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, out))
    sel = np.ones(env.N, bool) if mask is None else np.asarray(mask).astype(bool)
    for name, w, g in zip(("local", "subgoal", "dist"), want, got):
        g = bits(g.cpu().numpy())
        w = np.where(sel.reshape((-1,) + (1,) * (g.ndim - 1)), bits(w), np.uint32(NAN_BITS))
        assert np.array_equal(g, w), (name, reach, np.argwhere(g != w)[:5])
    for name, w, g in (("status", want[3], got[3]), ("ahead", want[4], got[4])):
        g = g.cpu().numpy()
        w = np.where(sel.reshape((-1,) + (1,) * (g.ndim - 1)), w, SENTINEL)
        assert np.array_equal(g, w), (name, reach, np.argwhere(g != w)[:5], g[:8], w[:8])
    # local has MRCA_F_LOCAL_GOAL's bits wherever the subgoal has the goal's
    same = sel & (bits(want[1]) == bits(goal)).all(axis=1)
    assert np.array_equal(bits(got[0].cpu().numpy())[same], bits(lg)[same])
    return want


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("worlds,robots", [(1, 1), (1, 37), (4, 75), (1, 80)])
def test_crafted_and_random_poses(hip, worlds, robots):
    """1, 37 and 300 robots are no multiples of a workgroup's 32, a world of 80 robots is more than a wavefront's lanes"""
    rng = np.random.default_rng(31 + robots)
    env, fields, names, case = crafted_env(hip, worlds, robots, rng)
    before = env.arena.clone()
    want = check_los(env, fields, case, 64)
    if env.N >= 21:
        from test_planner_los_host import crafted_los_expectations
        crafted_los_expectations(names, tuple(w[:len(names)] for w in want), env.goal.cpu().numpy(), case[1]["lookahead"])
        assert all((want[3] == v).sum() >= 1 for v in (1, 0, -1, -2))         # explicit slots, -1 and >= G among them
    check_los(env, fields, case, 64, mask=rng.random(env.N) < 0.5)
    check_los(env, fields, case, 64, mask=np.zeros(env.N, np.uint8))
    assert torch.equal(before, env.arena)               # nothing of the env is written
    env.close()


@pytest.mark.parametrize("lanes", ["8", "64"])
def test_both_lane_shapes(hip, lanes, monkeypatch):
    """the library picks a robot's group of lanes by the number of robots (a wavefront up to 8192, eight lanes beyond);
    MRCA_SUBGOAL_LOS_LANES forces one, read at every call: both give the restatement's bits, here on 300 robots"""
    monkeypatch.setenv("MRCA_SUBGOAL_LOS_LANES", lanes)
    rng = np.random.default_rng(35)
    env, fields, _names, case = crafted_env(hip, 4, 75, rng)
    for reach in (5, 64, 256):
        check_los(env, fields, case, reach)
    check_los(env, fields, case, 64, mask=rng.random(env.N) < 0.5)
    env.close()


def test_past_the_size_at_which_the_library_changes_the_shape(hip, monkeypatch):
    """8200 robots (> 8192: the library's own choice is eight lanes there, a wavefront below): the call as the library shapes it
    and both forced shapes write the same bits (each shape is held to the restatement above)"""
    rng = np.random.default_rng(36)
    grid, p, _blocked, want = PC.crafted_fields()
    env = hip.VecStageWorld(S.stage1(num_worlds=82, robots_per_world=100, grid=grid, seed=5))
    pose, slot = PC.random_poses(rng, env.N, grid)
    env.reset(None, dev(pose), dev(rng.uniform(-4, 4, (env.N, 2)).astype(f32)))
    fields = env.plan_goals(dev(PC.CRAFTED_GOALS), planner_params(p))
    fields.slot = dev(slot)
    outs = []
    for lanes in (None, "8", "64"):
        if lanes is None:
            monkeypatch.delenv("MRCA_SUBGOAL_LOS_LANES", raising=False)
        else:
            monkeypatch.setenv("MRCA_SUBGOAL_LOS_LANES", lanes)
        outs.append(env.subgoals_los(fields, los_params(64), out=sentinels(env)))
    torch.cuda.synchronize()
    assert (outs[0][4][:, 0] > 6).any() and all((outs[0][3] == v).any() for v in (1, 0, -1, -2))
    for other in outs[1:]:
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0], other))
    env.close()


@pytest.mark.parametrize("reach", [1, 5, 6, 7, 16, 64, 256])
def test_reaches_and_the_plain_call(hip, reach):
    """the list of reaches (lookahead 6); reach <= lookahead is mrca_subgoals on its four outputs, bit for bit"""
    rng = np.random.default_rng(300 + reach)
    env, fields, _names, case = crafted_env(hip, 8, 8, rng)
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    want = check_los(env, fields, case, reach)
    plain = env.subgoals(fields)
    got = env.subgoals_los(fields, los_params(reach))
    torch.cuda.synchronize()
    equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, got[:4]))
    assert equal == (reach <= case[1]["lookahead"]), reach
    if reach <= case[1]["lookahead"]:
        assert (want[4][:, 0] <= case[1]["lookahead"]).all()
    # only local_dev has to be there; los_params NULL is reach 60
    local = sentinels(env)[0]
    st = fields.params.struct()
    rc = env.lib.mrca_subgoals_los(env._h, C.byref(st), None, C.c_void_p(fields.field.data_ptr()), C.c_void_p(fields.goals.data_ptr()),
                                   fields.num_goals, C.c_void_p(fields.slot.data_ptr()), None, C.c_void_p(local.data_ptr()), None, None, None,
                                   None, env._stream())
    want60 = env.subgoals_los(fields, los_params(60))[0]
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(local.view(torch.int32), want60.view(torch.int32))
    env.close()


@pytest.mark.parametrize("which", ["crafted", "odd", "odd_stride3", "serpentine"])
def test_random_finite_cells_on_fields_planned_on_the_device(hip, which):
    """the host test's 400 robots per map, every branch of the choice among them (asserted there)"""
    from test_planner_los_host import random_case
    grid, p, blocked, fields_ref, goals, pose, slot, env_goal, want, _walks = random_case(which)
    env = hip.VecStageWorld(S.stage1(num_worlds=8, robots_per_world=50, grid=grid, seed=5))
    env.reset(None, dev(pose), dev(env_goal))
    fields = env.plan_goals(dev(goals), planner_params(p))
    fields.slot = dev(slot)
    torch.cuda.synchronize()
    back = fields.field.cpu().numpy().view(np.uint32)
    assert np.array_equal(back, fields_ref)
    check_los(env, fields, (grid, p, blocked, back), 64, goals=goals, want=want)
    env.close()


def test_default_slots_and_their_refusal(hip):
    """slot_dev NULL: robot n walks to goal n % robots_per_world, and only with G == robots_per_world"""
    from mrca.planner import GoalFields
    rng = np.random.default_rng(32)
    G = len(PC.CRAFTED_GOALS)
    env, fields, _names, case = crafted_env(hip, 7, G, rng)
    implicit = GoalFields(fields.field, fields.goals, None, fields.params)
    want = check_los(env, implicit, case, 64)
    assert (want[3] == -2).any() and (want[4][:, 0] > 6).any()
    short = GoalFields(fields.field[:3].contiguous(), fields.goals[:3].contiguous(), None, fields.params)
    with pytest.raises(RuntimeError, match="mrca_subgoals_los: slot_dev NULL .* robots_per_world"):
        env.subgoals_los(short)
    from mrca.planner import LosParams
    bad = LosParams(reach=60)
    bad.reach = 257
    with pytest.raises(RuntimeError, match="reach 257 outside 1..256"):
        env.subgoals_los(fields, bad)
    env.close()


def test_in_a_captured_graph(hip):
    rng = np.random.default_rng(33)
    env, fields, _names, case = crafted_env(hip, 8, 8, rng)
    want = check_los(env, fields, case, 64)
    out = sentinels(env)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        env.subgoals_los(fields, los_params(64), out=out)              # (warm-up outside the capture)
        with torch.cuda.graph(graph, stream=side):
            env.subgoals_los(fields, los_params(64), out=out)
    torch.cuda.synchronize()
    out[3].fill_(SENTINEL)
    out[4].fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[3].cpu().numpy(), want[3]) and np.array_equal(out[4].cpu().numpy(), want[4])
    assert np.array_equal(bits(out[0].cpu().numpy()), bits(want[0]))
    env.close()


# ------------------------------------------------------------------------------------------------ the controllers' goal argument
@pytest.fixture(scope="module")
def moved(hip):
    """21 robots on the crafted map after a few ticks, their line-of-sight subgoals, and host copies of what the controllers read"""
    rng = np.random.default_rng(34)
    env, fields, _names, case = crafted_env(hip, 3, 7, rng)
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    local = env.subgoals_los(fields, los_params(64))[0]
    torch.cuda.synchronize()
    rows = env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()].cpu().numpy()
    policy = np.stack([rng.uniform(0, 1, env.N), rng.uniform(-1, 1, env.N)], 1).astype(f32)
    assert not np.array_equal(bits(local.cpu().numpy()), bits(env.local_goal.cpu().numpy()))
    yield env, local, rows, policy
    env.close()


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_dwa_steered_at_the_callers_rows(moved):
    env, local, rows, _policy = moved
    i32 = lambda: torch.full((env.N,), SENTINEL, dtype=torch.int32, device=env.device)
    fz = lambda: torch.full((env.N,), 7.0, device=env.device)

    def call(**kw):
        choice, score = i32(), fz()
        return env.dwa_actions(choice=choice, score=score, **kw), choice, score
    sibling = call()
    assert same_bits(sibling, call(goal=env.local_goal.clone()))
    arena = env.arena.clone()
    choice, score, act = i32(), fz(), torch.zeros((env.N, 2), device=env.device)
    args = (env._h, None, None, C.c_void_p(act.data_ptr()), C.c_void_p(choice.data_ptr()), C.c_void_p(score.data_ptr()))
    assert env.lib.mrca_dwa_actions_goal(*args, None, env._stream()) == 0            # NULL: MRCA_F_LOCAL_GOAL
    torch.cuda.synchronize()
    assert same_bits(sibling, (act, choice, score))
    got = call(goal=local)
    torch.cuda.synchronize()
    wact, wchoice, wscore, _d = dwa_ref.env_actions(dwa_ref.params(), local.cpu().numpy(), env.speed.cpu().numpy(), rows)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(wact)) and np.array_equal(got[1].cpu().numpy(), wchoice)
    assert np.array_equal(bits(got[2].cpu().numpy()), bits(wscore))
    assert not same_bits(sibling[:1], got[:1]) and torch.equal(arena, env.arena)
    # a mask keeps the other rows
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    out = torch.full((env.N, 2), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)
    env.dwa_actions(mask=dev(mask), out=out, goal=local)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), np.where(mask.astype(bool)[:, None], bits(wact), np.uint32(NAN_BITS)))
    with pytest.raises(RuntimeError, match="mrca_dwa_actions_goal: goal_dev must be 8-byte aligned"):
        env.dwa_actions(goal=torch.zeros(2 * env.N + 1, device=env.device)[1:])


def test_hybrid_steered_at_the_callers_rows(moved):
    env, local, rows, policy = moved
    p = hybrid_ref.params()

    def call(**kw):
        mode = torch.full((env.N,), SENTINEL, dtype=torch.int32, device=env.device)
        clear = torch.full((env.N, 3), 7.0, device=env.device)
        return env.hybrid_actions(dev(policy), mode=mode, clear=clear, **kw), mode, clear
    sibling = call()
    assert same_bits(sibling, call(goal=env.local_goal.clone()))
    act, mode, clear = dev(policy), torch.zeros(env.N, dtype=torch.int32, device=env.device), torch.zeros((env.N, 3), device=env.device)
    args = (env._h, None, None, C.c_void_p(act.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(mode.data_ptr()), C.c_void_p(clear.data_ptr()))
    assert env.lib.mrca_hybrid_actions_goal(*args, None, env._stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(sibling, (act, mode, clear))
    arena = env.arena.clone()
    got = call(goal=local)
    torch.cuda.synchronize()
    wact, wmode, wclear, _nb = hybrid_ref.env_actions(p, local.cpu().numpy(), policy, rows)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(wact)) and np.array_equal(got[1].cpu().numpy(), wmode)
    assert np.array_equal(bits(got[2].cpu().numpy()), bits(wclear))
    assert not np.array_equal(wmode, sibling[1].cpu().numpy()) or not same_bits(sibling[:1], got[:1])
    assert torch.equal(arena, env.arena)


def test_hybrid_plan_steered_at_the_callers_rows(moved):
    env, local, rows, _policy = moved
    p, sp = hybrid_ref.params(), safe_ref.params()

    def call(**kw):
        clear = torch.full((env.N, 3), 7.0, device=env.device)
        mode = torch.full((env.N,), SENTINEL, dtype=torch.int32, device=env.device)
        return env.hybrid_plan(mode=mode, clear=clear, **kw) + (clear,)
    sibling = call()
    assert same_bits(sibling, call(goal=env.local_goal.clone()))
    mode, scale = torch.zeros(env.N, dtype=torch.int32, device=env.device), torch.zeros(env.N, device=env.device)
    pid, clear = torch.zeros((env.N, 2), device=env.device), torch.zeros((env.N, 3), device=env.device)
    rc = env.lib.mrca_hybrid_plan_goal(env._h, None, None, None, C.c_void_p(mode.data_ptr()), C.c_void_p(scale.data_ptr()),
                                       C.c_void_p(pid.data_ptr()), C.c_void_p(clear.data_ptr()), None, env._stream())
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(sibling, (mode, scale, pid, clear))
    arena = env.arena.clone()
    got = call(goal=local)
    torch.cuda.synchronize()
    wmode, wscale, wpid, wclear = safe_ref.plan(p, sp, local.cpu().numpy(), rows)
    assert np.array_equal(got[0].cpu().numpy(), wmode) and np.array_equal(bits(got[1].cpu().numpy()), bits(wscale))
    assert np.array_equal(bits(got[2].cpu().numpy()), bits(wpid)) and np.array_equal(bits(got[3].cpu().numpy()), bits(wclear))
    assert torch.equal(arena, env.arena)


# ------------------------------------------------------------------------------------------------ the closed loop
def two_rooms():
    """the doorway scenario as two worlds of one robot, the first in the left room and the second in the right one, each with its
    goal in the other room -> (scenario, poses, goals)"""
    table = S.doorway(num_worlds=1, robots=2)
    return (S.doorway(num_worlds=2, robots=1), np.ascontiguousarray(table.init_table, f32), np.ascontiguousarray(table.goal_table, f32))


@pytest.mark.parametrize("kind", ["stand_in", "dwa", "hybrid"])
def test_doorway_closed_loop_equals_the_cpu_closed_loop(hip, kind):
    """A robot in each room, steered at mrca_subgoals_los' local subgoals (reach 60) by the stand-in, by mrca_dwa_actions_goal
    and by mrca_hybrid_actions_goal around the stand-in: both reach their goals, and the final poses are the bits of the same loop
    in the C oracle with the restatements.  (The stand-in, which is not under test, runs on the host in both loops.)"""
    from mrca.planner import PlannerParams
    from test_planner_los_host import DOORWAY_PLAN, DOORWAY_REACH, DoorwayPlan, closed_loop, cpu_controller, stand_in
    sc, poses, goals = two_rooms()
    ora = U.COracleEnv(sc)
    ora.reset(None, poses, goals)
    plan = DoorwayPlan(sc, goals=goals, slot=[0, 1])
    want, ticks = closed_loop(ora, cpu_controller(kind), plan.los)
    assert (want == 1).all(), (kind, want, ticks)

    env = hip.VecStageWorld(sc)
    env.reset(None, dev(poses), dev(goals))
    fields = env.plan_goals(params=PlannerParams.for_grid(sc.grid, **DOORWAY_PLAN))
    torch.cuda.synchronize()
    assert np.array_equal(fields.field.cpu().numpy().view(np.uint32)[fields.slot.cpu().numpy()], plan.fields[plan.slot])
    out = sentinels(env)
    los = los_params(DOORWAY_REACH)
    for k in range(ticks):
        local = env.subgoals_los(fields, los, out=out)[0]
        policy = lambda: dev(stand_in(env.obs.cpu().numpy(), local.cpu().numpy(), env.speed.cpu().numpy()))
        if kind == "stand_in":
            a = policy()
        elif kind == "dwa":
            a = env.dwa_actions(goal=local)
        else:
            a = env.hybrid_actions(policy(), goal=local)
        a = a.clone()
        a[:, 0] = torch.where(env.done.bool(), torch.zeros_like(a[:, 0]), a[:, 0])
        env.step(a.contiguous())
    torch.cuda.synchronize()
    first = env.first_result.cpu().numpy()
    assert (first == 1).all(), (kind, first)
    assert np.array_equal(bits(env.pose.cpu().numpy()), bits(ora.pose)), (kind, env.pose.cpu().numpy(), ora.pose)
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ the evaluator
def test_cli_planner_los(hip):
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), os.environ.get("PYTHONPATH", "")]))

    def evaluate(args):
        return subprocess.run([sys.executable, "-m", "mrca.evaluate", "--scenario", "doorway", "--circles", "2", "--robots", "1",
                               "--max-ticks", "900"] + args, env=env, capture_output=True, text=True, timeout=300)
    run = evaluate(["--planner-los"])
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout)
    assert out["scenario"] == "doorway" and out["robots"] == 2 and out["success_rate"] == 1.0
    assert out["los_params"] == {"reach": 60} and out["planner_params"]["lookahead"] == 15
    m, m_vis = out["planner_mean_ahead"]
    assert 15 <= m <= 60 and 1 <= m_vis <= m
    run = evaluate(["--planner-los", "--los-param", "reach=40", "--planner-param", "lookahead=10", "--dwa"])
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout)
    assert out["los_params"] == {"reach": 40} and out["planner_params"]["lookahead"] == 10 and "dwa_params" in out
    run = evaluate(["--planner-los", "--hybrid"])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "hybrid_modes" in json.loads(run.stdout) and "los_params" in json.loads(run.stdout)
    run = evaluate(["--planner-los", "--orca"])
    assert run.returncode == 2 and "--planner-los" in run.stderr
    run = evaluate(["--planner-los", "--dwa", "--planner-param", "lookahead=5"])
    assert run.returncode == 2 and "0.5 m" in run.stderr
    run = evaluate(["--planner", "--dwa"])
    assert run.returncode == 2 and "--planner" in run.stderr
