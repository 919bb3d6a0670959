"""GPU: mrca_dwa_actions -- ``actions``, ``choice`` and ``score`` EQUAL, bit for bit, to the NumPy float32 restatement of
tests/dwa_ref.py fed with host copies of the env's fields, for EVERY robot (small walled worlds right after a teleport and
after motion, every candidate-grid size that takes another path through the kernel, the shortest and the longest rollout, ring
heads that differ, a mask, worlds of more than 64 robots); the call reads the env and writes nothing of it; 30 closed-loop
ticks equal to the C oracle driven by the host build of the same rule; the error returns; ``mrca.evaluate --dwa``.

The crafted cases -- every branch, tie and threshold of the rule, and the inputs at which the kernel's own glue can go wrong
(the packing of points into groups of four, the deal of candidates to lanes and rounds, the wave maximum, the early exits) --
live in tests/dwa_cases.py, shared with tests/test_dwa_host.py; tests/controller_inject.py writes them into an env, one case
per robot, and ``test_crafted_cases_on_the_device`` asserts from the fields read back that each case stood on its edge."""
import ctypes as C

import numpy as np
import pytest
import torch

import controller_inject as J
import dwa_cases as K
import dwa_ref as R
import util as U
from dwa_cases import CRAFTED_AT, QUAD_AT, SECTORS_AT, SPECIAL_AT, WINNERS_AT
from test_dwa_host import host_env_actions, shim  # noqa: F401  (shim: the host build of csrc/mrca_dwa_device.h)
from test_gpu_orca import NAN_BITS, _evaluate, go_to_goal, nan_filled, small_scenario, teleport_poses
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32


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


def dwa_params(p):
    from mrca.dwa import DwaParams
    return DwaParams(**{k: (int(v) if k in R.INTS else float(v)) for k, v in p.items()})


def host_fields(env):
    """Host copies of what the call reads: (local_goal, speed, newest scan rows)."""
    torch.cuda.synchronize()
    rows = env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()]
    return env.local_goal.cpu().numpy(), env.speed.cpu().numpy(), rows.cpu().numpy()


def check_equal(env, p, mask=None, with_extras=True, fields=None, goal_dev=None, full=False):
    """One call compared with dwa_ref on the same fields, every robot -> (the reference's choice, its diagnostics), or with
    ``full`` (its actions, choice, score, diagnostics).  ``goal_dev``: a float32[N,2] tensor that goes in through
    mrca_dwa_actions_goal; the reference is then fed with a host copy of it in place of ``local_goal``."""
    goal, speed, rows = fields or host_fields(env)
    if goal_dev is not None:
        goal = goal_dev.cpu().numpy()
    act = nan_filled(env)
    choice = torch.full((env.N,), 12345, dtype=torch.int32, device=env.device) if with_extras else None
    score = nan_filled(env)[:, 0].contiguous() if with_extras else None
    m = None if mask is None else dev(np.ascontiguousarray(mask, np.uint8))
    got = env.dwa_actions(dwa_params(p), mask=m, out=act, choice=choice, score=score, goal=goal_dev)
    assert got is act
    robots = None if mask is None else np.flatnonzero(mask).tolist()
    wact, wchoice, wscore, diag = R.env_actions(p, goal, speed, rows, robots=robots)
    torch.cuda.synchronize()
    a = act.cpu().numpy().view(np.uint32)
    want_a = np.where(np.isnan(wact), np.uint32(NAN_BITS), wact.view(np.uint32))
    assert np.array_equal(a, want_a), (np.argwhere(a != want_a)[:5], act.cpu().numpy()[:8], wact[:8])
    if with_extras:
        skipped = np.isnan(wscore)
        assert np.array_equal(choice.cpu().numpy(), np.where(skipped, 12345, wchoice)), (choice.cpu().numpy(), wchoice)
        s = score.cpu().numpy().view(np.uint32)
        assert np.array_equal(s, np.where(skipped, np.uint32(NAN_BITS), wscore.view(np.uint32))), np.argwhere(s != wscore.view(np.uint32))[:5]
    return (wact, wchoice, wscore, diag) if full else (wchoice, diag)


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3), (1024, 2)])
def test_small_worlds_equal_the_reference(hip, beams, frames, lazy):
    """3 worlds x 7 robots = 21 robots: the last workgroup (4 robots each) has three empty waves."""
    sc = small_scenario(beams, frames)
    env = hip.VecStageWorld(sc, lazy_obs=lazy)
    rng = np.random.default_rng(2)
    poses, goals = teleport_poses(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    # right after the teleport: two robots on one spot (range 0: everything blocked), one 0.6 m from a wall and facing it
    choice, diag = check_equal(env, R.params())
    assert (choice == R.BLOCKED).any() and (choice >= 0).any()
    check_equal(env, R.params(obst_dist=6.0, acc_v=1.0, acc_w=3.0, clear_cap=0.5, w_heading=0.4))
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    choice, diag = check_equal(env, R.params())
    assert (diag["beam"] >= 0).any() and (choice >= 0).any()
    check_equal(env, R.params(obst_dist=6.0, acc_v=1.0, acc_w=3.0, clear_cap=0.5, w_heading=0.4))     # (now the window is a part)
    env.close()


@pytest.fixture(scope="module")
def moved_env(hip):
    """The small scenario after a teleport and 10 random ticks, and host copies of its fields: shared by the shape tests."""
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(3)
    poses, goals = teleport_poses(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    yield env, host_fields(env)
    env.close()


@pytest.mark.parametrize("nv,nw", [(1, 1), (1, 64), (16, 4), (5, 21), (16, 64)])
def test_candidate_grids(moved_env, nv, nw):
    """nv * nw = 1 (one lane works), 64 (exactly one round), 105 (a second round with a tail of 41), 1024 (16 full rounds)."""
    env, fields = moved_env
    choice, _d = check_equal(env, R.params(nv=nv, nw=nw), fields=fields)
    assert (choice >= 0).any()


@pytest.mark.parametrize("steps", [1, 64])
def test_shortest_and_longest_rollout(moved_env, steps):
    env, fields = moved_env
    check_equal(env, R.params(steps=steps), fields=fields)
    check_equal(env, R.params(steps=steps, horizon=0.5, nv=3, nw=7), fields=fields)


def test_ring_heads_that_differ_between_robots(hip):
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(6)
    env.reset()
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    mask = (np.arange(env.N) % 4 == 1).astype(np.uint8)
    env.reset(dev(mask))                                 # a masked reset: these robots start a new history
    env.step(dev(U.random_actions(rng, env.N)), worlds=(0, 1))            # ... and world 0 ticks alone, once more
    torch.cuda.synchronize()
    assert len(set(env.ring_head.cpu().numpy().tolist())) > 1
    check_equal(env, R.params(obst_dist=6.0))
    env.close()


# ------------------------------------------------------------------------------------------------ the crafted cases, on the device
# tests/dwa_cases.py, one case per robot (``K.layout``), written by tests/controller_inject.py
def crafted_env(hip, beams):
    """A walled env with ring heads that differ and every case of dwa_cases written into it -> (env, names of ``crafted``)"""
    env = J.walled_env(hip, beams, K.N_CASES)
    names, goal, speed, rows = K.layout(beams)
    J.write_cases(env, 0, local_goal=goal, speed=speed, rows=rows)
    assert J.heads_differ(env)
    return env, names


def crafted_checks(env, names, beams, goal_dev=None):
    """Every check of the crafted cases on one env, the goals read from ``local_goal`` or from ``goal_dev``"""
    p = R.params()
    act, choice, score, d = check_equal(env, p, goal_dev=goal_dev, full=True)
    K.expectations(names, p, beams, act, choice, score, d)                # (each edge occurred: from the fields read back)
    K.sector_expectations(d, SECTORS_AT)
    K.special_expectations(p, act, choice, d, SPECIAL_AT)
    # the same robots under another window and another horizon: the packed points are walked by other arcs
    check_equal(env, R.params(acc_v=1.0, acc_w=3.0, obst_dist=6.0, clear_cap=0.5, w_heading=0.4), goal_dev=goal_dev)
    # ties: two mirror arcs, every candidate of the default grid (across lanes and into the partial round), all 1024 (16 rounds)
    for name, grid in K.TIE_GRIDS.items():
        act, choice, _s, d = check_equal(env, R.params(**grid), goal_dev=goal_dev, full=True)
        K.tie_expectations(name, act, choice, d, CRAFTED_AT + K.TIE_ROW)
    # the winner in lane 0, in lane 63, in the first round, in the last partial round
    kinds, done = set(), {}
    for k, (grid, _g) in enumerate(K.WINNER_SETS):
        q = R.params(**grid)
        key = tuple(sorted(grid.items()))
        if key not in done:
            done[key] = check_equal(env, q, goal_dev=goal_dev)[0]
        kinds |= K.winner_kinds(q, int(done[key][WINNERS_AT + k]))
    assert kinds == K.WINNER_KINDS, kinds
    # one workgroup whose four robots are masked out, at the goal, blocked and choosing
    mask = np.ones(env.N, np.uint8)
    mask[QUAD_AT] = 0
    choice, _d = check_equal(env, p, mask=mask, goal_dev=goal_dev)
    assert choice[QUAD_AT + 1] == R.AT_GOAL and choice[QUAD_AT + 2] == R.BLOCKED and choice[QUAD_AT + 3] >= 0


@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_crafted_cases_on_the_device(hip, beams):
    """Every row of ``dwa_cases.crafted``, rows with 0, 1, 3, 4, 5, 63 and 64 occupied sectors, NaN and Inf in goal and speed, the
    grids on which ties decide and the four places a winner can take, written into an env -- and once more with the goals
    handed to mrca_dwa_actions_goal while ``local_goal`` holds something else."""
    env, names = crafted_env(hip, beams)
    crafted_checks(env, names, beams)
    goals = env.local_goal.clone()
    env.local_goal[:] = dev(np.random.default_rng(beams).uniform(-5.0, 5.0, (env.N, 2)).astype(f32))
    crafted_checks(env, names, beams, goal_dev=goals)
    env.check()
    env.close()


def test_mask_keeps_the_other_rows_and_the_extras_are_optional(moved_env):
    env, fields = moved_env
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    check_equal(env, R.params(), mask=mask, fields=fields)               # (rows with mask 0 keep their patterns exactly)
    check_equal(env, R.params(), mask=mask, with_extras=False, fields=fields)
    check_equal(env, R.params(), with_extras=False, fields=fields)
    check_equal(env, R.params(), mask=np.zeros(env.N, np.uint8), fields=fields)


def test_worlds_of_more_than_64_robots(hip):
    env = hip.VecStageWorld(S.circle_big(66))
    env.reset()
    check_equal(env, R.params())
    env.check()
    env.close()
    env = hip.VecStageWorld(S.circle_big(500))
    env.reset()
    for _ in range(10):
        torch.cuda.synchronize()
        env.step(dev(go_to_goal(env.local_goal.cpu().numpy())))
    choice, diag = check_equal(env, R.params())
    assert (diag["beam"] >= 0).any() and (choice >= 0).all()             # neighbours are seen, and nobody is boxed in yet
    env.check()
    env.close()


def test_the_call_writes_nothing_of_the_env(hip):
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc, lazy_obs=False)
    rng = np.random.default_rng(8)
    env.reset()
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    names = U.STATE_FIELDS + ["scan_ring", "ring_head", "hit_bits", "fresh"]
    before = {k: getattr(env, k).clone() for k in names}
    arena = env.arena.clone()
    env.dwa_actions(choice=torch.zeros(env.N, dtype=torch.int32, device=env.device), score=torch.zeros(env.N, device=env.device))
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k], getattr(env, k)), k
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory
    env.close()


def test_thirty_closed_loop_ticks_equal_the_oracle(hip, shim):  # noqa: F811
    """mrca_step on the same stream right behind the call, nothing synchronised in between."""
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    ora = U.COracleEnv(sc)
    poses, goals = teleport_poses(sc, np.random.default_rng(2))
    env.reset(None, dev(poses), dev(goals))
    ora.reset(None, poses, goals)
    p = R.params()
    for k in range(30):
        a = env.dwa_actions(dwa_params(p))
        env.step(a)
        act, _c, _s, _d = host_env_actions(shim, p, ora.local_goal, ora.speed, ora.scan)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), act.view(np.uint32)), k
        ora.step(act)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
        U.assert_hits_equal(env, ora, what=f"tick {k}")
    env.close()


def test_errors(hip):
    from mrca import _lib
    env = hip.VecStageWorld(small_scenario(64, 1))
    env.reset()
    out = torch.zeros(env.N, 2, device=env.device)
    choice = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    bad = [("radius", 0.0), ("horizon", -1.0), ("clear_cap", 0.0), ("max_speed", 0.0), ("max_speed", 1.5), ("max_omega", 0.0),
           ("max_omega", 2.0), ("obst_dist", -0.1), ("obst_dist", 6.5), ("acc_v", -1.0), ("acc_w", -1.0), ("w_goal", -1.0),
           ("w_heading", -1.0), ("w_clear", -1.0), ("w_speed", -1.0), ("steps", 0), ("steps", 65), ("nv", 0), ("nv", 17), ("nw", 0),
           ("nw", 65)]
    bad += [(k, v) for k in R.FIELDS if k not in R.INTS for v in (float("nan"), float("inf"))]
    for k, v in bad:
        st = _lib.DwaParamsStruct()
        env.lib.mrca_dwa_default_params(C.byref(st))
        setattr(st, k, v)
        rc = env.lib.mrca_dwa_actions(env._h, C.byref(st), None, out.data_ptr(), choice.data_ptr(), None, env._stream())
        assert rc == -1 and k.encode() in env.lib.mrca_last_error(), (k, v, env.lib.mrca_last_error())
    assert env.lib.mrca_dwa_actions(env._h, None, None, None, None, None, env._stream()) == -1
    assert env.lib.mrca_dwa_actions(env._h, None, None, out.data_ptr() + 4, None, None, env._stream()) == -1
    from mrca.dwa import DwaParams
    with pytest.raises(RuntimeError):
        env.dwa_actions(DwaParams(nv=17), out=out)
    with pytest.raises(ValueError):
        env.dwa_actions(out=out, choice=torch.zeros(env.N, device=env.device))       # choice must be int32
    env.check()                                          # no HIP error was left behind
    assert not out.any() and not choice.any()
    env.close()


def test_cli_dwa(hip):
    out = _evaluate(["--dwa", "--circles", "2", "--robots", "10", "--max-ticks", "200", "--dwa-param", "nw=15"])
    assert {"success_rate", "crash_rate", "extra_time_s", "extra_distance_m", "average_speed_mps", "robots"} <= set(out)
    assert out["robots"] == 20 and out["dwa_params"]["nw"] == 15 and "DWA" in out["policy"]


def test_cli_dwa_first_reports_both_groups(hip):
    out = _evaluate(["--circles", "2", "--robots", "10", "--dwa-first", "4", "--orca", "--max-ticks", "50"])
    assert set(out["groups"]) == {"dwa", "orca"}
    assert out["groups"]["dwa"]["robots"] == 8 and out["groups"]["orca"]["robots"] == 12
    assert {"success_rate", "crash_rate", "extra_time_s"} <= set(out["groups"]["dwa"])
    out = _evaluate(["--one-circle", "70", "--dwa-first", "35", "--max-ticks", "30"])
    assert out["groups"]["dwa"]["robots"] == 35 and out["groups"]["policy"]["robots"] == 35
