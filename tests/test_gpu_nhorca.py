"""GPU: mrca_nhorca_actions -- ``actions``, ``vel`` and ``mode`` EQUAL, bit for bit, to the NumPy float32 restatement of
tests/nhorca_ref.py fed with host copies of the env's fields: small walled worlds with robots on one spot, a full wave of
neighbours, a dense circle where LP3 decides, robots turned away from and standing at their goals, ring heads that differ, a
mask; worlds of more than 64 robots (the threshold, a lattice with several chunks of candidates, two worlds in one hash); closed
loops equal to the C oracle driven by the host build of the same rule; the call writes nothing of the env; the refusals with
their messages; ``mrca.evaluate --nh-orca``.

The crafted cases live in tests/orca_cases.py, shared with tests/test_orca_host.py and tests/test_nhorca_host.py;
tests/controller_inject.py puts them into an env as ONE world, and ``test_crafted_world_on_the_device`` asserts from the fields
read back that each edge occurred and each situation took its mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import controller_inject as J
import nhorca_ref as NR
import orca_cases as K
import orca_ref as R
import util as U
from test_gpu_orca import NAN_BITS, _evaluate, go_to_goal, host_fields, nan_filled, small_scenario, teleport_poses
from test_nhorca_host import host_env_actions, nhshim  # noqa: F401  (nhshim: the host build of csrc/mrca_nhorca_device.h)
from test_orca_big_host import lattice_poses, rule_robots
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_FILL = -7


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


def nh_params(p):
    from mrca.nhorca import NhOrcaParams
    return NhOrcaParams(**{k: (int(v) if k == "max_neighbors" else float(v)) for k, v in p.items()})


def check_equal(env, p, robots=None, mask=None, with_vel=True, with_mode=True):
    """One call compared with nhorca_ref on the env's fields as they stand.  ``robots``: the rows the reference is computed for
    (default: all, or the mask's); every other row the call wrote must be a command; rows the mask excludes keep the prefill.
    -> (the reference's modes, its diagnostics)"""
    pose, speed_gt, goal, rows, hit = host_fields(env)
    act, vel = nan_filled(env), (nan_filled(env) if with_vel else None)
    mode = torch.full((env.N,), MODE_FILL, dtype=torch.int32, device=env.device) if with_mode else None
    m = None if mask is None else dev(np.asarray(mask, np.uint8))
    got = env.nhorca_actions(nh_params(p), mask=m, out=act, vel=vel, mode=mode)
    assert got is act
    written = np.ones(env.N, bool) if mask is None else np.asarray(mask, bool)
    if robots is None:
        robots = np.flatnonzero(written).tolist()
    assert written[robots].all()
    wact, wvel, wmode, diags = NR.env_actions(p, env.R, env.scenario.seed, pose, speed_gt, goal, rows, hit, robots=robots)
    torch.cuda.synchronize()
    ref = np.zeros(env.N, bool)
    ref[robots] = True
    a = act.cpu().numpy()
    assert np.array_equal(a[ref].view(np.uint32), wact[ref].view(np.uint32)), (np.flatnonzero((a != wact).any(1) & ref)[:8],
                                                                               a[ref][:4], wact[ref][:4])
    other = written & ~ref
    assert np.isfinite(a[other]).all() and (a[other, 0] >= 0).all() and (a[other, 0] <= p["max_speed"]).all()
    assert (np.abs(a[other, 1]) <= 1).all()
    assert (a[~written].view(np.uint32) == NAN_BITS).all()
    if with_vel:
        v = vel.cpu().numpy()
        assert np.array_equal(v[ref].view(np.uint32), wvel[ref].view(np.uint32)), np.flatnonzero((v != wvel).any(1) & ref)[:8]
        assert np.isfinite(v[other]).all() and (v[~written].view(np.uint32) == NAN_BITS).all()
    if with_mode:
        md = mode.cpu().numpy()
        assert np.array_equal(md[ref], wmode[ref]), np.flatnonzero((md != wmode) & ref)[:8]
        assert ((md[other] >= 0) & (md[other] <= 3)).all() and (md[~written] == MODE_FILL).all()
    return wmode, diags


# ------------------------------------------------------------------------------------------------ worlds of up to 64 robots
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3)])
def test_small_worlds_equal_the_reference(hip, beams, frames, lazy):
    sc = small_scenario(beams, frames)
    env = hip.VecStageWorld(sc, lazy_obs=lazy)
    rng = np.random.default_rng(2)
    poses, goals = teleport_poses(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    seen = set()
    for p in (NR.params(), NR.params(jitter=0.0, obst_dist=6.0, max_neighbors=3, track_error=0.2, track_time=1.0)):
        for d in check_equal(env, p)[1].values():       # right after the teleport: two robots on one spot, one at the wall
            seen |= set(d["branches"])
    assert R.OVERLAP in seen
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    _m, diags = check_equal(env, NR.params())
    assert any(d["n_static"] > 0 for d in diags.values())
    check_equal(env, NR.params(jitter=0.1, obst_dist=6.0, neighbor_dist=20.0, responsibility=1.0, time_horizon_obst=3.0, track_error=0.5,
                               track_time=1.5))
    env.check()
    env.close()


@pytest.mark.parametrize("max_neighbors", [10, 46])
def test_a_full_wave_of_neighbours(hip, max_neighbors):
    env = hip.VecStageWorld(S.circle_n(64, 6.0))
    env.reset()
    _m, diags = check_equal(env, NR.params(max_neighbors=max_neighbors, neighbor_dist=20.0))
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) == max_neighbors
    env.check()
    env.close()


@pytest.mark.parametrize("robots,beams", [(34, 64), (34, 192), (66, 192)])
def test_crafted_world_on_the_device(hip, robots, beams):
    """``orca_cases.device_world`` written into an open env whose ring heads differ (tests/controller_inject.py), up to 64
    robots and through the lidar hash: the ties, touching discs (at twice the GROWN radius) and thresholds of the ORCA test, and
    the situations of the host test's crafted solves -- free, at its goal, facing away, goal to the left / right, a wall
    ahead, and the four pushed robots -- with the modes they are made for; all four modes occur.  Asserted from the fields read back."""
    env = J.open_env(hip, robots, beams)
    J.write_world(env, K.device_world(env.R, beams))
    pose, speed_gt, goal, rows, hit = host_fields(env)
    seen = set()
    for p in K.nh_device_params():
        modes, diags = check_equal(env, p)
        grown = dict(p, radius=NR.derive(p)[3])
        for w in range(env.W):
            K.device_expectations(grown, w * env.R, beams, pose, speed_gt, goal, rows, hit, {n: d["free"] for n, d in diags.items()},
                                  robots=env.R)
            if p["jitter"] == 0.0:
                K.nh_device_expectations(p, w * env.R, modes, diags)
        seen |= set(modes.tolist())
    assert seen == {NR.TRACK, NR.TURN, NR.STILL, NR.EVADE}, seen
    check_equal(env, K.nh_device_params()[1], mask=(np.arange(env.N) % 3 != 1).astype(np.uint8))
    env.check()
    env.close()


def test_a_robot_alone_in_its_world(hip):
    env = hip.VecStageWorld(S.circle_n(1, 6.0, num_worlds=2))
    env.reset()
    modes, diags = check_equal(env, NR.params(jitter=0.0))
    assert all(len(d["branches"]) == d["n_static"] for d in diags.values())
    assert (modes == NR.TRACK).all()                    # it faces its goal across the circle
    env.close()


def test_dense_circle_where_lp3_decides(hip):
    env = hip.VecStageWorld(S.circle_n(12, 1.5))
    env.reset()
    # twelve robots 0.78 m apart, less than twice the grown radius: on the CPU (C oracle, nhorca_ref) LP3 changes the tracked
    # solve's result for 9 robots at tick 0 and for 11 at tick 5, the free solve's for all 12 at tick 5
    for ticks in (0, 5):
        for _ in range(ticks):
            torch.cuda.synchronize()
            env.step(dev(go_to_goal(env.local_goal.cpu().numpy())))
        _m, diags = check_equal(env, NR.params())
        assert sum(d["lp3_changed"] for d in diags.values()) >= 1
    assert sum(d["free"]["lp3_changed"] for d in diags.values()) >= 1
    check_equal(env, NR.params(max_neighbors=46, track_error=0.1, track_time=0.5))
    env.close()


def test_robots_turned_away_from_their_goals_and_robots_at_their_goals(hip):
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(12)
    poses, goals = teleport_poses(sc, rng)
    for n in range(0, len(poses), 3):                   # every third robot stands at its goal, the next one has it behind its back
        goals[n] = poses[n, :2] + f32(0.1)
        th = float(poses[n + 1, 2]) + np.pi
        goals[n + 1] = poses[n + 1, :2] + f32(3.0) * np.array([np.cos(th), np.sin(th)], f32)
    env.reset(None, dev(poses), dev(goals))
    modes, diags = check_equal(env, NR.params(jitter=0.0))
    assert {NR.TURN, NR.STILL} <= set(modes.tolist())
    assert all(diags[n]["o"] == (0.0, 0.0) for n in range(0, len(poses), 3))
    check_equal(env, NR.params())
    env.close()


def test_ring_heads_that_differ_after_a_masked_reset(hip):
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(6)
    env.reset()
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    env.step(dev(U.random_actions(rng, env.N)), worlds=(0, 1))       # world 0 alone, once more
    env.reset(dev((np.arange(env.N) % 4 == 1).astype(np.uint8)))     # and every fourth robot starts a new episode
    torch.cuda.synchronize()
    assert len(set(env.ring_head.cpu().numpy().tolist())) > 1
    check_equal(env, NR.params(obst_dist=6.0))
    env.close()


def test_mask_keeps_the_other_rows_and_the_outputs_are_optional(hip):
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    env.reset()
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    check_equal(env, NR.params(), mask=mask)             # (rows with mask 0 keep the sentinels exactly)
    check_equal(env, NR.params(), mask=mask, with_vel=False)
    check_equal(env, NR.params(), with_vel=False, with_mode=False)
    check_equal(env, NR.params(), with_mode=False)
    check_equal(env, NR.params(), mask=np.zeros(env.N, np.uint8))
    env.close()


# ------------------------------------------------------------------------------------------------ worlds of more than 64 robots
@pytest.mark.parametrize("robots", [65, 66])
def test_the_threshold(hip, robots):
    env = hip.VecStageWorld(S.circle_big(robots))
    rng = np.random.default_rng(robots)
    env.reset()
    check_equal(env, NR.params())
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    for p in (NR.params(), NR.params(jitter=0.0, max_neighbors=3, track_error=0.2, track_time=1.0)):
        _m, diags = check_equal(env, p)
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) >= 2      # (3.14 m apart: the neighbours on the circle)
    env.check()
    env.close()


@pytest.mark.parametrize("neighbor_dist", [6.0, 12.8])
def test_a_lattice_with_many_chunks_of_candidates(hip, neighbor_dist):
    env = hip.VecStageWorld(S.circle_big(300))           # (test_orca_big_host's lattice: 0.7 m apart, cells of more than 64 robots)
    poses, goals = lattice_poses()
    env.reset(None, dev(poses), dev(goals))
    _m, diags = check_equal(env, NR.params(max_neighbors=46, neighbor_dist=neighbor_dist), robots=rule_robots())
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) == 46
    env.check()
    env.close()


def test_two_big_worlds_laid_over_each_other(hip):
    two = hip.VecStageWorld(S.circle_big(100, num_worlds=2, spacing=0.9))
    one = hip.VecStageWorld(S.circle_big(100, spacing=0.9))
    rng = np.random.default_rng(21)
    two.reset()
    one.reset()
    for _ in range(5):
        a = U.random_actions(rng, 100)
        two.step(dev(np.concatenate([a, a])))
        one.step(dev(a))
    p = NR.params(jitter=0.0)                            # (the jitter angle is drawn per robot of the ENV: world 1 would differ)
    a2, a1 = two.nhorca_actions(nh_params(p)), one.nhorca_actions(nh_params(p))
    torch.cuda.synchronize()
    assert torch.equal(a2[:100].view(torch.int32), a1.view(torch.int32))
    assert torch.equal(a2[100:].view(torch.int32), a1.view(torch.int32))
    check_equal(two, NR.params(), robots=list(range(0, 200, 7)))
    two.check()
    two.close()
    one.close()


# ------------------------------------------------------------------------------------------------ closed loop, and what is not written
@pytest.mark.parametrize("big", [False, True])
def test_thirty_closed_loop_ticks_equal_the_oracle(hip, nhshim, big):  # noqa: F811
    if big:
        sc = S.circle_big(66, spacing=0.9)
        sc.beams, sc.frames = 64, 1
        poses = goals = None
    else:
        sc = small_scenario(64, 1)
        poses, goals = teleport_poses(sc, np.random.default_rng(2))
    env = hip.VecStageWorld(sc)
    ora = U.COracleEnv(sc)
    env.reset(None, None if poses is None else dev(poses), None if goals is None else dev(goals))
    ora.reset(None, poses, goals)
    p = NR.params(jitter=0.2)
    for k in range(30):
        a = env.nhorca_actions(nh_params(p))
        act, _v, _m, _s1, _l, _c = host_env_actions(nhshim, p, sc.robots_per_world, sc.seed, ora.pose, ora.speed_gt, ora.goal, ora.scan,
                                                    ora.hit_robot)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), act.view(np.uint32)), k
        env.step(a)
        ora.step(act)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
        U.assert_hits_equal(env, ora, what=f"tick {k}")
    assert (ora.speed_gt[:, 0] > 0).any()
    env.close()


@pytest.mark.parametrize("big", [False, True])
def test_the_call_writes_nothing_of_the_env(hip, big):
    from mrca import _lib
    sc = S.circle_big(100, spacing=0.9) if big else small_scenario(512, 3)
    env = hip.VecStageWorld(sc, lazy_obs=False)
    rng = np.random.default_rng(8)
    env.reset()
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    names = ["_" + n if n in ("obs", "scan") else n for n, _dt, _shape in _lib.FIELDS]       # every MRCA_F_*
    before = {k: getattr(env, k).clone() for k in names}
    arena = env.arena.clone()
    env.nhorca_actions(vel=torch.zeros(env.N, 2, device=env.device), mode=torch.zeros(env.N, dtype=torch.int32, device=env.device))
    env.nhorca_actions(nh_params(NR.params(neighbor_dist=19.3, max_neighbors=46)))
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k], getattr(env, k)), k
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory, the broad phase's scratch included
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ the refusals
def test_refusals(hip):
    from mrca import _lib
    small = hip.VecStageWorld(small_scenario(64, 1))
    big = hip.VecStageWorld(S.circle_big(66))
    small.reset()
    big.reset()
    bad = [("max_neighbors", 47, -1, "max_neighbors 47 outside 1..46"), ("max_neighbors", 0, -1, "max_neighbors 0 outside 1..46"),
           ("track_time", 0.05, -1, "track_time outside [0.1, 1.5]"), ("track_time", 1.6, -1, "track_time outside [0.1, 1.5]"),
           ("track_error", 0.0, -1, "track_error outside (0, 0.5]"), ("track_error", float("nan"), -1, "track_error is not finite"),
           ("radius", 0.0, -1, "radius must be > 0"), ("jitter", float("inf"), -1, "jitter is not finite")]
    for env in (small, big):
        call = env.lib.mrca_nhorca_actions
        out = torch.zeros(env.N, 2, device=env.device)
        for k, v, want_rc, msg in bad:
            st = _lib.NhOrcaParamsStruct()
            env.lib.mrca_nhorca_default_params(C.byref(st))
            setattr(st, k, v)
            rc = call(env._h, C.byref(st), None, out.data_ptr(), None, None, env._stream())
            assert rc == want_rc and env.lib.mrca_last_error().decode() == "mrca_nhorca_actions: " + msg, (k, v, env.lib.mrca_last_error())
        assert call(env._h, None, None, None, None, None, env._stream()) == -1 and b"actions_dev is NULL" in env.lib.mrca_last_error()
        assert call(env._h, None, None, out.data_ptr() + 4, None, None, env._stream()) == -1
        assert call(env._h, None, None, out.data_ptr(), None, out.data_ptr() + 2, env._stream()) == -1
        assert b"mode_dev must be 4-byte aligned" in env.lib.mrca_last_error()
        assert call(None, None, None, out.data_ptr(), None, None, env._stream()) == -1 and b"env is NULL" in env.lib.mrca_last_error()
        st = _lib.NhOrcaParamsStruct()
        env.lib.mrca_nhorca_default_params(C.byref(st))
        st.neighbor_dist = 19.4
        rc = call(env._h, C.byref(st), None, out.data_ptr(), None, None, env._stream())
        if env is big:
            assert rc == -4
            assert env.lib.mrca_last_error().decode() == "mrca_nhorca_actions: neighbor_dist 19.4 > 19.3 with robots_per_world 66 > 64 " \
                                                         "(the search looks at three rings of 6.5 m cells at most)"
            assert not out.any()
        else:
            assert rc == 0                               # worlds of up to 64 robots: any neighbor_dist
            out.zero_()
        env.check()                                      # no HIP error was left behind
        assert not out.any()
    # between the move phase and the observe phase the hash describes the poses BEFORE the move
    out = torch.zeros(big.N, 2, device=big.device)
    act = dev(U.random_actions(np.random.default_rng(26), big.N))
    big.move(act, (0, 1))
    rc = big.lib.mrca_nhorca_actions(big._h, None, None, out.data_ptr(), None, None, big._stream())
    assert rc == -1
    assert big.lib.mrca_last_error().decode() == "mrca_nhorca_actions: the lidar hash does not describe the current poses -- call " \
                                                 "mrca_observe_worlds (after mrca_move_worlds) or mrca_reset first (robots_per_world 66 > 64)"
    big.check()
    assert not out.any()
    big.observe((0, 1))
    check_equal(big, NR.params())
    for e in (small, big):
        e.check()
        e.close()


# ------------------------------------------------------------------------------------------------ the evaluator
FIELDS = {"success_rate", "crash_rate", "extra_time_s", "extra_distance_m", "average_speed_mps", "robots"}


def test_cli_nh_orca(hip):
    out = _evaluate(["--circles", "2", "--robots", "6", "--radius", "3", "--nh-orca", "--max-ticks", "50", "--nh-orca-param", "track_error=0.1"])
    assert FIELDS <= set(out) and out["robots"] == 12 and "NH-ORCA" in out["policy"]
    assert abs(out["nhorca_params"]["track_error"] - 0.1) < 1e-6 and out["nhorca_params"]["max_neighbors"] == 10
    assert set(out["nhorca_modes"]) == {"track", "turn", "still", "evade"}
    assert abs(sum(out["nhorca_modes"].values()) - 1.0) < 1e-9


def test_cli_nh_orca_first_reports_both_groups(hip):
    out = _evaluate(["--circles", "2", "--robots", "6", "--radius", "3", "--nh-orca-first", "3", "--max-ticks", "50"])
    assert set(out["groups"]) == {"nhorca", "policy"}
    assert out["groups"]["nhorca"]["robots"] == 6 and out["groups"]["policy"]["robots"] == 6
    assert FIELDS - {"robots"} <= set(out["groups"]["nhorca"]) and "nhorca_params" in out
    assert abs(sum(out["nhorca_modes"].values()) - 1.0) < 1e-9
