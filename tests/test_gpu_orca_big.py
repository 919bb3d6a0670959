"""GPU: mrca_orca_actions_any -- the ORCA baseline on worlds of more than 64 robots, ``actions`` and ``vel`` EQUAL, bit for
bit, to the NumPy float32 restatement of tests/orca_ref.py fed with host copies of the env's fields: at the threshold (65 and
66 robots), on a 300-robot lattice where every robot's cells hold several chunks of candidates, after motion, with two worlds
laid over each other in one hash, lazy and eager views, a mask after a sliced tick, in closed loop; the call writes nothing of
the env; worlds of up to 64 robots get mrca_orca_actions' very bits; the error returns; ``mrca.evaluate --one-circle``.

The crafted cases (tests/orca_cases.py, written into an env by tests/controller_inject.py) run here as a world of 66 robots:
``test_crafted_world_of_66_robots``."""
import ctypes as C

import numpy as np
import pytest
import torch

import controller_inject as J
import orca_ref as R
import util as U
from test_gpu_orca import NAN_BITS, _evaluate, crafted_world_checks, go_to_goal, host_fields, nan_filled, orca_params, small_scenario
from test_orca_big_host import lattice_poses, rule_robots
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


def check_equal(env, p, robots=None, mask=None, with_vel=True):
    """One call compared with orca_ref on the env's fields as they stand.  ``robots``: the rows the reference is computed for
    (default: all, or the mask's); every other row the call wrote must be finite and inside [0, max_speed] x [-1, 1]; rows
    the mask excludes keep the prefill pattern.  -> the reference's diagnostics"""
    pose, speed_gt, goal, rows, hit = host_fields(env)
    act, vel = nan_filled(env), (nan_filled(env) if with_vel else None)
    m = None if mask is None else dev(np.asarray(mask, np.uint8))
    got = env.orca_actions(orca_params(p), mask=m, out=act, vel=vel)
    assert got is act
    written = np.ones(env.N, bool) if mask is None else np.asarray(mask, bool)
    if robots is None:
        robots = np.flatnonzero(written).tolist()
    assert written[robots].all()
    wact, wvel, diags = R.env_actions(p, env.R, env.scenario.seed, pose, speed_gt, goal, rows, hit, robots=robots)
    torch.cuda.synchronize()
    a = act.cpu().numpy()
    v = vel.cpu().numpy() if with_vel else None
    ref = np.zeros(env.N, bool)
    ref[robots] = True
    assert np.array_equal(a[ref].view(np.uint32), wact[ref].view(np.uint32)), (np.flatnonzero((a != wact).any(1) & ref)[:8],
                                                                               a[ref][:4], wact[ref][:4])
    if with_vel:
        assert np.array_equal(v[ref].view(np.uint32), wvel[ref].view(np.uint32)), np.flatnonzero((v != wvel).any(1) & ref)[:8]
    other = written & ~ref
    assert np.isfinite(a[other]).all() and (a[other, 0] >= 0).all() and (a[other, 0] <= p["max_speed"]).all()
    assert (np.abs(a[other, 1]) <= 1).all()
    if with_vel:
        assert np.isfinite(v[other]).all()
    assert (a[~written].view(np.uint32) == NAN_BITS).all()
    if with_vel:
        assert (v[~written].view(np.uint32) == NAN_BITS).all()
    return diags


# ------------------------------------------------------------------------------------------------ equality with the reference
@pytest.mark.parametrize("robots", [65, 66])
def test_the_threshold(hip, robots):
    env = hip.VecStageWorld(S.circle_big(robots))
    rng = np.random.default_rng(robots)
    env.reset()
    for p in (R.params(), R.params(jitter=0.3, max_neighbors=3)):
        check_equal(env, p)
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    for p in (R.params(), R.params(jitter=0.3, max_neighbors=3)):
        diags = check_equal(env, p)
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) >= 2      # (3.14 m apart: the neighbours on the circle)
    env.check()
    env.close()


def test_crafted_world_of_66_robots(hip):
    """``orca_cases.device_world`` (tests/test_gpu_orca.py: ``crafted_world_checks``) with 66 robots a world: the same ties,
    touching discs and thresholds with the neighbours found through the lidar hash"""
    env = J.open_env(hip, 66, 192)
    crafted_world_checks(env, 192)
    env.close()


@pytest.fixture(scope="module")
def lattice_env(hip):
    """One world of 300 robots teleported onto the host test's lattice (every robot's 3 x 3 cells hold more than 64 robots)."""
    env = hip.VecStageWorld(S.circle_big(300))
    poses, goals = lattice_poses()
    env.reset(None, dev(poses), dev(goals))
    yield env
    env.close()


@pytest.mark.parametrize("neighbor_dist", [6.0, 12.8, 19.3])
@pytest.mark.parametrize("max_neighbors", [10, 48])
def test_many_chunks_of_candidates(lattice_env, max_neighbors, neighbor_dist):
    diags = check_equal(lattice_env, R.params(max_neighbors=max_neighbors, neighbor_dist=neighbor_dist), robots=rule_robots())
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) == max_neighbors
    lattice_env.check()


def test_after_motion(hip):
    env = hip.VecStageWorld(S.circle_big(300))
    poses, goals = lattice_poses()
    env.reset(None, dev(poses), dev(goals))
    for _ in range(15):
        torch.cuda.synchronize()
        env.step(dev(go_to_goal(env.local_goal.cpu().numpy())))
    torch.cuda.synchronize()
    assert (env.speed_gt[:, 0] != 0).any()               # robots are moving (or were when they crashed)
    diags = check_equal(env, R.params(), robots=rule_robots())
    assert {R.OVERLAP, R.CIRCLE} & {b for d in diags.values() for b in d["branches"]}
    check_equal(env, R.params(max_neighbors=48, neighbor_dist=12.8, jitter=0.2), robots=rule_robots())
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
    p = R.params(jitter=0.2)                              # (the jitter angle is drawn per robot of the ENV: world 1 differs)
    a2, a1 = two.orca_actions(orca_params(p)), one.orca_actions(orca_params(p))
    torch.cuda.synchronize()
    assert torch.equal(a2[:100].view(torch.int32), a1.view(torch.int32))
    check_equal(two, p)
    check_equal(one, p)
    two.check()
    two.close()
    one.close()


@pytest.mark.parametrize("lazy", [True, False])
def test_lazy_and_eager_views_with_small_beams(hip, lazy):
    sc = S.circle_big(70, spacing=0.9)
    sc.beams, sc.frames = 64, 1
    env = hip.VecStageWorld(sc, lazy_obs=lazy)
    rng = np.random.default_rng(22)
    env.reset()
    check_equal(env, R.params())
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    check_equal(env, R.params(obst_dist=6.0, max_neighbors=48))
    env.check()
    env.close()


def test_mask_after_a_sliced_tick(hip):
    env = hip.VecStageWorld(S.circle_big(150, spacing=0.9))
    rng = np.random.default_rng(23)
    env.reset()
    env.step(dev(U.random_actions(rng, env.N)))
    env.step(dev(U.random_actions(rng, env.N)), ray_slice=(40, 70))
    mask = np.zeros(env.N, np.uint8)
    mask[40:110] = 1
    check_equal(env, R.params(), mask=mask)
    check_equal(env, R.params(), mask=mask, with_vel=False)
    check_equal(env, R.params(), mask=np.zeros(env.N, np.uint8))
    env.check()
    env.close()


def test_the_call_writes_nothing_of_the_env(hip):
    from mrca import _lib
    sc = S.circle_big(100, spacing=0.9)
    env, twin = hip.VecStageWorld(sc, lazy_obs=False), hip.VecStageWorld(sc, lazy_obs=False)
    rng = np.random.default_rng(24)
    acts = [dev(U.random_actions(rng, env.N)) for _ in range(4)]
    for e in (env, twin):
        e.reset()
        for a in acts[:3]:
            e.step(a)
    names = ["_" + n if n in ("obs", "scan") else n for n, _dt, _shape in _lib.FIELDS]       # every MRCA_F_*
    before = {k: getattr(env, k).clone() for k in names}
    arena = env.arena.clone()
    env.orca_actions(vel=torch.zeros(env.N, 2, device=env.device))
    env.orca_actions(orca_params(R.params(neighbor_dist=19.3, max_neighbors=48)))
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k], getattr(env, k)), k
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory, the broad phase's scratch included
    env.step(acts[3])
    twin.step(acts[3])
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(twin, k), getattr(env, k)), k
    env.check()
    env.close()
    twin.close()


def test_twenty_closed_loop_ticks(hip):
    env = hip.VecStageWorld(S.circle_big(100, spacing=0.9))
    env.reset()
    p = R.params()
    for k in range(20):
        if k in (0, 5, 10, 19):
            check_equal(env, p)
        env.step(env.orca_actions())
    torch.cuda.synchronize()
    assert (env.speed_gt[:, 0] > 0).any()
    env.check()
    env.close()


def test_the_small_path_is_untouched(hip):
    env = hip.VecStageWorld(small_scenario(64, 1))
    rng = np.random.default_rng(25)
    env.reset()
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    for p in (R.params(), R.params(jitter=0.3, neighbor_dist=20.0, max_neighbors=48)):
        st = orca_params(p).struct()
        outs = []
        for fn in (env.lib.mrca_orca_actions, env.lib.mrca_orca_actions_any):
            a, v = nan_filled(env), nan_filled(env)
            assert fn(env._h, C.byref(st), None, a.data_ptr(), v.data_ptr(), env._stream()) == 0
            outs.append((a, v))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
        assert not (outs[1][0].view(torch.int32) == NAN_BITS).any()
    env.close()


# ------------------------------------------------------------------------------------------------ the error returns
def test_errors(hip):
    from mrca import _lib
    small = hip.VecStageWorld(small_scenario(64, 1))
    big = hip.VecStageWorld(S.circle_big(66))
    small.reset()
    big.reset()
    bad = [("radius", 0.0), ("radius", -1.0), ("neighbor_dist", 0.0), ("time_horizon", 0.0), ("time_horizon_obst", -2.0),
           ("max_speed", 0.0), ("obst_dist", -0.1), ("obst_dist", 6.5), ("responsibility", -0.1), ("responsibility", 1.5),
           ("max_neighbors", -1), ("max_neighbors", 49)]
    bad += [(k, v) for k in R.FIELDS[:-1] for v in (float("nan"), float("inf"))]
    for env in (small, big):
        call = env.lib.mrca_orca_actions_any
        out = torch.zeros(env.N, 2, device=env.device)
        for k, v in bad:
            st = _lib.OrcaParamsStruct()
            env.lib.mrca_orca_default_params(C.byref(st))
            setattr(st, k, v)
            rc = call(env._h, C.byref(st), None, out.data_ptr(), None, env._stream())
            assert rc == -1 and k.encode() in env.lib.mrca_last_error(), (k, v, env.lib.mrca_last_error())
            assert b"mrca_orca_actions_any" in env.lib.mrca_last_error()
        assert call(env._h, None, None, None, None, env._stream()) == -1 and b"actions_dev" in env.lib.mrca_last_error()
        assert call(env._h, None, None, out.data_ptr() + 4, None, env._stream()) == -1
        assert call(None, None, None, out.data_ptr(), None, env._stream()) == -1 and b"env is NULL" in env.lib.mrca_last_error()
        st = _lib.OrcaParamsStruct()
        env.lib.mrca_orca_default_params(C.byref(st))
        st.neighbor_dist = 19.4 if env is big else 20.0
        rc = call(env._h, C.byref(st), None, out.data_ptr(), None, env._stream())
        if env is big:
            assert rc == -4 and b"neighbor_dist" in env.lib.mrca_last_error()
            assert env.lib.mrca_last_error().decode() == "mrca_orca_actions_any: neighbor_dist 19.4 > 19.3 with robots_per_world 66 > 64 " \
                                                         "(the search looks at three rings of 6.5 m cells at most)"
            assert env.lib.mrca_orca_actions(env._h, None, None, out.data_ptr(), None, env._stream()) == -4
            assert env.lib.mrca_last_error().decode() == "mrca_orca_actions: robots_per_world 66 > 64"
            assert not out.any()
            st.neighbor_dist = 19.3
            assert call(env._h, C.byref(st), None, out.data_ptr(), None, env._stream()) == 0
            out.zero_()
        else:
            assert rc == 0                               # worlds of up to 64 robots: any neighbor_dist, as before
            out.zero_()
        env.check()                                      # no HIP error was left behind
        assert not out.any()
    # between the move phase and the observe phase the hash describes the poses BEFORE the move
    out = torch.zeros(big.N, 2, device=big.device)
    act = dev(U.random_actions(np.random.default_rng(26), big.N))
    big.move(act, (0, 1))
    rc = big.lib.mrca_orca_actions_any(big._h, None, None, out.data_ptr(), None, big._stream())
    assert rc == -1 and b"mrca_observe_worlds" in big.lib.mrca_last_error()
    assert big.lib.mrca_last_error().decode() == "mrca_orca_actions_any: the lidar hash does not describe the current poses -- call " \
                                                 "mrca_observe_worlds (after mrca_move_worlds) or mrca_reset first (robots_per_world 66 > 64)"
    big.check()
    assert not out.any()
    big.observe((0, 1))
    check_equal(big, R.params())
    twin = hip.VecStageWorld(S.circle_big(66))           # (move + observe is the tick)
    twin.reset()
    twin.step(act)
    torch.cuda.synchronize()
    assert torch.equal(twin.pose, big.pose) and torch.equal(twin.scan_ring, big.scan_ring)
    # the two phases alternate: a second move is refused (and moves nobody), a reset in between starts over, and an observe
    # phase with no move before it rebuilds the hash from the poses as they are
    big.move(act, (0, 1))
    pose = big.pose.clone()
    rc = big.lib.mrca_move_worlds(big._h, act.data_ptr(), 0, 1, big._stream())
    assert rc == -1 and b"mrca_observe_worlds" in big.lib.mrca_last_error()
    torch.cuda.synchronize()
    assert torch.equal(pose, big.pose)
    big.reset()
    twin.reset()
    check_equal(big, R.params())
    for e in (big, twin):
        e.step(act)
    big.observe((0, 1))                                  # (one more scan of the same poses)
    check_equal(big, R.params())
    big.step(act)
    twin.step(act)
    assert torch.equal(twin.pose, big.pose) and np.array_equal(host_fields(twin)[3], host_fields(big)[3])
    assert big.lib.mrca_move_worlds(big._h, act.data_ptr(), 0, 0, big._stream()) == -4       # a part of a big world: as before
    big.check()
    for e in (small, big, twin):
        e.close()


# ------------------------------------------------------------------------------------------------ the evaluator
def test_cli_one_circle_orca(hip):
    out = _evaluate(["--one-circle", "100", "--spacing", "0.9", "--orca", "--max-ticks", "50"])
    assert {"success_rate", "crash_rate", "extra_time_s", "extra_distance_m", "average_speed_mps", "robots"} <= set(out)
    assert out["robots"] == 100 and out["one_circle"] == 100 and "ORCA" in out["policy"]
    assert abs(out["radius_m"] - 100 * 0.9 / (2 * np.pi)) < 1e-3


def test_cli_one_circle_orca_first_reports_both_groups(hip):
    out = _evaluate(["--one-circle", "100", "--orca-first", "10", "--max-ticks", "50"])
    assert set(out["groups"]) == {"orca", "policy"}
    assert out["groups"]["orca"]["robots"] == 10 and out["groups"]["policy"]["robots"] == 90
    assert out["one_circle"] == 100
