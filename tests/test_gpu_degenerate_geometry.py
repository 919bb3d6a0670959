"""The env kernels against the C oracle on degenerate poses and commands (run with -m gpu on an MI355X).

Every other GPU parity test draws poses and commands from continuous distributions, which land on a cell boundary, a
cardinal heading, an exact contact or an exact zero command with probability zero -- the inputs on which the device code
differs from what the CPU gates compile (rcp_exact's v_rcp_f32 + Newton step, med3, float-to-int conversions, the NaN rules of
v_min / v_max, the sign of a zero).  tests/degenerate_scenes.py holds such scenes as data; tests/test_degenerate_scenes_host.py
shows on the CPU that the NumPy oracle, the C oracle and the host build agree on them and that each scene meets the edges it is
there for.  Here every scene runs in the HIP library: all nine ray-cast families, lazy and eager views, every field of
U.STATE_FIELDS and the hit flags after the reset and after EVERY tick, bit for bit (a -0.0 range is a -0.0 range).  Further:
the same scenes through mrca_step_many (the multi-tick ray cast is another instantiation of the body), a tick of non-finite
commands on move_kernel and bw_integrate_kernel, a masked mrca_reset back onto the degenerate poses in mid-run, and the sign
bit of a zero range against the observation."""
import numpy as np
import pytest
import torch

import degenerate_scenes as D
import util as U
from test_gpu_raycast_variants import RawView, host_copy, selection

pytestmark = pytest.mark.gpu

FLOAT_FIELDS = ("pose", "speed", "speed_gt", "goal", "init_pose", "scan", "obs", "local_goal", "reward", "prev_dist")


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


def compare(env, eager, want, what):
    torch.cuda.synchronize()
    U.assert_state_equal(RawView(env, eager), want, what=what)
    U.assert_hits_equal(env, want, what=what)


def assert_finite(env, what):
    for k in FLOAT_FIELDS:
        assert bool(torch.isfinite(getattr(env, k)).all()), f"{what}: {k} is not finite"


def the_run(name):
    run = D.oracle_run(name)
    missing = D.missing_flags(name, run.flags)
    assert not missing, f"{name}: the oracle's run does not exercise {missing}"
    sc = D.scenario(name)
    assert selection(sc) == D.SCENES[name].selects
    return run, sc


# ------------------------------------------------------------------------------------------------ mrca_step, every family
@pytest.mark.parametrize("lazy_obs", [True, False], ids=["lazy", "eager"])
@pytest.mark.parametrize("name", list(D.SCENES))
def test_scene_bit_exact_after_every_tick(hip, name, lazy_obs):
    run, sc = the_run(name)
    env = hip.VecStageWorld(sc, lazy_obs=lazy_obs)
    mode = "lazy" if lazy_obs else "eager"
    env.reset(None, dev(run.poses), dev(run.goals))
    compare(env, not lazy_obs, run.snaps[-1], f"{name} {mode} reset")
    for k, a in enumerate(run.actions):
        env.step(dev(a))
        compare(env, not lazy_obs, run.snaps[k], f"{name} {mode} tick {k}")
    assert_finite(env, f"{name} {mode}")
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ mrca_step_many
MANY = [(name, chains, tpl) for name in ("coarse_exact_k2", "fine_exact_k1", "raster8_k2") for chains in (1, 2)
        for tpl in ((None, 3) if name == "raster8_k2" else (None,))]


@pytest.mark.parametrize("name,chains,ticks_per_launch", MANY)
def test_step_many_on_degenerate_scenes(hip, monkeypatch, name, chains, ticks_per_launch):
    """calls of 1, 3 and 7 ticks (raycast_ticks_kernel casts several ticks' rays per launch; the raster shape does so under
    MRCA_TICKS_PER_LAUNCH=3 only), after each the oracle stepped tick by tick"""
    if ticks_per_launch is None:
        monkeypatch.delenv("MRCA_TICKS_PER_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", str(ticks_per_launch))
    run, sc = the_run(name)
    env = hip.VecStageWorld(sc)                                    # (the switch is read here, once)
    pool = [dev(a) for a in run.actions]
    env.reset(None, dev(run.poses), dev(run.goals))
    k = 0
    for K in (1, 3, 7):
        env.step_many(pool, k, K, chains)
        env.invalidate_views()
        k += K
        compare(env, False, run.snaps[k - 1], f"{name}, chains {chains}, after the call of {K} ticks")
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ non-finite commands
@pytest.mark.parametrize("name", ["coarse_exact_k1", "big_k1", "stage2_hold"])
def test_non_finite_commands_idle_the_robot(hip, name):
    """move_kernel (worlds of at most 64 robots), bw_integrate_kernel (a world of 66) and hold_velocity with dead robots: ticks
    in which five of every six commands are non-finite, between ordinary ones.  A live robot whose two components are
    non-finite keeps its pose and stores (0, 0) as its speed; every field equals the oracle's and stays finite."""
    run, sc = the_run(name)
    env, ora = hip.VecStageWorld(sc), U.COracleEnv(sc)
    env.reset(None, dev(run.poses), dev(run.goals))
    ora.reset(None, run.poses, run.goals)
    bad = D.non_finite_commands(sc.num_robots)
    idled = 0
    for k, a in enumerate([run.actions[0], run.actions[1], bad, run.actions[2], bad, run.actions[3]]):
        before, live = env.pose.clone(), env.live.clone().bool()
        env.step(dev(a))
        ora.step(a)
        compare(env, False, host_copy(ora), f"{name} call {k}")
        assert_finite(env, f"{name} call {k}")
        if a is bad:
            idle = live & dev(~np.isfinite(a).any(1)) & (env.done == 0)
            idled += int(idle.sum())
            assert torch.equal(env.pose[idle].view(torch.int32), before[idle].view(torch.int32))
            assert bool((env.speed[idle].view(torch.int32) == 0).all())
            sane = dev(np.where(np.isfinite(a), a, np.float32(0.0)).astype(np.float32))
            kept = live & (env.done == 0)
            assert torch.equal(env.speed[kept].view(torch.int32), sane[kept].view(torch.int32))
    assert idled >= 8
    if D.SCENES[name].stage2:
        assert bool((env.live == 0).any()), "no dead robot: hold_velocity's path was not taken"
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ a teleport in mid-run
@pytest.mark.parametrize("name", ["fine_exact_k2", "raster4_k1", "big_k2"])
def test_masked_reset_onto_the_degenerate_poses(hip, name):
    """ten ticks into a run every second robot is put back onto its degenerate pose by a masked mrca_reset (the path of a
    caller's teleport: the others keep their state and their scans), then five more ticks; lazy and eager"""
    run, sc = the_run(name)
    lazy, eager, ora = hip.VecStageWorld(sc), hip.VecStageWorld(sc, lazy_obs=False), U.COracleEnv(sc)
    for e in (lazy, eager):
        e.reset(None, dev(run.poses), dev(run.goals))
    ora.reset(None, run.poses, run.goals)
    mask = (np.arange(sc.num_robots) % 2 == 0).astype(np.uint8)

    def tick(k):
        a = D.commands(name, k)
        for e in (lazy, eager):
            e.step(dev(a))
        ora.step(a)
        want = host_copy(ora)
        compare(lazy, False, want, f"{name} lazy tick {k}")
        compare(eager, True, want, f"{name} eager tick {k}")

    for k in range(10):
        tick(k)
    for e in (lazy, eager):
        e.reset(dev(mask), dev(run.poses), dev(run.goals))
    ora.reset(mask, run.poses, run.goals)
    want = host_copy(ora)
    compare(lazy, False, want, f"{name} lazy masked reset")
    compare(eager, True, want, f"{name} eager masked reset")
    assert (want.pose[mask == 1].view(np.uint32) == run.poses[mask == 1].view(np.uint32)).all()
    assert (want.scan.view(np.uint32) == 0x80000000).any()          # the robot on the block's face is back: -0.0 ranges again
    for k in range(10, 15):
        tick(k)
    for e in (lazy, eager):
        e.check()
        e.close()


# ------------------------------------------------------------------------------------------------ the sign of a zero range
def test_the_sign_of_a_zero_range_does_not_reach_an_observation(hip):
    """a robot exactly on the face of a block has -0.0 ranges (the oracle's, the device's: compared above).  The newest
    observation row equals mrca_normalize_scans of the scan and the host's |x| / 6 - 0.5: -0.5 where the range is -0.0"""
    from mrca import policy_ops
    name = "coarse_exact_k1"
    run, sc = the_run(name)
    for lazy_obs in (True, False):
        env = hip.VecStageWorld(sc, lazy_obs=lazy_obs)
        env.reset(None, dev(run.poses), dev(run.goals))
        for k in range(3):
            scan = env.scan.cpu().numpy()
            zero = scan.view(np.uint32) == 0x80000000
            if k == 0:
                assert zero.sum() >= sc.beams // 2, "no -0.0 range: the scene does not test what it says"
            newest = env.obs[:, -1]
            assert torch.equal(newest, policy_ops.normalize_scans(env.scan))
            host = np.abs(scan) / np.float32(6.0) - np.float32(0.5)
            assert np.array_equal(newest.cpu().numpy().view(np.uint32), host.view(np.uint32))
            assert (newest.cpu().numpy()[zero] == np.float32(-0.5)).all()
            env.step(dev(run.actions[k]))
        env.check()
        env.close()
