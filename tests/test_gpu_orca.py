"""GPU: mrca_orca_actions -- ``actions`` and ``vel`` EQUAL, bit for bit, to the NumPy float32 restatement of tests/orca_ref.py
fed with host copies of the env's fields (small walled worlds with robots on one spot, a full wave of neighbours, a dense
circle where LP3 decides, ring heads that differ, a mask); the call reads the env and writes nothing of it; 30 closed-loop
ticks equal to the C oracle driven by the host build of the same rule; the error returns; ``mrca.evaluate --orca``.

The crafted cases -- ties between neighbours and between beams, discs that touch, the thresholds of the rule -- live in
tests/orca_cases.py, shared with tests/test_orca_host.py and tests/test_nhorca_host.py; tests/controller_inject.py puts them
into an env as ONE world (poses and goals by reset, speed_gt, scan rows and hit flags through the field views), and
``test_crafted_world_on_the_device`` asserts from the fields read back that each edge occurred.  tests/test_gpu_orca_big.py runs
the same world with 66 robots through mrca_orca_actions_any."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import orca_ref as R
import util as U
from test_orca_host import host_env_actions, shim  # noqa: F401  (shim: the host build of csrc/mrca_orca_device.h)
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN_BITS = 0x7FC0BEEF


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def orca_params(p):
    from mrca.orca import OrcaParams
    return OrcaParams(**{k: (int(v) if k == "max_neighbors" else float(v)) for k, v in p.items()})


def small_scenario(beams=512, frames=3):
    """3 worlds x 7 robots on a 40 x 40-cell map (0.5 m cells, walled, two blocks)."""
    occ = np.zeros((40, 40), bool)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = True
    occ[8:11, 25:33] = occ[28:34, 6:8] = True
    sc = S.stage1(num_worlds=3, robots_per_world=7, seed=(5 << 32) | 4, grid=S.GridData.from_dense(occ, 0.5, -10.0, -10.0))
    sc.beams, sc.frames = beams, frames
    return sc


def teleport_poses(sc, rng):
    """Robots 1 and 2 of every world on ONE spot, robot 3 0.3 m from robot 0, robot 5 of world 0 0.6 m from the wall at
    x = -9.5 and facing it."""
    W, Rn = sc.num_worlds, sc.robots_per_world
    poses = np.zeros((W, Rn, 3), f32)
    poses[..., :2] = rng.uniform(-7.0, 7.0, (W, Rn, 2))
    poses[..., 2] = rng.uniform(-np.pi, np.pi, (W, Rn))
    poses[:, 2, :2] = poses[:, 1, :2]
    poses[:, 3, :2] = poses[:, 0, :2] + f32(0.3) * np.array([1.0, 0.0], f32)
    poses[0, 5] = (-8.9, 0.0, np.pi)
    goals = rng.uniform(-7.0, 7.0, (W, Rn, 2)).astype(f32)
    return poses.reshape(-1, 3), goals.reshape(-1, 2)


def host_fields(env):
    """Host copies of what the call reads: (pose, speed_gt, goal, newest scan rows, hit flags of those rows)."""
    torch.cuda.synchronize()
    head = env.ring_head.long()
    rows = env.scan_ring[torch.arange(env.N, device=env.device), head]
    return (env.pose.cpu().numpy(), env.speed_gt.cpu().numpy(), env.goal.cpu().numpy(), rows.cpu().numpy(),
            env.hit_robot.cpu().numpy())


def nan_filled(env):
    return torch.full((env.N, 2), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)


def check_equal(env, p, mask=None, with_vel=True):
    """One call compared with orca_ref on the same fields -> the reference's diagnostics."""
    pose, speed_gt, goal, rows, hit = host_fields(env)
    act, vel = nan_filled(env), (nan_filled(env) if with_vel else None)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(env.device)
    got = env.orca_actions(orca_params(p), mask=m, out=act, vel=vel)
    assert got is act
    robots = None if mask is None else np.flatnonzero(mask).tolist()
    wact, wvel, diags = R.env_actions(p, env.R, env.scenario.seed, pose, speed_gt, goal, rows, hit, robots=robots)
    torch.cuda.synchronize()
    a = act.cpu().numpy().view(np.uint32)
    want_a = np.where(np.isnan(wact), np.uint32(NAN_BITS), wact.view(np.uint32))
    assert np.array_equal(a, want_a), (np.argwhere(a != want_a)[:5], act.cpu().numpy()[:8], wact[:8])
    if with_vel:
        v = vel.cpu().numpy().view(np.uint32)
        want_v = np.where(np.isnan(wvel), np.uint32(NAN_BITS), wvel.view(np.uint32))
        assert np.array_equal(v, want_v), np.argwhere(v != want_v)[:5]
    return diags


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3)])
def test_small_worlds_equal_the_reference(hip, beams, frames, lazy):
    sc = small_scenario(beams, frames)
    env = hip.VecStageWorld(sc, lazy_obs=lazy)
    rng = np.random.default_rng(2)
    poses, goals = teleport_poses(sc, rng)
    env.reset(None, torch.from_numpy(poses).cuda(), torch.from_numpy(goals).cuda())
    seen = set()
    for p in (R.params(), R.params(jitter=0.3, obst_dist=6.0, max_neighbors=3)):
        for d in check_equal(env, p).values():          # right after the teleport: robots on one spot, one at the wall
            seen |= set(d["branches"])
    assert R.OVERLAP in seen
    for _ in range(10):
        env.step(torch.from_numpy(U.random_actions(rng, env.N)).cuda())
    diags = check_equal(env, R.params())
    assert any(d["n_static"] > 0 for d in diags.values())
    check_equal(env, R.params(jitter=0.3, obst_dist=6.0, neighbor_dist=20.0, responsibility=1.0, time_horizon_obst=3.0))
    env.close()


@pytest.mark.parametrize("max_neighbors", [10, 48])
def test_a_full_wave_of_neighbours(hip, max_neighbors):
    env = hip.VecStageWorld(S.circle_n(64, 6.0))
    env.reset()
    diags = check_equal(env, R.params(max_neighbors=max_neighbors, neighbor_dist=20.0))
    assert max(len(d["branches"]) - d["n_static"] for d in diags.values()) == max_neighbors
    env.close()


def crafted_world_checks(env, beams):
    """``orca_cases.device_world`` written into every world of ``env`` (tests/controller_inject.py) under every set of
    ``device_params``: equal to the restatement, and each edge occurred -- asserted from the fields read back"""
    import controller_inject as J
    import orca_cases as K
    J.write_world(env, K.device_world(env.R, beams))
    pose, speed_gt, goal, rows, hit = host_fields(env)
    for p in K.device_params():
        diags = check_equal(env, p)
        for w in range(env.W):
            K.device_expectations(p, w * env.R, beams, pose, speed_gt, goal, rows, hit, diags, robots=env.R)
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    check_equal(env, K.device_params()[1], mask=mask)
    env.check()


@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_crafted_world_on_the_device(hip, beams):
    """Four neighbours at one distance and max_neighbors cutting through the tie, two robots on one spot, centres at exactly
    2 * radius and one ulp either side, a robot exactly on its goal, speed_gt of 0, -0.0 and the speed limit; sector minima
    that tie, empty sectors, a minimum that carries the hit-robot flag, a return at exactly obst_dist and one ulp below: two
    open worlds of 34 robots whose ring heads differ."""
    import controller_inject as J
    import orca_cases as K
    env = J.open_env(hip, K.N_CASES + 1, beams)
    crafted_world_checks(env, beams)
    env.close()


def test_a_robot_alone_in_its_world(hip):
    env = hip.VecStageWorld(S.circle_n(1, 6.0, num_worlds=2))
    env.reset()
    diags = check_equal(env, R.params())
    assert all(len(d["branches"]) == d["n_static"] for d in diags.values())
    env.close()


def go_to_goal(local_goal):
    lx, ly = local_goal[:, 0].astype(np.float64), local_goal[:, 1].astype(np.float64)
    b = np.arctan2(ly, lx)
    return np.stack([(np.abs(b) < 1.0) * 1.0, np.clip(2.0 * b, -1.0, 1.0)], 1).astype(f32)


def test_dense_circle_where_lp3_decides(hip):
    env = hip.VecStageWorld(S.circle_n(50, 3.0))
    env.reset()
    # 40 go-to-goal ticks (checked on the CPU with the C oracle and the host build: at ticks 0, 1, 5, 10, 20, 40 and 60 LP2 falls
    # short and LP3 changes the result for all 50 robots -- they stand shoulder to shoulder, every pair of discs overlaps)
    for _ in range(40):
        torch.cuda.synchronize()
        env.step(torch.from_numpy(go_to_goal(env.local_goal.cpu().numpy())).cuda())
    diags = check_equal(env, R.params())
    assert sum(d["lp3_changed"] for d in diags.values()) >= 1
    check_equal(env, R.params(max_neighbors=48))
    env.close()


def test_ring_heads_that_differ_between_robots(hip):
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(6)
    env.reset()
    for _ in range(4):
        env.step(torch.from_numpy(U.random_actions(rng, env.N)).cuda())
    env.step(torch.from_numpy(U.random_actions(rng, env.N)).cuda(), worlds=(0, 1))       # world 0 alone, once more
    torch.cuda.synchronize()
    heads = env.ring_head.cpu().numpy()
    assert len(set(heads.tolist())) > 1
    check_equal(env, R.params(obst_dist=6.0))
    env.close()


def test_mask_keeps_the_other_rows_and_vel_is_optional(hip):
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    env.reset()
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    check_equal(env, R.params(), mask=mask)              # (rows with mask 0 keep the NaN pattern exactly)
    check_equal(env, R.params(), mask=mask, with_vel=False)
    check_equal(env, R.params(), with_vel=False)
    check_equal(env, R.params(), mask=np.zeros(env.N, np.uint8))
    env.close()


def test_the_call_writes_nothing_of_the_env(hip):
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc, lazy_obs=False)
    rng = np.random.default_rng(8)
    env.reset()
    for _ in range(3):
        env.step(torch.from_numpy(U.random_actions(rng, env.N)).cuda())
    names = U.STATE_FIELDS + ["scan_ring", "ring_head", "hit_bits", "fresh"]
    before = {k: getattr(env, k).clone() for k in names}
    arena = env.arena.clone()
    env.orca_actions(vel=torch.zeros(env.N, 2, device=env.device))
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k], getattr(env, k)), k
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory
    env.close()


def test_thirty_closed_loop_ticks_equal_the_oracle(hip, shim):  # noqa: F811
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    ora = U.COracleEnv(sc)
    poses, goals = teleport_poses(sc, np.random.default_rng(2))
    env.reset(None, torch.from_numpy(poses).cuda(), torch.from_numpy(goals).cuda())
    ora.reset(None, poses, goals)
    p = R.params(jitter=0.2)
    for k in range(30):
        a = env.orca_actions(orca_params(p))
        act, _v, _d, _l, _c = host_env_actions(shim, p, sc.robots_per_world, sc.seed, ora.pose, ora.speed_gt, ora.goal, ora.scan,
                                               ora.hit_robot)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), act.view(np.uint32)), k
        env.step(a)
        ora.step(act)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
        U.assert_hits_equal(env, ora, what=f"tick {k}")
    env.close()


def test_errors(hip):
    from mrca import _lib
    big = hip.VecStageWorld(S.circle_big(66))
    big.reset()
    out = torch.zeros(big.N, 2, device=big.device)
    rc = big.lib.mrca_orca_actions(big._h, None, None, out.data_ptr(), None, big._stream())
    assert rc == -4 and b"robots_per_world" in big.lib.mrca_last_error()
    big.check()
    big.close()
    env = hip.VecStageWorld(small_scenario(64, 1))
    env.reset()
    out = torch.zeros(env.N, 2, device=env.device)
    bad = [("radius", 0.0), ("radius", -1.0), ("neighbor_dist", 0.0), ("time_horizon", 0.0), ("time_horizon_obst", -2.0),
           ("max_speed", 0.0), ("obst_dist", -0.1), ("obst_dist", 6.5), ("responsibility", -0.1), ("responsibility", 1.5),
           ("max_neighbors", -1), ("max_neighbors", 49)]
    bad += [(k, v) for k in R.FIELDS[:-1] for v in (float("nan"), float("inf"))]
    for k, v in bad:
        st = _lib.OrcaParamsStruct()
        env.lib.mrca_orca_default_params(C.byref(st))
        setattr(st, k, v)
        rc = env.lib.mrca_orca_actions(env._h, C.byref(st), None, out.data_ptr(), None, env._stream())
        assert rc == -1 and k.encode() in env.lib.mrca_last_error(), (k, v, env.lib.mrca_last_error())
    assert env.lib.mrca_orca_actions(env._h, None, None, None, None, env._stream()) == -1
    assert env.lib.mrca_orca_actions(env._h, None, None, out.data_ptr() + 4, None, env._stream()) == -1
    env.check()                                          # no HIP error was left behind
    assert not out.any()
    env.close()


def _evaluate(args):
    cmd = [sys.executable, "-m", "mrca.evaluate"] + args
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_cli_orca(hip):
    out = _evaluate(["--circles", "2", "--orca", "--max-ticks", "50", "--orca-param", "jitter=0.1", "--orca-param", "max_neighbors=12"])
    assert {"success_rate", "crash_rate", "extra_time_s", "extra_distance_m", "average_speed_mps", "robots"} <= set(out)
    assert out["robots"] == 100 and out["orca_params"]["max_neighbors"] == 12 and "ORCA" in out["policy"]


def test_cli_orca_first_reports_both_groups(hip):
    ckpt = os.path.join(U.ROOT, "rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")
    out = _evaluate(["--circles", "2", "--orca-first", "10", "--policy", ckpt, "--max-ticks", "50"])
    assert set(out["groups"]) == {"orca", "policy"}
    assert out["groups"]["orca"]["robots"] == 20 and out["groups"]["policy"]["robots"] == 80
    assert {"success_rate", "crash_rate", "extra_time_s"} <= set(out["groups"]["orca"])
