"""GPU: hybrid control in the paper's form -- the two front ends with a per-robot scan scale
(mrca_lidar_features_scaled, mrca_lidar_features_bf16_scaled), mrca_hybrid_plan and mrca_hybrid_commit.

* scale = 1 is the identity: every bit of the unscaled entry, at n = 1, 2, 3, 5 and at the depth of the kernels' pipelines;
* mixed factors, to the bit: the scaled entry equals the UNSCALED entry run on a ring pre-scaled on the host
  (tests/safe_ref.py: scaled_ring) -- the arithmetic behind the multiply is the same on the same inputs, so there is no
  tolerance.  The factors are dealt so that robots one stride apart differ: a factor fetched one stride short (the slip the
  head of tests/test_gpu_rollout_inference.py records for the frame rows) or applied to two frames of three cannot pass;
* the plan on real envs, every robot, bit for bit against safe_ref fed with the fields read back, mode and clearances also
  against mrca_hybrid_actions on the same state;
* the closed loop plan -> act_fused(scan_scale) -> commit -> step against the host chain (safe_ref plan -> act_fused on a
  pre-scaled copy of the ring -> safe_ref commit) and the C oracle;
* masks, in place, the arena untouched, a captured tick, the error returns, ``mrca.evaluate --hybrid-safe``.

The crafted cases of plan and commit live in tests/hybrid_cases.py and tests/safe_cases.py, shared with the host tests
(tests/test_hybrid_host.py, tests/test_safe_host.py); tests/controller_inject.py writes the plan's rows into an env, one case
per robot, and the two tests "on the device" assert from what is read back that each case stood on its edge."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import controller_inject as J
import hybrid_cases as HK
import hybrid_ref as R
import safe_cases as K
import safe_ref as SR
import util as U
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN_BITS = 0x7FC0BEEF
MODE_SENTINEL = 12345
CKPT = os.path.join(U.ROOT, "rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")
FACTORS = np.array([1.0, 0.5, 0.8, 0.7, 2.0 ** -20], f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    from mrca.net import CNNPolicy
    pol = CNNPolicy(3, 2).cuda()
    pol.load_state_dict(torch.load(CKPT, map_location="cuda"))
    rc = pol._rollout_cache()
    return {"env": vec_env, "pol": pol, "w": (rc["w1"], rc["b1"], rc["w2"], rc["b2"]),
            "cus": torch.cuda.get_device_properties(0).multi_processor_count}


# ------------------------------------------------------------------------------------------------ the front ends
def geometry(cus, bf16, n=None):
    """-> (n, stride): the robots a wave pair walks are n0, n0 + stride, ...  fp32 (csrc/mrca_policy.hip): one workgroup of two
    (actor, critic) wave pairs per CU, no more than there is work for; bf16 (csrc/mrca_policy_bf16.hip): 4 SIMDs x 2 one-wave
    workgroups per CU in pairs.  n = None: the pipeline's depth -- 6 CUs + 5 robots (fp32), 16 CUs + 5 (bf16)."""
    if bf16:
        n = 16 * cus + 5 if n is None else n
        return n, min(cus * 4 * 2 // 2, n)
    n = 6 * cus + 5 if n is None else n
    return n, 2 * min(cus, (n + 1) // 2)


def deep_ring(n, stride, seed):
    """A ring of raw ranges in [0, 6] with exact 0.0, -0.0 and 6.0 among them and per-robot head slots, all three present inside
    every run of ``stride`` robots of three or more."""
    rng = np.random.default_rng(seed)
    ring = (rng.random((n, 3, 512), dtype=f32) * f32(6.0)).astype(f32)
    ring[0::7, :, 5] = 0.0
    ring[3::7, :, 6] = -0.0
    ring[5::7, :, 7] = 6.0
    ring[n - 1, 2, 511] = -0.0
    ring[0, 0, 0], ring[0, 1, 1], ring[0, 2, 2] = 6.0, 0.0, -0.0
    ring[n - 1, 1, 3] = np.nextafter(f32(6.0), f32(0.0))
    assert ring.min() == 0.0 and ring.max() == 6.0 and np.signbit(ring).any()
    slots = rng.integers(0, 3, n).astype(np.uint8)
    for lo in range(0, n, stride):
        if min(n - lo, stride) >= 3:
            slots[lo: lo + 3] = (0, 1, 2)
            assert set(slots[lo: lo + stride].tolist()) == {0, 1, 2}, lo
    return ring, slots


def deal_factors(n, stride, seed):
    """A factor of FACTORS per robot such that robots one stride apart DIFFER (so the factor is no function of n mod stride),
    with the first and the last robot of every depth on a factor below 1."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(FACTORS), n)
    depth = -(-n // stride)
    pinned = {}
    for d in range(depth):
        pinned[d * stride] = 1 + d % 4
        pinned[min((d + 1) * stride, n) - 1] = 1 + (d + 1) % 4
    if n - 1 - stride in pinned and n - 1 - stride >= 0 and pinned[n - 1 - stride] == pinned[n - 1]:
        pinned[n - 1] = 1 + (pinned[n - 1]) % 4
    for k, v in pinned.items():
        idx[k] = v
    for k in range(n):
        if k in pinned:
            continue
        avoid = {int(idx[k - stride])} if k >= stride else set()
        if k + stride in pinned:
            avoid.add(pinned[k + stride])
        while int(idx[k]) in avoid:
            idx[k] = (idx[k] + 1) % len(FACTORS)
    s = FACTORS[idx]
    # asserted on the host, as the kernel's failure modes are: one stride apart differ; every depth's ends are scaled
    assert all(s[k] != s[k - stride] for k in range(stride, n)), "robots one stride apart must differ"
    assert all(s[k] < 1.0 for k in pinned) and (n == 1 or len(set(s.tolist())) > 1)
    if n > stride:
        assert any(s[k] != s[k % stride] for k in range(n))              # not a function of n mod stride
    return s


def front_end(bf16):
    from mrca import policy_ops
    return policy_ops.lidar_features_bf16 if bf16 else policy_ops.lidar_features


SIZES = [1, 2, 3, 5, None]        # None: the pipeline's depth


@pytest.mark.parametrize("bf16", [False, True])
def test_ones_are_the_identity(hip, bf16):
    from mrca.policy_ops import RingHead
    fn = front_end(bf16)
    for size in SIZES:
        n, stride = geometry(hip["cus"], bf16, size)
        if size is None:
            assert -(-n // stride) == (5 if bf16 else 4) and n % stride == 5
        ring, slots = deep_ring(n, stride, seed=11 + n)
        x, head = dev(ring), RingHead(dev(slots), raw=True)
        want = fn(x, *hip["w"], head=head)
        got = fn(x, *hip["w"], head=head, scale=torch.ones(n, device="cuda"))
        torch.cuda.synchronize()
        assert got.dtype == want.dtype and torch.equal(got, want), (n, bf16)


@pytest.mark.parametrize("bf16", [False, True])
def test_mixed_factors_equal_the_unscaled_entry_on_a_prescaled_ring(hip, bf16):
    from mrca.policy_ops import RingHead
    fn = front_end(bf16)
    for size in SIZES:
        n, stride = geometry(hip["cus"], bf16, size)
        ring, slots = deep_ring(n, stride, seed=23 + n)
        s = deal_factors(n, stride, seed=5 + n)
        head = RingHead(dev(slots), raw=True)
        got = fn(dev(ring), *hip["w"], head=head, scale=dev(s))
        want = fn(dev(SR.scaled_ring(ring, s)), *hip["w"], head=head)
        plain = fn(dev(ring), *hip["w"], head=head)
        torch.cuda.synchronize()
        bad = (got != want).flatten(2).any(2).any(0).nonzero().flatten().tolist()
        assert not bad, (n, stride, bf16, bad[:8], [float(s[k]) for k in bad[:8]])
        # (and the factors do something: every robot whose factor is below 1 differs from the unscaled result)
        differs = (got != plain).flatten(2).any(2).any(0).cpu().numpy()
        assert np.array_equal(differs, s < 1.0), (n, bf16)


def test_the_python_layer_refuses_what_cannot_be_rescaled(hip):
    from mrca import policy_ops
    x, s = torch.zeros(4, 3, 512, device="cuda"), torch.ones(4, device="cuda")
    slots = torch.zeros(4, dtype=torch.uint8, device="cuda")
    for fn in (policy_ops.lidar_features, policy_ops.lidar_features_bf16):
        for head in (None, slots, policy_ops.RingHead(slots, raw=False)):
            with pytest.raises(ValueError, match="raw=True"):
                fn(x, *hip["w"], head=head, scale=s)
        with pytest.raises(ValueError):
            fn(x, *hip["w"], head=policy_ops.RingHead(slots, raw=True), scale=torch.ones(5, device="cuda"))
    lib = hip["env"]._lib.load()
    a = [x.data_ptr(), slots.data_ptr(), s.data_ptr(), 4, 3, 512] + [w.data_ptr() for w in hip["w"]] + [x.data_ptr(), None]
    for name in ("mrca_lidar_features_scaled", "mrca_lidar_features_bf16_scaled"):
        assert getattr(lib, name)(a[0], None, *a[2:]) == -1 and getattr(lib, name)(a[0], a[1], None, *a[3:]) == -1
        assert getattr(lib, name)(*a[:4], 2, *a[5:]) == -4 and getattr(lib, name)(*a[:5], 256, *a[6:]) == -4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the plan on real envs
def small_scenario(beams=512, frames=3):
    """3 worlds x 7 robots on a 40 x 40-cell map (0.5 m cells, walled, two blocks): the scene of tests/test_gpu_hybrid.py"""
    occ = np.zeros((40, 40), bool)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = True
    occ[8:11, 25:33] = occ[28:34, 6:8] = True
    sc = S.stage1(num_worlds=3, robots_per_world=7, seed=(5 << 32) | 4, grid=S.GridData.from_dense(occ, 0.5, -10.0, -10.0))
    sc.beams, sc.frames = beams, frames
    return sc


def parity_scene(sc, rng):
    """Robots 1 and 2 of every world on ONE spot, robot 3 0.3 m from robot 0, robot 5 of world 0 0.6 m from a wall and facing it
    (mode 2); robot 4 of every world 0.2 m from its goal (mode -2), robot 6 looking at its goal 3 m ahead (mode 1 where nothing
    stands in between).  Drawn exactly as tests/test_gpu_hybrid.py draws it."""
    W, Rn = sc.num_worlds, sc.robots_per_world
    poses = np.zeros((W, Rn, 3), f32)
    poses[..., :2] = rng.uniform(-7.0, 7.0, (W, Rn, 2))
    poses[..., 2] = rng.uniform(-np.pi, np.pi, (W, Rn))
    poses[:, 2, :2] = poses[:, 1, :2]
    poses[:, 3, :2] = poses[:, 0, :2] + f32(0.3) * np.array([1.0, 0.0], f32)
    poses[0, 5] = (-8.9, 0.0, np.pi)
    goals = rng.uniform(-7.0, 7.0, (W, Rn, 2)).astype(f32)
    poses, goals = poses.reshape(-1, 3), goals.reshape(-1, 2)
    for w in range(W):
        goals[w * Rn + 4] = poses[w * Rn + 4, :2] + f32(0.2)
        th = poses[w * Rn + 6, 2]
        goals[w * Rn + 6] = poses[w * Rn + 6, :2] + f32(3.0) * np.array([np.cos(th), np.sin(th)], f32)
    return poses, goals


def seeded_commands(rng, n):
    return np.stack([rng.uniform(0, 1, n), rng.uniform(-1, 1, n)], 1).astype(f32)


def host_fields(env):
    """Host copies of what the plan reads of the env: (local_goal, newest scan rows)."""
    torch.cuda.synchronize()
    rows = env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()]
    return env.local_goal.cpu().numpy(), rows.cpu().numpy()


def hybrid_params(p):
    from mrca.hybrid import HybridParams
    return HybridParams(**{k: float(v) for k, v in p.items()})


def safe_params(sp):
    from mrca.hybrid import SafePolicyParams
    return SafePolicyParams(**{k: float(v) for k, v in sp.items()})


def sentinels(env):
    """outputs filled with patterns no plan writes"""
    mode = torch.full((env.N,), MODE_SENTINEL, dtype=torch.int32, device=env.device)
    scale, pid, clear = (torch.full(shape, NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)
                         for shape in ((env.N,), (env.N, 2), (env.N, 3)))
    return mode, scale, pid, clear


def check_plan(env, p, sp, mask=None, fields=None, with_clear=True, goal_dev=None):
    """One plan compared with safe_ref on the same fields, every robot, and with mrca_hybrid_actions on the same state
    -> the reference's (mode, scale, pid, clear).  ``goal_dev``: a float32[N,2] tensor that goes in through
    mrca_hybrid_plan_goal; the reference is then fed with a host copy of it in place of ``local_goal``."""
    goal, rows = fields or host_fields(env)
    if goal_dev is not None:
        goal = goal_dev.cpu().numpy()
    mode, scale, pid, clear = sentinels(env)
    m = None if mask is None else dev(np.ascontiguousarray(mask, np.uint8))
    got = env.hybrid_plan(hybrid_params(p), safe_params(sp), mask=m, mode=mode, scale=scale, pid=pid, clear=clear if with_clear else None,
                          goal=goal_dev)
    assert got[0] is mode and got[1] is scale and got[2] is pid
    hmode, hclear = torch.zeros_like(mode), torch.zeros_like(clear)
    env.hybrid_actions(dev(seeded_commands(np.random.default_rng(0), env.N)), hybrid_params(p), mode=hmode, clear=hclear, goal=goal_dev)
    wmode, wscale, wpid, wclear = SR.plan(p, sp, goal, rows)
    sel = np.ones(env.N, bool) if mask is None else np.asarray(mask).astype(bool)
    torch.cuda.synchronize()
    nan = np.uint32(NAN_BITS)
    assert np.array_equal(mode.cpu().numpy(), np.where(sel, wmode, MODE_SENTINEL)), (mode.cpu().numpy(), wmode)
    assert np.array_equal(bits(scale.cpu().numpy()), np.where(sel, bits(wscale), nan))
    assert np.array_equal(bits(pid.cpu().numpy()), np.where(sel[:, None], bits(wpid), nan))
    if with_clear:
        assert np.array_equal(bits(clear.cpu().numpy()), np.where(sel[:, None], bits(wclear), nan))
    else:
        assert (clear.view(torch.int32) == NAN_BITS).all()
    # exactly the mode and the clearances mrca_hybrid_actions reports on the same state
    assert np.array_equal(hmode.cpu().numpy(), wmode) and np.array_equal(bits(hclear.cpu().numpy()), bits(wclear))
    return wmode, wscale, wpid, wclear


# ------------------------------------------------------------------------------------------------ the crafted cases, on the device
@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_plan_on_the_crafted_rows_on_the_device(hip, beams):
    """``hybrid_cases.device_cases`` (every edge of the rule on the env's own beam table, lone returns on the first and the last
    lane of the first and the last round, all B beams blocking, ranges of 0.0 and -0.0) written into an env one case per robot
    and planned: mode, scale, pid and clear, the scale on the edges of the risk rule; with and without a mask, and with the
    goals handed to mrca_hybrid_plan_goal while ``local_goal`` holds something else.  That each row stood on its edge is
    asserted from the fields read back."""
    names, goal, policy, rows = HK.device_cases(beams)
    env = J.walled_env(hip["env"], beams, len(names))
    J.write_cases(env, 0, local_goal=goal, rows=rows)
    assert J.heads_differ(env)
    rng = np.random.default_rng(beams)
    pol = seeded_commands(rng, env.N)
    pol[:len(names)] = policy
    p, sp = R.params(**HK.PARAMS), SR.params(**K.PLAN_SAFE)
    goals = env.local_goal.clone()
    for goal_dev in (None, goals):
        if goal_dev is not None:
            env.local_goal[:] = dev(rng.uniform(-5.0, 5.0, (env.N, 2)).astype(f32))
        wmode, wscale, wpid, wclear = check_plan(env, p, sp, goal_dev=goal_dev)
        back = host_fields(env)[1]
        hact, hmode, hclear, nb = R.env_actions(p, goals.cpu().numpy(), pol, back)
        HK.expectations(names, p, pol, back, hact, hmode, hclear, nb)
        K.plan_expectations(names, sp, wmode, wscale, wpid, wclear, (hact, hmode, hclear))
        check_plan(env, p, sp, mask=(np.arange(env.N) % 3 != 1).astype(np.uint8), goal_dev=goal_dev)
        check_plan(env, R.params(), SR.params(), goal_dev=goal_dev)      # (the same rows off their edges, under the defaults)
    env.check()
    env.close()


def test_commit_under_special_commands_in_every_mode_on_the_device(hip):
    """``safe_cases.commit_cases`` (NaN, Inf, -0.0, v at the cap and one ulp either side, in every mode and in two that are
    none) through mrca_hybrid_commit: out of place and in place, without a mask, under a mask and under its complement."""
    mode, pid, policy = K.commit_cases()
    n = len(mode)
    env = hip["env"].VecStageWorld(J.small_walled_scenario(64, 1, n))     # (the commit reads nothing of the env but its size)
    rng = np.random.default_rng(7)
    N = env.N
    mode = np.concatenate([mode, rng.integers(-2, 3, N - n).astype(np.int32)])
    pid = np.concatenate([pid, seeded_commands(rng, N - n)])
    policy = np.concatenate([policy, seeded_commands(rng, N - n)])
    sp = SR.params(**K.COMMIT_SAFE)
    ssp = safe_params(sp)
    want = SR.commit(sp, mode, pid, policy)
    K.commit_expectations(want[:n], pid[:n], policy[:n])                  # (the restatement stands on the edges ...)
    nan_out = torch.full((N, 2), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)
    dmode, dpid = dev(mode), dev(pid)
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    out = env.hybrid_commit(dev(policy), dmode, dpid, ssp, out=nan_out.clone())
    inpl = env.hybrid_commit(dev(policy), dmode, dpid, ssp)
    part = env.hybrid_commit(dev(policy), dmode, dpid, ssp, mask=dev(mask), out=nan_out.clone())
    both = env.hybrid_commit(dev(policy), dmode, dpid, ssp, mask=dev(1 - mask), out=part.clone())
    part_in = env.hybrid_commit(dev(policy), dmode, dpid, ssp, mask=dev(mask))
    torch.cuda.synchronize()
    sel = mask.astype(bool)[:, None]
    for got in (out, inpl, both):                                         # (... and the device equals it, bit for bit)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), np.argwhere(bits(got.cpu().numpy()) != bits(want))[:5]
    K.commit_expectations(out.cpu().numpy()[:n], pid[:n], policy[:n])
    assert np.array_equal(bits(part.cpu().numpy()), np.where(sel, bits(want), np.uint32(NAN_BITS)))
    assert np.array_equal(bits(part_in.cpu().numpy()), np.where(sel, bits(want), bits(policy)))
    env.check()
    env.close()


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3), (1024, 2)])
def test_plan_on_small_worlds_equals_the_restatement(hip, beams, frames, lazy):
    """3 worlds x 7 robots = 21 robots: the last workgroup (4 robots each) has three empty waves.  The run is the one of
    tests/test_gpu_hybrid.py (same scene, same seed, driven by the command-scaling rule's output), on which every mode occurs;
    the C oracle runs beside it."""
    sc = small_scenario(beams, frames)
    sc.timeout = 3
    env, ora = hip["env"].VecStageWorld(sc, lazy_obs=lazy), U.COracleEnv(sc)
    rng = np.random.default_rng(2)
    poses, goals = parity_scene(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    ora.reset(None, poses, goals)
    p, sp = R.params(), SR.params()
    seen = set()
    for k in range(13):                                  # after the reset and after each of 12 ticks
        policy = seeded_commands(rng, env.N)
        wmode, wscale, _pid, _c = check_plan(env, p, sp)
        omode, oscale, _op, _oc = SR.plan(p, sp, ora.local_goal, ora.scan)
        assert np.array_equal(omode, wmode) and np.array_equal(bits(oscale), bits(wscale)), k
        seen |= set(wmode.tolist())
        if k == 12:
            break
        wact = R.env_actions(p, ora.local_goal, policy, ora.scan)[0]
        env.step(dev(wact))
        ora.step(wact)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
    assert seen == {R.AT_GOAL, R.NORMAL, R.SIMPLE, R.EMERGENT}, seen
    env.check()
    env.close()


@pytest.fixture(scope="module")
def moved_env(hip):
    """The small scenario after a teleport and 10 random ticks, host copies of its fields: shared by the tests below."""
    sc = small_scenario(512, 3)
    env = hip["env"].VecStageWorld(sc)
    rng = np.random.default_rng(3)
    poses, goals = parity_scene(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    yield env, host_fields(env)
    env.close()


def test_plan_under_other_parameters(moved_env):
    env, fields = moved_env
    for p, sp in ((R.params(risk_dist=6.0, stop_dist=0.0, safe_scale=1.0), SR.params(scan_scale=0.7, v_cap=0.3)),
                  (R.params(corridor=3.0, look=6.0, risk_dist=0.2, stop_dist=0.1), SR.params(scan_scale=1.0, v_cap=1.0)),
                  (R.params(v_pid=0.3, max_speed=0.2, k_omega=0.0, front_cos=-1.0), SR.params(scan_scale=2.0 ** -20))):
        check_plan(env, p, sp, fields=fields)


def test_plan_with_ring_heads_that_differ(hip):
    sc = small_scenario(512, 3)
    env = hip["env"].VecStageWorld(sc)
    rng = np.random.default_rng(6)
    env.reset()
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    mask = (np.arange(env.N) % 4 == 1).astype(np.uint8)
    env.reset(dev(mask))                                 # a masked reset: these robots start a new history
    env.step(dev(U.random_actions(rng, env.N)), worlds=(0, 1))            # ... and world 0 ticks alone, once more
    torch.cuda.synchronize()
    assert len(set(env.ring_head.cpu().numpy().tolist())) > 1
    check_plan(env, R.params(), SR.params())
    check_plan(env, R.params(risk_dist=2.0, stop_dist=0.5, look=6.0), SR.params(scan_scale=0.5))
    env.close()


def test_plan_on_a_world_of_66_robots(hip):
    env = hip["env"].VecStageWorld(S.circle_big(66))
    env.reset()
    check_plan(env, R.params(), SR.params())
    check_plan(env, R.params(risk_dist=4.0, stop_dist=1.0, corridor=2.0, look=6.0), SR.params())
    env.check()
    env.close()


def test_plan_behind_the_noise_model_reads_the_noisy_row(hip):
    from mrca.noise import ScanNoiseParams
    sc = small_scenario(512, 3)
    env, clean = hip["env"].VecStageWorld(sc), hip["env"].VecStageWorld(sc)
    rng = np.random.default_rng(12)
    poses, goals = parity_scene(sc, rng)
    q = ScanNoiseParams(sigma_const=0.05, sigma_prop=0.02, dropout=0.05, quantum=0.01)
    for e in (env, clean):
        e.reset(None, dev(poses), dev(goals))
    env.scan_noise(q)
    for _ in range(3):
        a = dev(U.random_actions(rng, env.N))
        for e in (env, clean):
            e.step(a)
        env.scan_noise(q)
    (_g, noisy), (_g2, exact) = host_fields(env), host_fields(clean)
    assert not np.array_equal(noisy, exact)
    clear = check_plan(env, R.params(), SR.params())[3]                  # (the reference is fed the ring as read back: the noisy row)
    clear_exact = check_plan(clean, R.params(), SR.params())[3]
    assert not np.array_equal(clear, clear_exact)
    for e in (env, clean):
        e.close()


# ------------------------------------------------------------------------------------------------ the closed loop
def test_the_closed_loop_equals_the_host_chain_and_the_oracle(hip):
    """512 beams, 3 frames, the shipped checkpoint, 12 ticks.  Device: plan -> act_fused(scan_scale) (mean action) -> commit ->
    step.  Host: safe_ref plan -> act_fused WITHOUT a scale on a pre-scaled copy of the ring -> safe_ref commit."""
    from mrca.policy_ops import RingHead
    pol = hip["pol"]
    sc = small_scenario(512, 3)
    sc.timeout = 6
    env, ora = hip["env"].VecStageWorld(sc), U.COracleEnv(sc)
    rng = np.random.default_rng(2)
    poses, goals = parity_scene(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    ora.reset(None, poses, goals)
    p, sp = R.params(), SR.params()
    hp, ssp = hybrid_params(p), safe_params(sp)
    lo, hi = (torch.tensor(b, dtype=torch.float32, device="cuda") for b in ((0.0, -1.0), (1.0, 1.0)))
    scaled_ticks, seen = 0, set()
    for k in range(12):
        mode, scale, pid = env.hybrid_plan(hp, ssp)
        ring, head = env.policy_obs()
        cmd = pol.act_fused(ring, env.local_goal, env.speed, None, lo, hi, head=head, scan_scale=scale)[3]
        act = env.hybrid_commit(cmd.clone(), mode, pid, ssp)
        # the host chain on the fields read back
        goal, rows = host_fields(env)
        wmode, wscale, wpid, _c = SR.plan(p, sp, goal, rows)
        pre = dev(SR.scaled_ring(ring.cpu().numpy(), wscale))
        wcmd = pol.act_fused(pre, env.local_goal, env.speed, None, lo, hi, head=RingHead(head.slots, raw=True))[3]
        want = SR.commit(sp, wmode, wpid, wcmd.cpu().numpy())
        torch.cuda.synchronize()
        assert np.array_equal(mode.cpu().numpy(), wmode) and np.array_equal(bits(scale.cpu().numpy()), bits(wscale)), k
        assert np.array_equal(bits(cmd.cpu().numpy()), bits(wcmd.cpu().numpy())), k          # the forward, robot by robot
        assert np.array_equal(bits(act.cpu().numpy()), bits(want)), (k, np.argwhere(bits(act.cpu().numpy()) != bits(want))[:5])
        scaled_ticks += int(((wmode == R.EMERGENT) & (wscale < 1.0)).any())
        seen |= set(wmode.tolist())
        env.step(act)
        ora.step(want)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
    assert scaled_ticks > 0 and R.EMERGENT in seen and R.NORMAL in seen, (scaled_ticks, seen)
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ masks, in place, capture
def test_masks_and_in_place(moved_env):
    env, fields = moved_env
    p, sp = R.params(), SR.params()
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    check_plan(env, p, sp, mask=mask, fields=fields)                     # (rows with mask 0 keep their patterns exactly)
    check_plan(env, p, sp, mask=mask, fields=fields, with_clear=False)
    check_plan(env, p, sp, mask=np.zeros(env.N, np.uint8), fields=fields)
    hp, ssp = hybrid_params(p), safe_params(sp)
    # complementary masks, one after the other into the same buffers, equal one call
    one, two = sentinels(env), sentinels(env)
    env.hybrid_plan(hp, ssp, mode=one[0], scale=one[1], pid=one[2], clear=one[3])
    for m in (mask, 1 - mask):
        env.hybrid_plan(hp, ssp, mask=dev(m), mode=two[0], scale=two[1], pid=two[2], clear=two[3])
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one, two))
    # fresh outputs of a masked plan: mode 0, scale 1, pid 0 where the mask is 0
    mode, scale, pid = env.hybrid_plan(hp, ssp, mask=dev(mask))
    torch.cuda.synchronize()
    off = dev(mask) == 0
    assert not mode[off].any() and bool((scale[off] == 1).all()) and not pid[off].any()
    # the commit: against the restatement, masked rows keep the sentinel, in place == out of place, complementary masks == one call
    mode, pid = one[0], one[2]
    policy = seeded_commands(np.random.default_rng(5), env.N)
    policy[0], policy[1] = (np.nan, -0.0), (-0.0, np.nan)
    want = SR.commit(sp, mode.cpu().numpy(), pid.cpu().numpy(), policy)
    nan_out = torch.full((env.N, 2), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32)
    out = env.hybrid_commit(dev(policy), mode, pid, ssp, out=nan_out.clone())
    inpl = dev(policy)
    assert env.hybrid_commit(inpl, mode, pid, ssp) is inpl
    part = env.hybrid_commit(dev(policy), mode, pid, ssp, mask=dev(mask), out=nan_out.clone())
    both = env.hybrid_commit(dev(policy), mode, pid, ssp, mask=dev(1 - mask), out=part.clone())
    part_in = env.hybrid_commit(dev(policy), mode, pid, ssp, mask=dev(mask))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(bits(inpl.cpu().numpy()), bits(want))
    sel = mask.astype(bool)[:, None]
    assert np.array_equal(bits(part.cpu().numpy()), np.where(sel, bits(want), np.uint32(NAN_BITS)))
    assert np.array_equal(bits(both.cpu().numpy()), bits(want))
    assert np.array_equal(bits(part_in.cpu().numpy()), np.where(sel, bits(want), bits(policy)))


def test_plan_and_commit_write_nothing_of_the_env(hip):
    sc = small_scenario(512, 3)
    env = hip["env"].VecStageWorld(sc, lazy_obs=False)
    rng = np.random.default_rng(8)
    env.reset()
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    arena = env.arena.clone()
    clear = torch.zeros(env.N, 3, device=env.device)
    mode, scale, pid = env.hybrid_plan(clear=clear)
    env.hybrid_commit(dev(seeded_commands(rng, env.N)), mode, pid)
    torch.cuda.synchronize()
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory
    env.close()


def test_a_captured_tick_replays_as_the_eager_tick(hip):
    """torch.cuda.graph around plan + commit (on a fixed command buffer) + step: 4 replays == 4 eager ticks, bit for bit"""
    sc = small_scenario(512, 3)
    sc.timeout = 3
    graphed, eager = hip["env"].VecStageWorld(sc), hip["env"].VecStageWorld(sc)
    rng = np.random.default_rng(10)
    poses, goals = parity_scene(sc, rng)
    cmds = [dev(seeded_commands(rng, eager.N)) for _ in range(5)]
    a_in, a_out = cmds[0].clone(), torch.zeros(eager.N, 2, device=eager.device)
    mode, scale, pid, _c = sentinels(graphed)
    for e in (graphed, eager):
        e.reset(None, dev(poses), dev(goals))

    def tick():
        graphed.hybrid_plan(mode=mode, scale=scale, pid=pid)
        graphed.step(graphed.hybrid_commit(a_in, mode, pid, out=a_out))

    def eager_tick(cmd):
        m, _s, q = eager.hybrid_plan()
        want = eager.hybrid_commit(cmd.clone(), m, q)
        eager.step(want)
        return want, m
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tick()                                           # warm-up on the capture stream: tick 0
    torch.cuda.current_stream().wait_stream(side)
    eager_tick(cmds[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tick()
    for k in range(1, 5):
        a_in.copy_(cmds[k])
        g.replay()
        want, wmode = eager_tick(cmds[k])
    torch.cuda.synchronize()
    assert torch.equal(a_out.view(torch.int32), want.view(torch.int32)) and torch.equal(mode, wmode)
    assert torch.equal(graphed.arena, eager.arena)
    assert len(set(mode.cpu().numpy().tolist())) > 1
    for e in (graphed, eager):
        e.check()
        e.close()


def test_errors(hip):
    from mrca import _lib
    from mrca.hybrid import HybridParams, SafePolicyParams
    env = hip["env"].VecStageWorld(small_scenario(64, 1))
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    scale = torch.zeros(env.N, device=env.device)
    pid = torch.zeros(env.N, 2, device=env.device)
    pol, out = torch.ones(env.N, 2, device=env.device), torch.zeros(env.N, 2, device=env.device)
    with pytest.raises(RuntimeError, match="before the first mrca_reset"):
        env.hybrid_plan(mode=mode, scale=scale, pid=pid)
    env.reset()
    lib, st = env.lib, env._stream()
    for k, v in [("scan_scale", 0.0), ("scan_scale", 1.5), ("v_cap", 0.0), ("v_cap", 1.5), ("scan_scale", float("nan")), ("v_cap", float("inf"))]:
        s = _lib.SafePolicyParamsStruct()
        lib.mrca_safe_policy_default_params(C.byref(s))
        setattr(s, k, v)
        assert lib.mrca_hybrid_plan(env._h, None, C.byref(s), None, mode.data_ptr(), scale.data_ptr(), pid.data_ptr(), None, st) == -1
        assert k.encode() in lib.mrca_last_error()
        assert lib.mrca_hybrid_commit(env.N, C.byref(s), None, mode.data_ptr(), pid.data_ptr(), pol.data_ptr(), out.data_ptr(), st) == -1
        assert k.encode() in lib.mrca_last_error()
    assert lib.mrca_hybrid_plan(env._h, None, None, None, None, scale.data_ptr(), pid.data_ptr(), None, st) == -1
    assert lib.mrca_hybrid_plan(env._h, None, None, None, mode.data_ptr(), None, pid.data_ptr(), None, st) == -1
    assert lib.mrca_hybrid_plan(env._h, None, None, None, mode.data_ptr(), scale.data_ptr(), None, None, st) == -1
    assert lib.mrca_hybrid_commit(env.N, None, None, mode.data_ptr(), pid.data_ptr(), pol.data_ptr(), out.data_ptr() + 4, st) == -1
    assert lib.mrca_hybrid_commit(env.N, None, None, mode.data_ptr(), pid.data_ptr(), None, out.data_ptr(), st) == -1
    with pytest.raises(RuntimeError):
        env.hybrid_plan(HybridParams(corridor=0.0), mode=mode, scale=scale, pid=pid)
    with pytest.raises(RuntimeError):
        env.hybrid_plan(safe=SafePolicyParams(scan_scale=1.5), mode=mode, scale=scale, pid=pid)
    with pytest.raises(ValueError):
        env.hybrid_plan(mode=torch.zeros(env.N, device=env.device), scale=scale, pid=pid)          # mode must be int32
    with pytest.raises(ValueError):
        env.hybrid_commit(pol, mode, pid[:3])
    env.check()                                          # no HIP error was left behind
    assert not out.any() and not mode.any() and not scale.any() and not pid.any() and bool((pol == 1).all())
    env.close()


def _evaluate(args, ok=True):
    cmd = [sys.executable, "-m", "mrca.evaluate"] + args
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if not ok:
        assert out.returncode != 0 and not out.stdout.strip(), out.stdout[-500:]
        return out.stderr
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_cli_hybrid_safe(hip):
    base = ["--circles", "2", "--policy", CKPT, "--fused", "--max-ticks", "20"]
    out = _evaluate(base + ["--hybrid-safe", "--hybrid-safe-param", "scan_scale=0.7", "--hybrid-param", "risk_dist=0.8"])
    assert out["robots"] == 100 and "mrca_hybrid_plan" in out["policy"]
    assert abs(out["hybrid_safe_params"]["scan_scale"] - 0.7) < 1e-6 and out["hybrid_safe_params"]["v_cap"] == 0.75
    assert out["hybrid_params"]["risk_dist"] == 0.8 and out["hybrid_params"]["look"] == 6.0
    assert set(out["hybrid_modes"]) == {"normal", "simple", "emergent", "at_goal"}
    assert abs(sum(out["hybrid_modes"].values()) - 1.0) < 1e-9 and out["hybrid_modes"]["simple"] > 0
    # refused, with a message: a controller that reads no rescaled scan
    assert "--hybrid-safe" in _evaluate(base + ["--hybrid-safe", "--dwa"], ok=False)
