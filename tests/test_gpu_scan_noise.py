"""GPU: mrca_scan_noise -- the scan ring, the ring heads, the hit plane and the two views EQUAL, bit for bit, to the NumPy
restatement of tests/noise_ref.py applied once behind every cast to the clean rows of the C oracle (small walled worlds with
restarts inside the run: fresh and stale robots in one launch) or of a noise-free twin env (masked resets, world ranges, ray
slices, worlds of more than 64 robots); masks; the call writes the ring, the hit bits and the eager views and nothing else; a
captured tick; ``VecStageWorld(scan_noise=...)``; the trainer under noise; the error returns; ``mrca.evaluate --lidar-noise``."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_ref as R
import util as U
from test_gpu_orca import _evaluate, go_to_goal, small_scenario, teleport_poses
from util import S

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
P = R.params(sigma_const=0.05, sigma_prop=0.02, dropout=0.05, quantum=0.01)       # every part of the rule at work


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


def noise_params(p):
    from mrca.noise import ScanNoiseParams
    return ScanNoiseParams(**{k: float(v) for k, v in p.items()})


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def assert_ring_equal(env, model, what, views=True):
    """ring, heads, hit plane and the two views (raw fields with lazy_obs = 0, mrca_materialize's output otherwise) == model"""
    torch.cuda.synchronize()
    assert np.array_equal(env.ring_head.cpu().numpy(), model.head), (what, env.ring_head.cpu().numpy(), model.head)
    ring = env.scan_ring.cpu().numpy()
    assert np.array_equal(bits(ring), bits(model.ring)), (what, "scan_ring", np.argwhere(bits(ring) != bits(model.ring))[:5])
    words = env.hit_bits.cpu().numpy().view(np.uint64)
    assert np.array_equal(words, model.hit_words()), (what, "hit_bits", np.argwhere(words != model.hit_words())[:5])
    assert not (model.hit & (model.ring >= 6.0)).any(), what           # a set bit never stands on a 6.0
    if views:
        if env._eager_views:
            scan, obs = env._scan.cpu().numpy(), env._obs.cpu().numpy()       # the raw fields, nothing materialised
        else:
            env.invalidate_views()
            scan, obs = env.scan.cpu().numpy(), env.obs.cpu().numpy()
        assert np.array_equal(bits(scan), bits(model.newest())), (what, "scan")
        assert np.array_equal(bits(obs), bits(model.stack())), (what, "obs", np.argwhere(bits(obs) != bits(model.stack()))[:5])


def clean_cast(model, clean, p, robots=None):
    """the model takes the cast `clean` (an oracle env or a noise-free twin, synchronised) has just made"""
    if isinstance(clean, U.COracleEnv):
        rows, hit, fresh, ep, t = clean.scan, clean.hit_robot, clean.fresh, clean.episode, clean.t
    else:
        torch.cuda.synchronize()
        ar = torch.arange(clean.N, device=clean.device)
        rows = clean.scan_ring[ar, clean.ring_head.long()].cpu().numpy()
        hit, fresh = clean.hit_robot.cpu().numpy(), clean.fresh.cpu().numpy()
        ep, t = clean.episode.cpu().numpy(), clean.t.cpu().numpy()
    model.cast(p, rows, hit, fresh, ep, t, robots)


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3), (1024, 2)])
def test_small_worlds_equal_the_oracle_and_the_restatement(hip, beams, frames, lazy):
    """3 worlds x 7 robots = 21 robots: the last workgroup (4 robots each) has three empty waves.  timeout = 3: robots restart
    inside the run, so a launch holds fresh robots (all F slots) beside stale ones (the newest slot)."""
    sc = small_scenario(beams, frames)
    sc.timeout = 3
    env, ora = hip.VecStageWorld(sc, lazy_obs=lazy), U.COracleEnv(sc)
    model = R.RingModel(env.N, frames, beams, sc.seed)
    q = noise_params(P)
    rng = np.random.default_rng(2)
    poses, goals = teleport_poses(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    env.scan_noise(q)
    ora.reset(None, poses, goals)
    clean_cast(model, ora, P)
    assert_ring_equal(env, model, "reset")
    mixed = cleared = False
    for k in range(12):
        a = U.random_actions(rng, env.N)
        env.step(dev(a))
        env.scan_noise(q)
        ora.step(a)
        clean_cast(model, ora, P)
        mixed = mixed or (ora.fresh.any() and not ora.fresh.all())
        cleared = cleared or bool((np.asarray(ora.hit_robot).astype(bool) & (model.newest() >= 6.0)).any())
        U.assert_state_equal(U.HostView(env, fields=["pose", "t", "episode", "done", "local_goal"]), ora,
                             fields=["pose", "t", "episode", "done", "local_goal"], what=f"tick {k}")
        assert np.array_equal(env.fresh.cpu().numpy(), ora.fresh), k
        assert_ring_equal(env, model, f"tick {k}")
    assert mixed                                         # fresh and stale robots in one launch
    assert cleared                                       # a robot's return that the noise took away: its bit went with it
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ masks
def twins(hip, sc, **kw):
    return hip.VecStageWorld(sc, **kw), hip.VecStageWorld(sc, **kw)


def test_masked_reset_then_masked_noise_with_heads_that_differ(hip):
    sc = small_scenario(512, 3)
    env, clean = twins(hip, sc)
    model = R.RingModel(env.N, 3, 512, sc.seed)
    q, rng = noise_params(P), np.random.default_rng(6)
    for e in (env, clean):
        e.reset()
    env.scan_noise(q)
    clean_cast(model, clean, P)
    for _ in range(4):
        a = dev(U.random_actions(rng, env.N))
        for e in (env, clean):
            e.step(a)
        env.scan_noise(q)
        clean_cast(model, clean, P)
    mask = (np.arange(env.N) % 4 == 1).astype(np.uint8)
    for e in (env, clean):
        e.reset(dev(mask))                               # a masked reset: these robots start a new history
    env.scan_noise(q, mask=dev(mask))
    clean_cast(model, clean, P, robots=np.flatnonzero(mask))
    assert_ring_equal(env, model, "masked reset")
    a = dev(U.random_actions(rng, env.N))
    for e in (env, clean):
        e.step(a, worlds=(0, 1))                         # ... and world 0 ticks alone, once more
    first = np.zeros(env.N, np.uint8)
    first[:env.R] = 1
    env.scan_noise(q, mask=dev(first))
    clean_cast(model, clean, P, robots=np.arange(env.R))
    assert len(set(model.head.tolist())) > 1
    assert_ring_equal(env, model, "world 0 alone")
    for e in (env, clean):
        e.close()


@pytest.mark.parametrize("lazy", [True, False])
def test_complementary_masks_equal_one_call(hip, lazy):
    sc = small_scenario(512, 3)
    one, two = twins(hip, sc, lazy_obs=lazy)
    q, rng = noise_params(P), np.random.default_rng(7)
    for e in (one, two):
        e.reset()
    acts = [dev(U.random_actions(rng, one.N)) for _ in range(3)]
    mask = (np.arange(one.N) % 3 != 1).astype(np.uint8)
    for a in acts:
        for e in (one, two):
            e.step(a)
        one.scan_noise(q)
        two.scan_noise(q, mask=dev(1 - mask))
        two.scan_noise(q, mask=dev(mask))
    two.scan_noise(q, mask=dev(np.zeros(one.N, np.uint8)))              # nobody: nothing
    torch.cuda.synchronize()
    # (the raw view fields where the library keeps them; a lazy env has never written them)
    for name in ("scan_ring", "hit_bits", "ring_head", "pose", "t", "episode", "fresh") + (() if lazy else ("_scan", "_obs")):
        assert torch.equal(getattr(one, name), getattr(two, name)), name
    for e in (one, two):
        e.invalidate_views()
    assert torch.equal(one.scan, two.scan) and torch.equal(one.obs, two.obs)
    for e in (one, two):
        e.close()


@pytest.mark.parametrize("lazy", [True, False])
def test_the_call_writes_the_ring_the_hit_bits_and_the_eager_views_only(hip, lazy):
    from mrca import _lib
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc, lazy_obs=lazy)
    rng = np.random.default_rng(8)
    env.reset()
    for _ in range(3):
        env.step(dev(U.random_actions(rng, env.N)))
    torch.cuda.synchronize()
    before = env.arena.clone()
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    env.scan_noise(noise_params(P), mask=dev(mask))
    torch.cuda.synchronize()
    may = torch.zeros_like(env.arena, dtype=torch.bool)
    names = [n for n, _d, _s in _lib.FIELDS]
    for name in ["scan_ring", "hit_bits"] + ([] if lazy else ["scan", "obs"]):
        off, nb = C.c_size_t(), C.c_size_t()
        assert env.lib.mrca_get_field(env._h, names.index(name), None, C.byref(off), C.byref(nb)) == 0
        may[off.value: off.value + nb.value] = True
    changed = env.arena != before
    assert bool(changed.any()) and not bool((changed & ~may).any())      # every other field, and the rest of the arena
    keep = torch.from_numpy(mask == 0).cuda()                            # ... and the rows of the robots the mask leaves out
    other = hip.VecStageWorld(sc, lazy_obs=lazy)                         # the same fields of the arena as it was before
    other.arena.copy_(before)
    for name in ("scan_ring", "hit_bits", "_scan", "_obs"):
        assert torch.equal(getattr(env, name)[keep], getattr(other, name)[keep]), name
    assert not torch.equal(env.scan_ring[~keep], other.scan_ring[~keep])
    other.close()
    env.close()


# ------------------------------------------------------------------------------------------------ worlds of more than 64 robots
def test_worlds_of_more_than_64_robots(hip):
    q = noise_params(P)
    sc = S.circle_big(66)
    env, clean = twins(hip, sc)
    model = R.RingModel(env.N, env.F, env.B, sc.seed)
    for e in (env, clean):
        e.reset()
    env.scan_noise(q)
    clean_cast(model, clean, P)
    assert_ring_equal(env, model, "66 robots")
    for e in (env, clean):
        e.check()
        e.close()
    sc = S.circle_big(500)
    env, clean = twins(hip, sc)
    model = R.RingModel(env.N, env.F, env.B, sc.seed)
    for e in (env, clean):
        e.reset()
    env.scan_noise(q)
    clean_cast(model, clean, P)
    for _ in range(5):
        torch.cuda.synchronize()
        a = dev(go_to_goal(clean.local_goal.cpu().numpy()))
        for e in (env, clean):
            e.step(a)
        env.scan_noise(q)
        clean_cast(model, clean, P)
    assert model.hit.any()                               # neighbours are seen
    assert_ring_equal(env, model, "500 robots")
    for e in (env, clean):
        e.check()
        e.close()


# ------------------------------------------------------------------------------------------------ the env applies it itself
def test_env_with_scan_noise_applies_it_once_per_cast(hip):
    """reset, step, reset(mask), step(worlds=), observe, step(ray_slice=): the noise goes to exactly the robots that call cast"""
    sc = small_scenario(512, 3)
    env, clean = hip.VecStageWorld(sc, scan_noise=noise_params(P)), hip.VecStageWorld(sc)
    model = R.RingModel(env.N, 3, 512, sc.seed)
    rng = np.random.default_rng(9)
    Rn = env.R

    def both(call, robots=None, what=""):
        for e in (env, clean):
            call(e)
        clean_cast(model, clean, P, robots)
        assert_ring_equal(env, model, what)

    both(lambda e: e.reset(), what="reset")
    for k in range(3):
        a = dev(U.random_actions(rng, env.N))
        both(lambda e: e.step(a), what=f"step {k}")
    mask = (np.arange(env.N) % 4 == 2).astype(np.uint8)
    m = dev(mask)
    both(lambda e: e.reset(m), np.flatnonzero(mask), "reset(mask)")
    a = dev(U.random_actions(rng, env.N))
    both(lambda e: e.step(a, worlds=(1, 2)), np.arange(Rn, 3 * Rn), "step(worlds=)")
    a = dev(U.random_actions(rng, env.N))
    both(lambda e: e.move(a, (0, 1)).observe((0, 1)), np.arange(0, Rn), "move + observe")
    a = dev(U.random_actions(rng, env.N))
    both(lambda e: e.step(a, ray_slice=(3, 5)), np.arange(3, 8), "step(ray_slice=)")
    with pytest.raises(ValueError, match="scan_noise"):
        env.step_many([a], 0, 2)
    for e in (env, clean):
        e.check()
        e.close()


def test_a_captured_tick_replays_as_the_eager_tick(hip):
    """torch.cuda.graph around step + noise: 4 replays == 4 eager ticks, bit for bit, the whole arena"""
    sc = small_scenario(512, 3)
    sc.timeout = 3
    q = noise_params(P)
    graphed, eager = twins(hip, sc, scan_noise=q)
    rng = np.random.default_rng(10)
    acts = [dev(U.random_actions(rng, eager.N)) for _ in range(5)]
    a = acts[0].clone()
    for e in (graphed, eager):
        e.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step(a)                                  # warm-up on the capture stream: tick 0
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.step(a)
    for k in range(1, 5):
        a.copy_(acts[k])
        g.replay()
        eager.step(acts[k])
    torch.cuda.synchronize()
    graphed.invalidate_views()
    assert torch.equal(graphed.scan_ring, eager.scan_ring) and torch.equal(graphed.hit_bits, eager.hit_bits)
    assert torch.equal(graphed.ring_head, eager.ring_head) and torch.equal(graphed.obs, eager.obs)
    clean = hip.VecStageWorld(sc)
    clean.reset()
    for k in range(5):
        clean.step(acts[k])
    torch.cuda.synchronize()
    assert torch.equal(clean.pose, eager.pose) and not torch.equal(clean.scan_ring, eager.scan_ring)
    for e in (graphed, eager, clean):
        e.check()
        e.close()


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_under_noise_stores_and_reads_the_noisy_rows(hip):
    """Two horizons of 4 ticks (an update between them).  A noise-free twin replays the stored actions, clipped; the model's
    noisy ring is what the env holds at every tick, the buffer's stored stacks are x / 6 - 0.5 of its rows, the fused
    inference is handed the ring itself and the stored value is the policy's on the noisy stack."""
    from mrca import ppo
    from mrca.trainer import HParams, Stage1Trainer
    sc = S.stage1(num_worlds=3, robots_per_world=7, seed=2)
    env, clean = hip.VecStageWorld(sc, scan_noise=noise_params(P)), hip.VecStageWorld(sc)
    model = R.RingModel(env.N, env.F, env.B, sc.seed)
    hp = HParams(horizon=4, batch_size=28, epoch=1, rollout_fused=True)
    tr = Stage1Trainer(env, hp=hp, seed=5)
    tr.start()
    clean.reset()
    clean_cast(model, clean, P)
    assert_ring_equal(env, model, "start", views=False)
    obs, head = ppo.policy_input(env, True)
    assert obs.data_ptr() == env.scan_ring.data_ptr()    # act_fused reads the ring in place
    lo, hi = torch.tensor([0.0, -1.0], device="cuda"), torch.tensor([1.0, 1.0], device="cuda")
    for k in range(8):
        t = k % 4
        stack = model.stack()
        with torch.no_grad():
            _m, v = tr.policy.mean_value(dev(stack), env.local_goal, env.speed)
        tr.tick()
        torch.cuda.synchronize()
        got = tr.buffer.obs_rows().materialise()[t].cpu().numpy()
        assert np.array_equal(bits(got), bits(stack)), (k, np.argwhere(bits(got) != bits(stack))[:5])
        assert torch.allclose(tr.buffer.value[t].reshape(-1), v.reshape(-1), atol=1e-4, rtol=1e-4), k
        clean.step(torch.minimum(torch.maximum(tr.buffer.action[t], lo), hi).contiguous())
        clean_cast(model, clean, P)
        assert_ring_equal(env, model, f"tick {k}", views=False)
    assert tr.global_update == 2
    ret = model.ring[model.ring < 6.0]
    assert np.array_equal(bits(ret), bits(f32(0.01) * np.rint(ret / f32(0.01))))       # every return sits on the read-out grid
    for e in (env, clean):
        e.check()
        e.close()


# ------------------------------------------------------------------------------------------------ errors, the command line
def test_errors(hip):
    from mrca import _lib
    from mrca.noise import ScanNoiseParams
    sc = small_scenario(64, 1)
    env = hip.VecStageWorld(sc)
    st = ScanNoiseParams().struct()
    assert env.lib.mrca_scan_noise(env._h, C.byref(st), None, env._stream()) == -1       # before the first reset
    assert b"mrca_reset" in env.lib.mrca_last_error()
    with pytest.raises(RuntimeError, match="mrca_reset"):
        env.scan_noise()
    env.reset()
    torch.cuda.synchronize()
    before = env.arena.clone()
    bad = [("sigma_const", -0.01), ("sigma_const", 6.5), ("sigma_prop", -0.01), ("sigma_prop", 1.5), ("dropout", -0.1), ("dropout", 1.01),
           ("quantum", -0.01), ("quantum", 1.5)]
    bad += [(k, v) for k in R.FIELDS for v in (float("nan"), float("inf"))]
    for k, v in bad:
        st = _lib.ScanNoiseParamsStruct()
        env.lib.mrca_scan_noise_default_params(C.byref(st))
        setattr(st, k, v)
        rc = env.lib.mrca_scan_noise(env._h, C.byref(st), None, env._stream())
        assert rc == -1 and k.encode() in env.lib.mrca_last_error(), (k, v, env.lib.mrca_last_error())
    with pytest.raises(RuntimeError):
        env.scan_noise(ScanNoiseParams(dropout=2.0))
    with pytest.raises(ValueError):
        env.scan_noise(mask=torch.zeros(env.N, device=env.device))      # the mask must be uint8
    zero = _lib.ScanNoiseParamsStruct()
    assert env.lib.mrca_scan_noise(env._h, C.byref(zero), None, env._stream()) == 0      # all zero: MRCA_OK, no launch
    env.check()                                          # no HIP error was left behind
    assert torch.equal(before, env.arena)
    assert env.lib.mrca_scan_noise(env._h, None, None, env._stream()) == 0               # NULL: the defaults
    torch.cuda.synchronize()
    assert not torch.equal(before, env.arena)
    env.check()
    env.close()


def test_cli_lidar_noise(hip):
    out = _evaluate(["--circles", "2", "--robots", "10", "--radius", "8", "--max-ticks", "50", "--dwa", "--lidar-noise", "const=0.05"])
    assert out["robots"] == 20 and "DWA" in out["policy"]
    assert out["lidar_noise"] == dict(sigma_const=0.05, sigma_prop=0.0, dropout=0.0, quantum=0.0)
