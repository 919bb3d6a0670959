"""GPU: mrca_hybrid_actions -- command, mode and the three clearances EQUAL, bit for bit, to the NumPy float32 restatement of
tests/hybrid_ref.py fed with the fields read back, for EVERY robot: small walled worlds driven beside the C oracle (every mode
occurs), ring heads that differ, masks, in place and out of place, worlds of more than 64 robots, behind mrca_scan_noise, in a
captured tick; the call writes nothing of the env; the error returns; ``mrca.evaluate --hybrid``.

The crafted cases -- every edge of the rule, and the inputs at which the kernel's own glue can go wrong (the deal of beams to
lanes in rounds of 64, the butterfly merge of minima and counts, the early exits, the lane-0 epilogue) -- live in
tests/hybrid_cases.py, shared with tests/test_hybrid_host.py; tests/controller_inject.py writes them into an env, one case per
robot, and ``test_crafted_cases_on_the_device`` asserts from the fields read back that each case stood on its edge."""
import ctypes as C

import numpy as np
import pytest
import torch

import controller_inject as J
import hybrid_cases as K
import hybrid_ref as R
import util as U
from test_gpu_orca import NAN_BITS, _evaluate, go_to_goal, nan_filled, small_scenario, teleport_poses
from util import S

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_SENTINEL = 12345


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


def hybrid_params(p):
    from mrca.hybrid import HybridParams
    return HybridParams(**{k: float(v) for k, v in p.items()})


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def host_fields(env):
    """Host copies of what the call reads of the env: (local_goal, newest scan rows)."""
    torch.cuda.synchronize()
    rows = env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()]
    return env.local_goal.cpu().numpy(), rows.cpu().numpy()


def seeded_commands(rng, n):
    """an incoming command per robot: v in [0, 1], omega in [-1, 1]"""
    return np.stack([rng.uniform(0, 1, n), rng.uniform(-1, 1, n)], 1).astype(f32)


def parity_scene(sc, rng):
    """``teleport_poses`` (two robots on one spot, one 0.3 m from another, one 0.6 m from a wall: mode 2) with robot 4 of every
    world 0.2 m from its goal (mode -2) and robot 6 looking at its goal 3 m ahead (mode 1 where nothing stands in between)."""
    poses, goals = teleport_poses(sc, rng)
    Rn = sc.robots_per_world
    for w in range(sc.num_worlds):
        goals[w * Rn + 4] = poses[w * Rn + 4, :2] + f32(0.2)
        th = poses[w * Rn + 6, 2]
        goals[w * Rn + 6] = poses[w * Rn + 6, :2] + f32(3.0) * np.array([np.cos(th), np.sin(th)], f32)
    return poses, goals


def check_equal(env, p, policy, mask=None, with_extras=True, in_place=False, fields=None, goal_dev=None, full=False):
    """One call compared with hybrid_ref on the same fields, every robot -> (the reference's actions, modes, clearances), with
    ``full`` also its blocking counts.  ``goal_dev``: a float32[N,2] tensor that goes in through mrca_hybrid_actions_goal; the
    reference is then fed with a host copy of it in place of ``local_goal``."""
    goal, rows = fields or host_fields(env)
    if goal_dev is not None:
        goal = goal_dev.cpu().numpy()
    policy = np.ascontiguousarray(policy, f32)
    mode = torch.full((env.N,), MODE_SENTINEL, dtype=torch.int32, device=env.device) if with_extras else None
    clear = torch.full((env.N, 3), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32) if with_extras else None
    m = None if mask is None else dev(np.ascontiguousarray(mask, np.uint8))
    if in_place:
        act = dev(policy)
        got = env.hybrid_actions(act, hybrid_params(p), mask=m, mode=mode, clear=clear, goal=goal_dev)
        untouched = bits(policy)
    else:
        act, pol = nan_filled(env), dev(policy)
        got = env.hybrid_actions(pol, hybrid_params(p), mask=m, out=act, mode=mode, clear=clear, goal=goal_dev)
        untouched = np.full((env.N, 2), NAN_BITS, np.uint32)
    assert got is act
    wact, wmode, wclear, nb = R.env_actions(p, goal, policy, rows)
    sel = np.ones(env.N, bool) if mask is None else np.asarray(mask).astype(bool)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(bits(pol.cpu().numpy()), bits(policy))      # the incoming command is read, not written
    a = bits(act.cpu().numpy())
    want_a = np.where(sel[:, None], bits(wact), untouched)
    assert np.array_equal(a, want_a), (np.argwhere(a != want_a)[:5], act.cpu().numpy()[:8], wact[:8])
    if with_extras:
        assert np.array_equal(mode.cpu().numpy(), np.where(sel, wmode, MODE_SENTINEL)), (mode.cpu().numpy(), wmode)
        c = bits(clear.cpu().numpy())
        want_c = np.where(sel[:, None], bits(wclear), np.uint32(NAN_BITS))
        assert np.array_equal(c, want_c), (np.argwhere(c != want_c)[:5], clear.cpu().numpy()[:8], wclear[:8])
    return (wact, wmode, wclear, nb) if full else (wact, wmode, wclear)


# ------------------------------------------------------------------------------------------------ the crafted cases, on the device
@pytest.mark.parametrize("beams", [64, 192, 1024])
def test_crafted_cases_on_the_device(hip, beams):
    """``hybrid_cases.device_cases`` -- every edge of the host test's crafted rows rebuilt on the env's own beam table, lone
    returns on the first and the last lane of the first and the last round, a row in which all B beams block, ranges of 0.0 and
    -0.0, NaN / Inf / -0.0 commands in every mode -- written into an env one case per robot: out of place, in place, under a
    mask, and with the goals handed to mrca_hybrid_actions_goal while ``local_goal`` holds something else.  That each row stood
    on its edge is asserted from the fields read back."""
    names, goal, policy, rows = K.device_cases(beams)
    env = J.walled_env(hip, beams, len(names))
    J.write_cases(env, 0, local_goal=goal, rows=rows)
    assert J.heads_differ(env)
    rng = np.random.default_rng(beams)
    pol = seeded_commands(rng, env.N)
    pol[:len(names)] = policy
    p = R.params(**K.PARAMS)
    goals = env.local_goal.clone()
    for goal_dev in (None, goals):
        if goal_dev is not None:
            env.local_goal[:] = dev(rng.uniform(-5.0, 5.0, (env.N, 2)).astype(f32))
        for in_place in (False, True):
            act, mode, clear, nb = check_equal(env, p, pol, in_place=in_place, goal_dev=goal_dev, full=True)
            K.expectations(names, p, pol, host_fields(env)[1], act, mode, clear, nb)
            mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
            check_equal(env, p, pol, mask=mask, in_place=in_place, goal_dev=goal_dev)
        check_equal(env, R.params(), pol, goal_dev=goal_dev)             # (the same rows off their edges, under the defaults)
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ parity beside the oracle
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("beams,frames", [(64, 1), (512, 3), (1024, 2)])
def test_small_worlds_equal_the_oracle_and_the_restatement(hip, beams, frames, lazy):
    """3 worlds x 7 robots = 21 robots: the last workgroup (4 robots each) has three empty waves.  timeout = 3: robots restart
    inside the run.  The env is driven by the call's own output, the C oracle by the restatement's: they stay equal, and over
    the run every mode occurs (scene and seed were chosen on the CPU with the oracle; the rule reads only fields the oracle
    reproduces to the bit)."""
    sc = small_scenario(beams, frames)
    sc.timeout = 3
    env, ora = hip.VecStageWorld(sc, lazy_obs=lazy), U.COracleEnv(sc)
    rng = np.random.default_rng(2)
    poses, goals = parity_scene(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    ora.reset(None, poses, goals)
    p = R.params()
    seen = set()
    for k in range(13):                                  # after the reset and after each of 12 ticks
        policy = seeded_commands(rng, env.N)
        wact, wmode, _c = check_equal(env, p, policy, in_place=bool(k & 1))
        oact, omode, _oc, _n = R.env_actions(p, ora.local_goal, policy, ora.scan)
        assert np.array_equal(bits(oact), bits(wact)) and np.array_equal(omode, wmode), k
        seen |= set(wmode.tolist())
        if k == 12:
            break
        env.step(dev(wact))
        ora.step(wact)
        U.assert_state_equal(U.HostView(env), ora, what=f"tick {k}")
        U.assert_hits_equal(env, ora, what=f"tick {k}")
    assert seen == {R.AT_GOAL, R.NORMAL, R.SIMPLE, R.EMERGENT}, seen
    env.check()
    env.close()


@pytest.fixture(scope="module")
def moved_env(hip):
    """The small scenario after a teleport and 10 random ticks, host copies of its fields and a command: shared by the tests below."""
    sc = small_scenario(512, 3)
    env = hip.VecStageWorld(sc)
    rng = np.random.default_rng(3)
    poses, goals = parity_scene(sc, rng)
    env.reset(None, dev(poses), dev(goals))
    for _ in range(10):
        env.step(dev(U.random_actions(rng, env.N)))
    yield env, host_fields(env), seeded_commands(rng, env.N)
    env.close()


def test_other_parameters(moved_env):
    env, fields, policy = moved_env
    for p in (R.params(risk_dist=6.0, stop_dist=0.0, safe_scale=1.0), R.params(corridor=3.0, look=6.0, risk_dist=0.2, stop_dist=0.1),
              R.params(front_cos=1.0, safe_scale=0.0), R.params(v_pid=0.3, max_speed=0.2, k_omega=0.0, front_cos=-1.0)):
        check_equal(env, p, policy, fields=fields)


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
    check_equal(env, R.params(), seeded_commands(rng, env.N))
    check_equal(env, R.params(risk_dist=2.0, stop_dist=0.5, look=6.0), seeded_commands(rng, env.N))
    env.close()


def test_masks_extras_and_in_place(moved_env):
    env, fields, policy = moved_env
    p = R.params()
    mask = (np.arange(env.N) % 3 != 1).astype(np.uint8)
    for in_place in (False, True):
        check_equal(env, p, policy, mask=mask, fields=fields, in_place=in_place)          # (rows with mask 0 keep their patterns exactly)
        check_equal(env, p, policy, mask=mask, with_extras=False, fields=fields, in_place=in_place)
        check_equal(env, p, policy, with_extras=False, fields=fields, in_place=in_place)
        check_equal(env, p, policy, mask=np.zeros(env.N, np.uint8), fields=fields, in_place=in_place)
    # complementary masks, one after the other into the same buffers, equal one call
    q = hybrid_params(p)
    one, two = nan_filled(env), nan_filled(env)
    mode1, mode2 = (torch.full((env.N,), MODE_SENTINEL, dtype=torch.int32, device=env.device) for _ in range(2))
    clear1, clear2 = (torch.full((env.N, 3), NAN_BITS, dtype=torch.int32, device=env.device).view(torch.float32) for _ in range(2))
    pol = dev(policy)
    env.hybrid_actions(pol, q, out=one, mode=mode1, clear=clear1)
    env.hybrid_actions(pol, q, mask=dev(mask), out=two, mode=mode2, clear=clear2)
    env.hybrid_actions(pol, q, mask=dev(1 - mask), out=two, mode=mode2, clear=clear2)
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)) and torch.equal(mode1, mode2)
    assert torch.equal(clear1.view(torch.int32), clear2.view(torch.int32))
    # out is actions == out given separately
    inpl = pol.clone()
    assert env.hybrid_actions(inpl, q) is inpl
    torch.cuda.synchronize()
    assert torch.equal(inpl.view(torch.int32), one.view(torch.int32))


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
    env.hybrid_actions(dev(seeded_commands(rng, env.N)), mode=torch.zeros(env.N, dtype=torch.int32, device=env.device),
                       clear=torch.zeros(env.N, 3, device=env.device))
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k], getattr(env, k)), k
    assert torch.equal(arena, env.arena)                 # not a byte of the env's memory
    env.close()


def test_worlds_of_more_than_64_robots(hip):
    rng = np.random.default_rng(9)
    env = hip.VecStageWorld(S.circle_big(66))
    env.reset()
    check_equal(env, R.params(), seeded_commands(rng, env.N))
    env.check()
    env.close()
    env = hip.VecStageWorld(S.circle_big(500))
    env.reset()
    for _ in range(5):
        torch.cuda.synchronize()
        env.step(dev(go_to_goal(env.local_goal.cpu().numpy())))
    _a, mode, clear = check_equal(env, R.params(), seeded_commands(rng, env.N))
    assert (clear[:, 0] < 6.0).any()                     # neighbours are seen
    check_equal(env, R.params(risk_dist=4.0, stop_dist=1.0, corridor=2.0, look=6.0), seeded_commands(rng, env.N), in_place=True)
    env.check()
    env.close()


def test_behind_the_noise_model_the_call_reads_the_noisy_row(hip):
    from mrca.noise import ScanNoiseParams
    sc = small_scenario(512, 3)
    env, clean = hip.VecStageWorld(sc), hip.VecStageWorld(sc)
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
    policy = seeded_commands(rng, env.N)
    _a, _m, clear = check_equal(env, R.params(), policy)                 # (the reference is fed the ring as read back: the noisy row)
    _a, _m, clear_exact = check_equal(clean, R.params(), policy)
    assert not np.array_equal(clear, clear_exact)
    for e in (env, clean):
        e.close()


def test_a_captured_tick_replays_as_the_eager_tick(hip):
    """torch.cuda.graph around hybrid + step: 4 replays == 4 eager ticks, bit for bit, commands and the whole arena"""
    sc = small_scenario(512, 3)
    sc.timeout = 3
    graphed, eager = hip.VecStageWorld(sc), hip.VecStageWorld(sc)
    rng = np.random.default_rng(10)
    poses, goals = parity_scene(sc, rng)
    cmds = [dev(seeded_commands(rng, eager.N)) for _ in range(5)]
    a_in, a_out = cmds[0].clone(), torch.zeros(eager.N, 2, device=eager.device)
    mode = torch.zeros(eager.N, dtype=torch.int32, device=eager.device)
    for e in (graphed, eager):
        e.reset(None, dev(poses), dev(goals))

    def tick():
        graphed.step(graphed.hybrid_actions(a_in, out=a_out, mode=mode))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tick()                                           # warm-up on the capture stream: tick 0
    torch.cuda.current_stream().wait_stream(side)
    want = eager.hybrid_actions(cmds[0].clone())
    eager.step(want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tick()
    for k in range(1, 5):
        a_in.copy_(cmds[k])
        g.replay()
        want = eager.hybrid_actions(cmds[k].clone())
        eager.step(want)
    torch.cuda.synchronize()
    assert torch.equal(a_out.view(torch.int32), want.view(torch.int32))
    assert torch.equal(graphed.arena, eager.arena)
    assert len(set(mode.cpu().numpy().tolist())) > 1
    for e in (graphed, eager):
        e.check()
        e.close()


def test_errors(hip):
    from mrca import _lib
    from mrca.hybrid import HybridParams
    env = hip.VecStageWorld(small_scenario(64, 1))
    out = torch.zeros(env.N, 2, device=env.device)
    pol = torch.ones(env.N, 2, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    with pytest.raises(RuntimeError, match="before the first mrca_reset"):
        env.hybrid_actions(pol, out=out)
    env.reset()
    bad = [("stop_dist", -0.1), ("stop_dist", 0.6), ("risk_dist", 6.5), ("safe_scale", -0.1), ("safe_scale", 1.1), ("corridor", 0.0),
           ("look", 0.0), ("look", 6.5), ("front_cos", -1.1), ("front_cos", 1.1), ("v_pid", 0.0), ("max_speed", 0.0),
           ("max_speed", 1.5), ("k_omega", -1.0)]
    bad += [(k, v) for k in R.FIELDS for v in (float("nan"), float("inf"))]
    for k, v in bad:
        st = _lib.HybridParamsStruct()
        env.lib.mrca_hybrid_default_params(C.byref(st))
        setattr(st, k, v)
        rc = env.lib.mrca_hybrid_actions(env._h, C.byref(st), None, pol.data_ptr(), out.data_ptr(), mode.data_ptr(), None, env._stream())
        assert rc == -1 and k.encode() in env.lib.mrca_last_error(), (k, v, env.lib.mrca_last_error())
    assert env.lib.mrca_hybrid_actions(env._h, None, None, pol.data_ptr(), None, None, None, env._stream()) == -1
    assert env.lib.mrca_hybrid_actions(env._h, None, None, None, out.data_ptr(), None, None, env._stream()) == -1
    assert env.lib.mrca_hybrid_actions(env._h, None, None, pol.data_ptr(), out.data_ptr() + 4, None, None, env._stream()) == -1
    with pytest.raises(RuntimeError):
        env.hybrid_actions(pol, HybridParams(corridor=0.0), out=out)
    with pytest.raises(ValueError):
        env.hybrid_actions(pol, out=out, mode=torch.zeros(env.N, device=env.device))           # mode must be int32
    env.check()                                          # no HIP error was left behind
    assert not out.any() and not mode.any() and bool((pol == 1).all())
    env.close()


def test_cli_hybrid(hip):
    out = _evaluate(["--circles", "2", "--hybrid", "--max-ticks", "20", "--hybrid-param", "risk_dist=0.8"])
    assert out["robots"] == 100 and "hybrid control" in out["policy"]
    assert out["hybrid_params"]["risk_dist"] == 0.8 and out["hybrid_params"]["look"] == 6.0
    assert set(out["hybrid_modes"]) == {"normal", "simple", "emergent", "at_goal"}
    assert abs(sum(out["hybrid_modes"].values()) - 1.0) < 1e-9 and out["hybrid_modes"]["simple"] > 0
