"""Every ray-cast variant a config can select in the product library, against the C oracle (run with -m gpu on an MI355X).

launch_raycast (csrc/mrca_kernels.hip) picks a raycast_kernel instantiation (ray_shape, csrc/mrca_ray_shape.h) from three
properties of the config: the beams a marching thread owns (product_ray_shift: 1, 2 or -- big worlds -- 4), the lidar family
(exact rectangles, the raster lidar with a 4-cell or an 8-cell outline window, worlds of more than 64 robots) and whether the
epilogue forms MRCA_F_SCAN / MRCA_F_OBS itself (lazy_obs = 0).  Nine families times two epilogues are reachable without a
profiling switch; SHAPES below holds one small env or more for each, ``selection`` restates the dispatch rules so that a change
of them says which family lost its shape (test_the_shapes_cover_every_family: no GPU needed; tests/test_ray_shape_host.py holds
the restatement against the header itself), and every shape runs lazy and eager against tests/util.COracleEnv, every field bit
for bit.  An eager env is read through its RAW fields (``_scan`` / ``_obs``: no
mrca_materialize call), so what is compared is what the epilogue stored.

The further tests drive a lazy and an eager HIP env side by side through the calls beyond mrca_step that form the views too:
masked resets, world ranges, the sharded tick of a big world, mrca_step_many and a captured tick.

The seeds below were chosen on the CPU with the C oracle: every run restarts a robot, returns a beam from another robot and --
the raster shapes -- crashes two robots into each other, which each case asserts from the oracle's own run."""
import types

import numpy as np
import pytest
import torch

import util as U
from util import S

gpu = pytest.mark.gpu

FAMILIES = {("exact", 1), ("exact", 2), ("raster4", 1), ("raster4", 2), ("raster8", 1), ("raster8", 2),
            ("big", 1), ("big", 2), ("big", 4)}


def _shape(make, beams, frames, selects, raster=None, ticks=60, action_seed=1):
    return dict(make=make, beams=beams, frames=frames, selects=selects, raster=raster, ticks=ticks, action_seed=action_seed)


# name -> scenario, beams / frames, the (family, beams per thread) it is here for
SHAPES = {
    "exact_k1_one_wave": _shape(lambda: S.stage1(num_worlds=3, robots_per_world=5, seed=21), 64, 1, ("exact", 1)),
    "exact_k1_five_waves": _shape(lambda: S.stage1(num_worlds=2, robots_per_world=8, seed=22), 320, 4, ("exact", 1)),
    # (test_gpu_parity.test_stage2_bit_exact_group_episodes' run: group restarts)
    "exact_k2_stage2": _shape(lambda: S.stage2(num_worlds=1, seed=5), 512, 3, ("exact", 2), ticks=215, action_seed=3),
    "exact_k2_full_wave": _shape(lambda: S.stage1(num_worlds=1, robots_per_world=64, seed=23), 1024, 8, ("exact", 2)),
    "raster4_k2": _shape(lambda: S.stage1(num_worlds=4, robots_per_world=8, seed=24, stage_resolution=True), 512, 3,
                         ("raster4", 2)),
    "raster4_k1": _shape(lambda: S.stage1(num_worlds=3, robots_per_world=8, seed=25, stage_resolution=True), 128, 2,
                         ("raster4", 1)),
    # (the raster-8 shapes keep the 0.05 m map: the raster is aligned at the world's origin, whatever the map's cell)
    "raster8_k2": _shape(lambda: S.stage1(num_worlds=2, robots_per_world=24, seed=26), 512, 3, ("raster8", 2), raster=0.1),
    "raster8_k1": _shape(lambda: S.stage1(num_worlds=3, robots_per_world=8, seed=27), 192, 3, ("raster8", 1), raster=0.13),
    # (these actions restart a group of four at tick 46)
    "raster8_stage2": _shape(lambda: S.stage2(num_worlds=1, seed=28), 512, 3, ("raster8", 2), raster=0.1, action_seed=2),
    "big_k4": _shape(lambda: S.stage1(num_worlds=1, robots_per_world=200, seed=29), 512, 3, ("big", 4)),
    "big_k2": _shape(lambda: S.stage1(num_worlds=1, robots_per_world=80, seed=30), 256, 2, ("big", 2)),
    "big_k1": _shape(lambda: S.stage1(num_worlds=2, robots_per_world=66, seed=31), 128, 5, ("big", 1)),
}


def scenario(name):
    sh = SHAPES[name]
    sc = sh["make"]()
    sc.beams, sc.frames = sh["beams"], sh["frames"]
    if sh["raster"] is not None:
        sc.collision_raster = sh["raster"]
    return sc


# ------------------------------------------------------------------------------------------------ the dispatch rules, restated
def product_ray_shift(beams, big):
    """csrc/mrca_ray_shape.h: log2 of the beams per marching thread"""
    if big and (beams >> 2) >= 128 and (beams >> 2) % 64 == 0:
        return 2
    return 1 if beams >= 256 and (beams >> 1) % 64 == 0 else 0


def outline_span(inv_res):
    """csrc/mrca_device.h: raster cells an outline can span along an axis (fp32, as the library computes it)"""
    f = np.float32
    return int(np.floor((f(0.2907) + f(0.2927) + f(0.002)) * f(inv_res))) + 2


def selection(sc):
    """(family, beams per thread) of the raycast_kernel instantiation ray_shape (csrc/mrca_ray_shape.h) picks for ``sc``"""
    big = sc.robots_per_world > 64
    shift = product_ray_shift(sc.beams, big)
    raster = np.float32(getattr(sc, "collision_raster", 0.0))
    if big:
        return "big", 1 << shift
    if raster > 0:
        window = 4 if outline_span(np.float32(1.0) / raster) <= 4 else 8
        return f"raster{window}", 1 if shift == 0 else 2      # (fidelity mode launches 1 or 2 beams per thread only)
    return "exact", 1 << shift


def test_the_shapes_cover_every_family():
    got = {name: selection(scenario(name)) for name in SHAPES}
    for name, sh in SHAPES.items():
        assert got[name] == sh["selects"], f"{name} is here for {sh['selects']} and now selects {got[name]}"
    missing = FAMILIES - set(got.values())
    assert not missing, f"no shape selects {sorted(missing)}"
    assert len(SHAPES) == 12
    # the rules themselves at their edges
    assert [product_ray_shift(b, 0) for b in (64, 128, 192, 256, 320, 384, 448, 512, 1024)] == [0, 0, 0, 1, 0, 1, 0, 1, 1]
    assert [product_ray_shift(b, 1) for b in (128, 256, 448, 512, 768, 1024)] == [0, 1, 0, 2, 2, 2]
    assert [outline_span(1.0 / r) <= 4 for r in (0.1, 0.13, 0.19, 0.2, 0.25)] == [False, False, False, True, True]
    assert outline_span(1.0 / 0.1) <= 8


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


class RawView:
    """Host copy of an env's state.  ``eager``: scan / obs from the raw fields (what the library itself stored: no
    materialize call); otherwise through the properties (formed from the ring on demand)."""

    def __init__(self, env, eager):
        for k in U.STATE_FIELDS:
            t = getattr(env, "_" + k) if eager and k in ("scan", "obs") else getattr(env, k)
            setattr(self, k, t.cpu().numpy())


def host_copy(ora):
    snap = types.SimpleNamespace(**{k: np.array(getattr(ora, k)) for k in U.STATE_FIELDS})
    snap.hit_robot = np.array(ora.hit_robot)
    return snap


def compare(env, eager, want, what):
    torch.cuda.synchronize()
    U.assert_state_equal(RawView(env, eager), want, what=what)
    U.assert_hits_equal(env, want, what=what)


_oracle_runs = {}


def oracle_run(name):
    """The C oracle's run of a shape, computed once: its actions, its state after the reset (tick -1), after every 4th tick
    and after the last one, and what happened on the way."""
    if name not in _oracle_runs:
        sc = scenario(name)
        sh = SHAPES[name]
        ora = U.COracleEnv(sc)
        ora.reset()
        rng = np.random.default_rng(sh["action_seed"])
        run = types.SimpleNamespace(actions=[], snaps={-1: host_copy(ora)}, hit=False, robot_crash=False, episodes=0)
        for k in range(sh["ticks"]):
            a = U.random_actions(rng, sc.num_robots)
            run.actions.append(a)
            ora.step(a)
            run.hit |= bool(ora.hit_robot.any())
            run.robot_crash |= bool(((ora.result == 2) & (ora.done != 0)).any())
            if k % 4 == 3 or k == sh["ticks"] - 1:
                run.snaps[k] = host_copy(ora)
        run.episodes = int(ora.episode.max())
        _oracle_runs[name] = run
    return _oracle_runs[name]


def assert_the_run_tests_what_it_claims(name, run):
    assert run.episodes >= 2, f"{name}: no robot restarted in the oracle's run"
    assert run.hit, f"{name}: no beam returned from another robot in the oracle's run"
    if SHAPES[name]["selects"][0].startswith("raster"):
        assert run.robot_crash, f"{name}: no crash in the oracle's run"


# ------------------------------------------------------------------------------------------------ mrca_step, every variant
@gpu
@pytest.mark.parametrize("lazy_obs", [True, False], ids=["lazy", "eager"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_variant_bit_exact_against_the_c_oracle(hip, name, lazy_obs):
    run = oracle_run(name)
    assert_the_run_tests_what_it_claims(name, run)
    sc = scenario(name)
    assert selection(sc) == SHAPES[name]["selects"]
    env = hip.VecStageWorld(sc, lazy_obs=lazy_obs)
    mode = "lazy" if lazy_obs else "eager"
    env.reset()
    compare(env, not lazy_obs, run.snaps[-1], f"{name} {mode} reset")
    for k, a in enumerate(run.actions):
        env.step(torch.from_numpy(a).cuda())
        if k in run.snaps:
            compare(env, not lazy_obs, run.snaps[k], f"{name} {mode} step {k}")
    env.check()
    env.close()


# ------------------------------------------------------------------------------------------------ eager mode beyond mrca_step
def _views_equal(eager, lazy, lo, hi, what):
    assert torch.equal(eager._obs[lo:hi], lazy.obs[lo:hi]), f"{what}: obs of robots [{lo}, {hi})"
    assert torch.equal(eager._scan[lo:hi], lazy.scan[lo:hi]), f"{what}: scan of robots [{lo}, {hi})"


@gpu
@pytest.mark.parametrize("name", ["raster8_k2", "big_k2"])
def test_eager_masked_reset_with_overrides(hip, name):
    """mrca_reset of every third robot with poses and goals of the caller's, ten ticks into a run: the eager env's raw views
    (mrca_reset forms them itself) and every other field against the C oracle given the same mask; then five more ticks, whose
    epilogues shift the restarted robots' stacks."""
    sc = scenario(name)
    N = sc.num_robots
    lazy, eager, ora = hip.VecStageWorld(sc), hip.VecStageWorld(sc, lazy_obs=False), U.COracleEnv(sc)
    for e in (lazy, eager, ora):
        e.reset()
    rng = np.random.default_rng(7)

    def ticks(n, what):
        for k in range(n):
            a = U.random_actions(rng, N)
            d = torch.from_numpy(a).cuda()
            lazy.step(d)
            eager.step(d)
            ora.step(a)
        want = host_copy(ora)
        compare(eager, True, want, f"{name} eager {what}")
        compare(lazy, False, want, f"{name} lazy {what}")

    ticks(10, "ten ticks")
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    ang = rng.uniform(-np.pi, np.pi, N)
    rad = rng.uniform(0.0, 5.0, N)
    poses = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3, 3, N)], 1).astype(np.float32)
    goals = rng.uniform(-5, 5, (N, 2)).astype(np.float32)
    before = eager._obs.clone()
    for e in (lazy, eager):
        e.reset(torch.from_numpy(mask).cuda(), torch.from_numpy(poses).cuda(), torch.from_numpy(goals).cuda())
    ora.reset(mask, poses, goals)
    want = host_copy(ora)
    compare(eager, True, want, f"{name} eager masked reset")
    compare(lazy, False, want, f"{name} lazy masked reset")
    keep = torch.from_numpy(mask == 0).cuda()
    assert torch.equal(eager._obs[keep], before[keep])          # the others' stacks stay as they were
    assert (np.asarray(want.pose)[mask == 1] == poses[mask == 1]).all()
    ticks(5, "five ticks after the masked reset")
    for e in (lazy, eager):
        e.check()
        e.close()


@gpu
@pytest.mark.parametrize("name", ["raster4_k2", "raster8_k1"])
def test_eager_world_ranges(hip, name):
    """mrca_step_worlds alternating with mrca_move_worlds + mrca_observe_worlds on worlds [1, 3): the epilogue forms the views
    of the range's robots -- equal to the lazy env's, formed from the ring -- and touches no other row."""
    sc = scenario(name)
    assert sc.num_worlds >= 3
    R = sc.robots_per_world
    lo, hi = R, 3 * R
    lazy, eager = hip.VecStageWorld(sc), hip.VecStageWorld(sc, lazy_obs=False)
    lazy.reset()
    eager.reset()
    rng = np.random.default_rng(8)
    outside = torch.ones(sc.num_robots, dtype=torch.bool, device="cuda")
    outside[lo:hi] = False
    for k in range(12):
        a = torch.from_numpy(U.random_actions(rng, sc.num_robots)).cuda()
        obs0, scan0 = eager._obs.clone(), eager._scan.clone()
        for e in (lazy, eager):
            if k % 2:
                e.move(a, (1, 2))
                e.observe((1, 2))
            else:
                e.step(a, worlds=(1, 2))
        torch.cuda.synchronize()
        _views_equal(eager, lazy, lo, hi, f"{name} call {k}")
        assert torch.equal(eager._obs[outside], obs0[outside]) and torch.equal(eager._scan[outside], scan0[outside]), \
            f"{name} call {k}: a view outside the range changed"
        assert not torch.equal(eager._scan[lo:hi], scan0[lo:hi])
        for f in ("pose", "reward", "done", "result", "episode", "local_goal"):
            assert torch.equal(getattr(eager, f), getattr(lazy, f)), f
    for e in (lazy, eager):
        e.check()
        e.close()


@gpu
def test_eager_step_slice_in_a_big_world(hip):
    """mrca_step_slice (one env sharded over ranks) in worlds of more than 64 robots: every robot advances -- as in an env
    stepped whole --, the views of the slice's robots equal the lazy env's, every other row stays as it was.  One slice starts
    at robot 40 and crosses the worlds' border at 66, the other is the second world."""
    name = "big_k1"
    sc = scenario(name)
    N = sc.num_robots
    whole, lazy, eager = hip.VecStageWorld(sc), hip.VecStageWorld(sc), hip.VecStageWorld(sc, lazy_obs=False)
    for e in (whole, lazy, eager):
        e.reset()
    rng = np.random.default_rng(9)
    for k, (first, count) in enumerate([(40, 70), (66, 66), (40, 70), (66, 66), (0, 41), (40, 70)]):
        a = torch.from_numpy(U.random_actions(rng, N)).cuda()
        obs0, scan0 = eager._obs.clone(), eager._scan.clone()
        whole.step(a)
        lazy.step(a, ray_slice=(first, count))
        eager.step(a, ray_slice=(first, count))
        torch.cuda.synchronize()
        _views_equal(eager, lazy, first, first + count, f"{name} slice ({first}, {count}), call {k}")
        outside = torch.ones(N, dtype=torch.bool, device="cuda")
        outside[first:first + count] = False
        assert torch.equal(eager._obs[outside], obs0[outside]) and torch.equal(eager._scan[outside], scan0[outside]), \
            f"call {k}: a view outside the slice changed"
        assert torch.equal(eager._scan[first:first + count], whole.scan[first:first + count])
        for f in ("pose", "speed", "speed_gt", "reward", "done", "crashed", "t", "episode"):
            assert torch.equal(getattr(eager, f), getattr(whole, f)), f
    for e in (whole, lazy, eager):
        e.check()
        e.close()


@gpu
@pytest.mark.parametrize("ticks_per_launch", [None, 3])
@pytest.mark.parametrize("chains", [1, 2, 3])
@pytest.mark.parametrize("name", ["raster8_k2", "exact_k1_five_waves"])
def test_eager_step_many_against_the_c_oracle(hip, monkeypatch, name, chains, ticks_per_launch):
    """mrca_step_many in eager mode: calls of 1, 7 and 30 ticks, after each the raw views and every field equal the C oracle
    stepped tick by tick.  The VIEWS epilogue reads the rows earlier ticks stored, so an eager env sends a launch per tick
    whatever MRCA_TICKS_PER_LAUNCH says: the same must hold with the switch at 3."""
    import bench
    if ticks_per_launch is None:
        monkeypatch.delenv("MRCA_TICKS_PER_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", str(ticks_per_launch))
    sc = scenario(name)
    eager, ora = hip.VecStageWorld(sc, lazy_obs=False), U.COracleEnv(sc)        # (the switch is read here, once)
    pool = bench.action_pool(sc.num_robots, eager.device, 9, depth=40)
    host_pool = [a.cpu().numpy() for a in pool]
    eager.reset()
    ora.reset()
    k = 0
    for K in (1, 7, 30):
        eager.step_many(pool, k, K, chains)
        for j in range(K):
            ora.step(host_pool[(k + j) % len(host_pool)])
        k += K
        compare(eager, True, host_copy(ora), f"{name} eager, chains {chains}, after the call of {K} ticks")
    eager.check()
    eager.close()


@gpu
def test_eager_tick_captured_and_replayed(hip):
    """One mrca_step of an eager env captured into a hipGraph on a side stream and replayed eight times: the epilogue's views
    after eight ticks of the one action, against the C oracle."""
    name = "raster8_k1"
    sc = scenario(name)
    eager, ora = hip.VecStageWorld(sc, lazy_obs=False), U.COracleEnv(sc)
    eager.reset()
    ora.reset()
    a = U.random_actions(np.random.default_rng(10), sc.num_robots)
    d = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        eager.step(d)
    compare(eager, True, host_copy(ora), f"{name}: a capture must not move the world")
    for _ in range(8):
        g.replay()
        ora.step(a)
    compare(eager, True, host_copy(ora), f"{name}: eight replays of a captured tick")
    eager.check()
    eager.close()
