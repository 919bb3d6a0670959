"""The ray casts of several run-ahead ticks in one launch (csrc/mrca_raycast_ticks.hip, mrca_step_many's run-ahead pass) against
the same ticks taken one by one (run with -m gpu on an MI355X).

Two envs of one seed and one action pool: one is driven by ``step_many`` -- calls of 1, 2, 3, 4, 5, 7, 38 and 300 ticks one
after the other, the last one crossing a pass boundary (a pass is at most 256 ticks) --, the other tick by tick with ``step``.
After every call every field a caller reads (bench.DUMP_FIELDS), the scan ring, the ring heads and the hit bits must be equal
bit for bit.  The whole set runs with the library's own choice of ticks per launch (the ring's frame count for these shapes,
one in fidelity mode), with MRCA_TICKS_PER_LAUNCH=1, with 2 (whose blocks follow a rule of their own) and with 3 (fidelity mode's
launches of several ticks).

A launch of several ticks treats a robot that restarts in its first, a middle or its last tick differently (ring_rule,
mrca_device.h): the reference run must hold each of them, which the test asserts from the reference's fresh flags -- the seeds
below were checked beforehand against the C oracle (tests/util.COracleEnv) on the CPU."""
import numpy as np
import pytest
import torch

import util as U
from pass_plan_ref import PASS_TICKS, launch_plan
from util import S

pytestmark = pytest.mark.gpu

CALLS = (1, 2, 3, 4, 5, 7, 38, 300)
def _stage1(beams=512, raster=None, **kw):
    sc = S.stage1(**kw)
    sc.beams = beams
    if raster is not None:
        sc.collision_raster = raster
    return sc


SHAPES = {
    "stage1_4x8": lambda: S.stage1(num_worlds=4, robots_per_world=8, seed=41),
    "stage1_3x5": lambda: S.stage1(num_worlds=3, robots_per_world=5, seed=42),       # 15 robots: no multiple of 8
    "stage2_2x44": lambda: S.stage2(num_worlds=2, seed=43),                          # group restarts: many fresh in one tick
    "stage1_fidelity_4x8": lambda: S.stage1(num_worlds=4, robots_per_world=8, seed=44, stage_resolution=True),
    # one beam per thread (128 beams: two waves, raycast_ticks_kernel<1, false, 0>)
    "stage1_k1_3x5": lambda: _stage1(beams=128, num_worlds=3, robots_per_world=5, seed=45),
    # the raster lidar with the 8-cell outline window on the 0.05 m map (<2, true, 8>; several ticks per launch only under
    # MRCA_TICKS_PER_LAUNCH=3, like the fidelity shape above)
    "stage1_raster8_4x8": lambda: _stage1(raster=0.1, num_worlds=4, robots_per_world=8, seed=46),
}
EXTRA = ("scan_ring", "ring_head", "hit_bits", "fresh")


def restart_positions(fresh, T):
    """{"first", "middle", "last"} positions inside a launch of several ticks at which some robot of the run restarts; fresh:
    [ticks, N] the fresh flags after every tick of the CALLS sequence"""
    seen, t0 = set(), 0
    for K in CALLS:
        for p0 in range(0, K, PASS_TICKS):
            for k, n in launch_plan(min(PASS_TICKS, K - p0), T):
                for j in range(n if n > 1 else 0):
                    if fresh[t0 + p0 + k + j].any():
                        seen.add("first" if j == 0 else "last" if j == n - 1 else "middle")
        t0 += K
    return seen


def host_actions(sc):
    rng = np.random.default_rng(1000 + sc.seed)
    return [U.random_actions(rng, sc.num_robots) for _ in range(64)]


def snapshot(env, fields):
    torch.cuda.synchronize()
    return {k: getattr(env, k).cpu().numpy().copy() for k in fields}


_reference = {}


def reference_run(hip, bench, name):
    """the tick-by-tick run of a shape, computed once: the state after every call's last tick and the fresh flags of every tick"""
    if name not in _reference:
        sc = SHAPES[name]()
        env = hip.VecStageWorld(sc)
        pool = [torch.from_numpy(a).to(env.device) for a in host_actions(sc)]
        env.reset()
        snaps, fresh, k = [], [], 0
        for K in CALLS:
            for _ in range(K):
                env.step(pool[k % len(pool)])
                fresh.append(env.fresh.cpu().numpy().copy())
                k += 1
            snaps.append(snapshot(env, bench.DUMP_FIELDS + EXTRA))
        env.close()
        _reference[name] = (snaps, np.stack(fresh))
    return _reference[name]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


@pytest.mark.parametrize("ticks_per_launch", [None, 1, 2, 3])
@pytest.mark.parametrize("chains", [1, 2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_step_many_equals_tick_by_tick(hip, monkeypatch, name, chains, ticks_per_launch):
    import bench
    if ticks_per_launch is None:
        monkeypatch.delenv("MRCA_TICKS_PER_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", str(ticks_per_launch))
    snaps, fresh = reference_run(hip, bench, name)
    sc = SHAPES[name]()
    # the reference run restarts robots at every position of a launch of several ticks
    assert restart_positions(fresh, sc.frames) == {"first", "middle", "last"}, restart_positions(fresh, sc.frames)
    env = hip.VecStageWorld(sc)               # (the switch is read here, once)
    pool = [torch.from_numpy(a).to(env.device) for a in host_actions(sc)]
    env.reset()
    k = 0
    for K, want in zip(CALLS, snaps):
        env.step_many(pool, k, K, chains)
        env.invalidate_views()
        k += K
        got = snapshot(env, bench.DUMP_FIELDS + EXTRA)
        for f in bench.DUMP_FIELDS + EXTRA:
            a, b = got[f], want[f]
            same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
            assert same.all(), (f"{name}, chains {chains}, ticks per launch {ticks_per_launch}: {f} differs at "
                                f"{int((~same).sum())} of {same.size} entries after the call of {K} ticks ({k} in all)")
    env.check()
    env.close()
