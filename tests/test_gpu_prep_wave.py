"""The preparing wave of the ray cast (csrc/mrca_raycast_body.h: the cull at the hardware's accuracy, the prefix sum over the lanes
as six DPP steps, the list's stores) against the C oracle on CHOSEN geometry, bit for bit -- every field of util.STATE_FIELDS (the
newest scan, the observation stack, which is the scan ring in deque order and so the ring's heads) and the hit bits -- over four
ticks (run with -m gpu on an MI355X; the scenes' own claims are checked on the CPU, without one).

A world's robots start -- and restart -- on table poses in an open 64 m map; robot 1 is the OBSERVER the claims are about (at the
origin, heading 0: its frame is the world's), and a candidate's LANE in its preparing wave is the candidate's number in the world:

  rows      candidates kept exactly at lanes 0, 15, 16, 31, 32, 47, 48 and 63 -- the first and last lane of each of the wave's four
            rows of 16 --, everyone else beyond the reach: what the row shifts leave to the two broadcasts
  cluster   every other robot of the world inside 6 m ahead: 63 kept in a world of 64, thousands of pairs
  edges     one neighbour just inside `near` and one just outside, one just inside the reach and one just outside
  compass   neighbours dead ahead, at +-90 degrees and directly behind

in worlds of 64 robots (every row holds candidates), 33 (lane 32 is alone in its row), 2 and 1, two worlds each, 512 beams.  Each runs
through mrca_step, through mrca_step_many at three ticks per launch, with lazy_obs = 0 and in fidelity mode (the raster lidar, its
own radius and near); and each scene once more in a world of 65 robots: the big-world kernel.  ``kept_lanes`` computes with the
host's form of the cull which candidates the observer keeps, and the first test asserts that this is the pattern the scene was
built for -- a scene cannot degenerate unnoticed."""
import types

import numpy as np
import pytest
import torch

import util as U
from test_gpu_raycast_variants import compare, host_copy
from util import S

f = np.float32
BEAMS = 512
TICKS = 4
OBS = 1                                     # the observer's number in its world
ROW_ENDS = (0, 15, 16, 31, 32, 47, 48, 63)
SCENES = ("rows", "cluster", "edges", "compass")
SIZES = (64, 33, 2, 1)
BIG = 65
NEAR, REACH = 0.30, 6.3                     # mrca_create's: every beam up to `near`; lidar_reach2 = 39.69


def _far(k):
    """the k-th place beyond every reach: a lattice of 1 m, 12 m and more from the origin"""
    return (12.0 + k % 8, -4.0 + k // 8, 0.37 * k)


def table(scene, R):
    """[(x, y, heading)] of a world's R robots; robot OBS (robot 0 of a world of one) is the observer"""
    if R == 1:
        return [(0.0, 0.0, 0.0)]
    others = {}                             # number in the world -> pose, of the robots the scene places; the rest stand far away
    if scene == "rows":
        lanes = [l for l in ROW_ENDS if l < R and l != OBS]
        for i, l in enumerate(lanes):
            a = np.deg2rad(-63.0 + 18.0 * i)
            others[l] = (3.0 * np.cos(a), 3.0 * np.sin(a), 0.5 * i)
    elif scene == "cluster":
        k = 0
        for n in range(R):
            if n != OBS:
                others[n] = (1.2 + 0.6 * (k % 8), -2.4 + 0.6 * (k // 8), 0.41 * k)       # 8 x 9 places, 0.6 m apart
                k += 1
    elif scene == "edges":
        places = [(NEAR * (1 - 3e-4), 0.0, 0.3), (0.0, NEAR * (1 + 3e-4), 1.0),
                  (REACH * (1 - 1e-4) * np.cos(0.5), REACH * (1 - 1e-4) * np.sin(0.5), 2.0),
                  (REACH * (1 + 1e-4) * np.cos(-0.5), REACH * (1 + 1e-4) * np.sin(-0.5), -2.0)]
        for n, p in zip([n for n in range(R) if n != OBS], places):
            others[n] = p
    elif scene == "compass":
        places = [(2.0, 0.0, 0.4), (0.0, 2.0, 1.1), (0.0, -2.0, -0.7), (-2.0, 0.0, 2.5)]
        for n, p in zip([n for n in range(R) if n != OBS], places):
            others[n] = p
    else:
        raise KeyError(scene)
    poses, k = [], 0
    for n in range(R):
        if n == OBS:
            poses.append((0.0, 0.0, 0.0))
        elif n in others:
            poses.append(others[n])
        else:
            poses.append(_far(k))
            k += 1
    return poses


def expected_lanes(scene, R):
    """the lanes the scene is built to keep"""
    if R == 1:
        return []
    if scene == "rows":
        return [l for l in ROW_ENDS if l < R and l != OBS]
    if scene == "cluster":
        return [n for n in range(R) if n != OBS]
    placed = [n for n in range(R) if n != OBS][:4]
    if scene == "edges":          # inside near, outside near, inside the reach: kept; outside the reach: dropped
        return placed[:3]
    if scene == "compass":        # ahead and both sides: kept; behind: dropped
        return placed[:3]
    raise KeyError(scene)


def kept_lanes(poses):
    """(lanes, pairs): the candidates the observer keeps by the host's form of the cull (the reach on the squares, then
    beam_interval), and the number of (neighbour, beam) pairs their intervals hold"""
    if len(poses) == 1:
        return [], 0
    p = np.asarray(poses, np.float64).astype(f)
    ox, oy = p[OBS, 0], p[OBS, 1]
    assert p[OBS, 2] == 0                                       # heading 0: cos = 1 and sin = 0 bit for bit, the frame is the world's
    lx, ly = (p[:, 0] - ox).astype(f), (p[:, 1] - oy).astype(f)
    n = len(p)
    lo, hi = np.zeros(n, np.int32), np.zeros(n, np.int32)
    U.emul_lib().emul_beam_interval(n, lx.ctypes.data_as(U.C.c_void_p), ly.ctypes.data_as(U.C.c_void_p), BEAMS,
                                    lo.ctypes.data_as(U.C.c_void_p), hi.ctypes.data_as(U.C.c_void_p))
    keep = (lx * lx + ly * ly <= f(39.69)) & (lo <= hi)
    keep[OBS] = False
    return [int(l) for l in np.nonzero(keep)[0]], int((hi - lo + 1)[keep].sum())


def scenario(scene, R, raster=0.0):
    sc = S.stage1(num_worlds=2, robots_per_world=R, seed=71, grid=S.empty_grid(cells=64, cell=1.0))
    sc.beams = BEAMS
    sc.collision_raster = raster
    sc.reset_mode[:] = S.RESET_TABLE
    sc.goal_mode[:] = S.RESET_TABLE
    sc.init_table[:] = np.asarray(table(scene, R), np.float64)
    sc.goal_table[:] = (20.0, 20.0)
    return sc


_runs = {}


def oracle_run(scene, R, raster=0.0):
    """the C oracle's run, computed once and never changed: the commands (the first tick's are zero: the first ray cast of `step`
    sees the table poses too), the state after the reset (-1) and after every tick"""
    key = (scene, R, raster)
    if key not in _runs:
        sc = scenario(scene, R, raster)
        ora = U.COracleEnv(sc)
        ora.reset()
        rng = np.random.default_rng(700 + len(scene) + R)
        run = types.SimpleNamespace(actions=[], snaps={-1: host_copy(ora)})
        for k in range(TICKS):
            a = U.random_actions(rng, sc.num_robots)
            if k == 0:
                a[:] = 0.0
            ora.step(a)
            run.actions.append(a)
            run.snaps[k] = host_copy(ora)
        _runs[key] = run
    return _runs[key]


@pytest.mark.parametrize("R", SIZES + (BIG,))
@pytest.mark.parametrize("scene", SCENES)
def test_the_observer_keeps_the_lanes_the_scene_is_built_for(scene, R):
    poses = table(scene, R)
    assert len(poses) == R
    lanes, pairs = kept_lanes(poses)
    want = expected_lanes(scene, R)
    assert lanes == want, f"{scene}, a world of {R}: the observer keeps lanes {lanes}, the scene is built for {want}"
    if scene == "rows" and R >= 64:
        assert lanes == [0, 15, 16, 31, 32, 47, 48, 63]
    if scene == "rows" and R == 33:
        assert lanes[-1] == 32 and R - 1 == 32                                      # the only lane of its row of 16
    if scene == "cluster" and R >= 33:
        assert pairs > 4 * 256, pairs                                               # well beyond one pass of the pair loop
    if scene == "edges" and R >= 5:
        ivs = np.asarray(poses)[:, :2]
        d = np.hypot(*(ivs - ivs[OBS]).T)
        inside, outside, reach_in, reach_out = [d[n] for n in [n for n in range(R) if n != OBS][:4]]
        assert inside < NEAR < outside < NEAR * 1.001 and reach_in < REACH < reach_out < REACH * 1.001
    # nobody left a table pose in the tick of zero commands: the first ray cast of `step` sees this geometry as well
    if R <= 64:
        run = oracle_run(scene, R)
        moved = run.snaps[0].pose.view(np.uint32) != run.snaps[-1].pose.view(np.uint32)
        assert not moved.any()
        if want and scene != "edges":
            assert run.snaps[-1].hit_robot[OBS].any(), "no beam of the observer returns from a robot"


# ------------------------------------------------------------------------------------------------ the device
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


def tick_by_tick(hip, monkeypatch, sc, run, lazy_obs, what):
    monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", "1")                    # (read once, in mrca_create)
    env = hip.VecStageWorld(sc, lazy_obs=lazy_obs)
    env.reset()
    compare(env, not lazy_obs, run.snaps[-1], f"{what} reset")
    for k in range(TICKS):
        env.step(dev(run.actions[k]))
        compare(env, not lazy_obs, run.snaps[k], f"{what} tick {k}")
    env.check()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("scene", SCENES)
def test_scene_bit_exact_against_the_c_oracle(hip, monkeypatch, scene, R):
    run, sc = oracle_run(scene, R), scenario(scene, R)
    what = f"{scene}, worlds of {R}:"
    tick_by_tick(hip, monkeypatch, sc, run, True, f"{what} mrca_step")
    tick_by_tick(hip, monkeypatch, sc, run, False, f"{what} lazy_obs = 0")
    # three ticks per launch: a call of three ticks (one launch of three) and a call of one
    monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", "3")
    env = hip.VecStageWorld(sc)
    env.reset()
    pool = [dev(a) for a in run.actions]
    k = 0
    for K in (3, 1):
        env.step_many(pool, k, K, 1)
        env.invalidate_views()
        k += K
        compare(env, False, run.snaps[k - 1], f"{what} three ticks per launch, after the call of {K}")
    env.check()
    env.close()
    # fidelity mode: the raster lidar's preparation, with its own radius and near
    raster = 0.2
    tick_by_tick(hip, monkeypatch, scenario(scene, R, raster), oracle_run(scene, R, raster), True, f"{what} fidelity mode")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_scene_in_a_big_world(hip, monkeypatch, scene):
    tick_by_tick(hip, monkeypatch, scenario(scene, BIG), oracle_run(scene, BIG), True, f"{scene}, worlds of {BIG} (the big-world kernel):")
