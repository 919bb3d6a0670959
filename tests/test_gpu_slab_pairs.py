"""The pair-major slab tests of the ray cast (csrc/mrca_raycast_body.h, PAIRS: small worlds, exact rectangles) against the C
oracle on CHOSEN geometry (run with -m gpu on an MI355X; the scenes' own claims are checked on the CPU, without one).

Every scene is a Stage-1 world on tests/degenerate_scenes.coarse_grid whose robots start -- and restart -- on table poses
(RESET_TABLE), so which (neighbour, beam) pairs a robot's workgroup forms is set here and not drawn:

  alone          one robot per world: an empty list, no second barrier
  straddle_63    one neighbour whose beams straddle 63 | 64: two waves merge into one neighbour's interval
  straddle_255   ... and 255 | 256: a thread's first beam and another thread's second
  inside_near    a neighbour closer than beam_interval's `near`: every beam of the row is a pair of one neighbour (512 pairs, two
                 passes of the pair loop)
  cluster8       eight robots in a ring of 0.9 m, facing its centre: more than 256 pairs per robot
  tandem         two neighbours one behind the other dead ahead: the minimum is taken across them, the hit bit is set
  behind_wall    a neighbour beyond a block that is nearer: the range and the hit bit stay the block's
  minus_zero     a sensor exactly on the face of a block, looking along and into it, and a neighbour beyond the block whose
                 interval covers beams that enter the block at boundary time -0: the range stays -0.0 and the hit bit clear -- the
                 merge is a SIGNED minimum of the bit patterns (slab_pair_merge, csrc/mrca_device.h)
  full64         64 robots in one world on a lattice of 1 m: 63 candidates, lists of more than eight (the search's loop)

each with 512 beams (two beams per thread, four waves) and with 64 (one wave, one beam per thread).  ``test_the_scenes_are_what_
they_claim`` holds each claim against the oracle's own scan after the reset.  On the device the first tick's commands are zero --
the geometry above is what the first ray cast of ``step`` sees as well --, six ticks of random commands follow (crashed robots
restart on their table poses).  Three envs per scene: one stepped tick by tick and compared after every tick (the single-tick
kernel), one under MRCA_TICKS_PER_LAUNCH=3 through ``step_many`` in calls of 3 and 4 ticks (launches of three ticks and of one), and
for two scenes one with lazy_obs = 0 (the VIEWS instantiation), its raw scan and observation compared.  Compared bit for bit:
every field of util.STATE_FIELDS -- the newest scan, the observation stack (the scan ring in deque order), poses, rewards -- and
the hit bits."""
import types

import numpy as np
import pytest
import torch

import degenerate_scenes as D
import util as U
from test_gpu_raycast_variants import compare, host_copy
from util import S

f = np.float32
TICKS = 7
MINUS_ZERO = 0x80000000


def bearing(i, beams=512):
    """of beam i in the sensor's frame"""
    return -np.pi / 2 + i * np.pi / (beams - 1)


def _at(angle, dist, heading):
    return (dist * np.cos(angle), dist * np.sin(angle), heading)


def _ring8():
    ang = 2 * np.pi * np.arange(8) / 8
    return [(0.9 * np.cos(a), 0.9 * np.sin(a), a + np.pi) for a in ang]


def _lattice64():
    rng = np.random.default_rng(9)
    return [(-3.5 + i, -3.5 + j, rng.uniform(-np.pi, np.pi)) for j in range(8) for i in range(8)]


# name -> the table poses of a world's robots (x, y, heading); robot 0 is the sensor the claim is about
SCENES = {
    "alone": [(0.0, 0.0, 0.3)],
    "straddle_63": [(0.0, 0.0, 0.0), _at(bearing(63.5), 2.0, 0.7)],
    "straddle_255": [(0.0, 0.0, 0.0), (2.0, 0.0, 2.0)],
    "inside_near": [(0.0, 0.0, 0.0), (0.25, 0.0, 1.0)],
    "cluster8": _ring8(),
    "tandem": [(0.0, 0.0, 0.0), (1.5, 0.0, 0.4), (3.0, 0.0, -0.4)],
    "behind_wall": [(4.5, -3.5, -np.pi / 2), (4.5, -7.0, 0.0)],          # block A: x in [2.5, 6.5), y in [-6, -4.5)
    "minus_zero": [(-6.0, 6.0, np.pi / 2), (-8.5, 6.0, 0.0)],            # block B: x in [-7, -6), y in [4, 7)
    "full64": _lattice64(),
}
BEAMS = (512, 64)
EAGER = ("cluster8", "minus_zero")           # the scenes that also run with lazy_obs = 0, at 512 beams


def scenario(name, beams):
    poses = np.asarray(SCENES[name], np.float64)
    sc = S.stage1(num_worlds=2, robots_per_world=len(poses), seed=61, grid=D.coarse_grid())
    sc.beams = beams
    sc.reset_mode[:] = S.RESET_TABLE
    sc.goal_mode[:] = S.RESET_TABLE
    sc.init_table[:] = poses
    sc.goal_table[:] = (8.0, 8.0)
    return sc


_runs = {}


def oracle_run(name, beams):
    """the C oracle's run of a scene, computed once and never changed: the commands, the state after the reset (-1) and after every tick"""
    if (name, beams) not in _runs:
        sc = scenario(name, beams)
        ora = U.COracleEnv(sc)
        ora.reset()
        rng = np.random.default_rng(600 + len(name))
        run = types.SimpleNamespace(actions=[], snaps={-1: host_copy(ora)})
        for k in range(TICKS):
            a = U.random_actions(rng, sc.num_robots)
            if k == 0:
                a[:] = 0.0
            ora.step(a)
            run.actions.append(a)
            run.snaps[k] = host_copy(ora)
        _runs[name, beams] = run
    return _runs[name, beams]


def claim(name, beams, snap):
    """what the scene is here for, of the oracle's scan of the sensor (robot 0 of world 0) at the table poses"""
    scan, hit = snap.scan[0], snap.hit_robot[0].astype(bool)
    ahead = beams // 2
    if name == "alone":
        return not snap.hit_robot.any()
    if name == "straddle_63":
        return bool(hit[63] and hit[64]) if beams == 512 else bool(hit.any() and not hit.all())
    if name == "straddle_255":
        return bool(hit[ahead - 1] and hit[ahead] and not hit[0] and not hit[-1])
    if name == "inside_near":
        return hit.sum() >= beams // 4         # (a row of pairs whatever they return: the centre distance is under `near`)
    if name == "cluster8":
        # every hit beam is a pair at least: more than one pass of the 256-thread pair loop
        return all(snap.hit_robot[n].sum() > beams // 2 for n in range(8))
    if name == "tandem":
        # the nearer one's return (its rectangle begins before 1.5 m), from a robot; alone, the farther one would return > 2.5 m
        return bool(hit[ahead] and scan[ahead] < 1.5 and scan[ahead] > 1.0)
    if name == "behind_wall":
        return bool(not hit[ahead] and 0.9 < scan[ahead] < 1.1 and not hit.any())
    if name == "minus_zero":
        # the last beams look west along and into the block; the neighbour is dead west, 2.5 m away: its interval ends at them
        zero = scan.view(np.uint32) == MINUS_ZERO
        return bool(zero[-8:].all() and not hit[-8:].any())
    if name == "full64":
        return bool(snap.hit_robot[:64].any(1).sum() >= 48)
    raise KeyError(name)


@pytest.mark.parametrize("beams", BEAMS)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_scenes_are_what_they_claim(name, beams):
    run = oracle_run(name, beams)
    assert claim(name, beams, run.snaps[-1]), f"{name}, {beams} beams: the oracle's scan at the table poses does not show it"
    # the first tick's commands are zero: nobody has moved when the first ray cast of `step` runs
    moved = run.snaps[0].pose.view(np.uint32) != run.snaps[-1].pose.view(np.uint32)
    assert not moved.any(), f"{name}: a robot left its table pose in the tick of zero commands"
    assert claim(name, beams, run.snaps[0])


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


@pytest.mark.gpu
@pytest.mark.parametrize("beams", BEAMS)
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_bit_exact_against_the_c_oracle(hip, monkeypatch, name, beams):
    run = oracle_run(name, beams)
    sc = scenario(name, beams)
    pool = [dev(a) for a in run.actions]
    # tick by tick: the single-tick kernel (lazy views; for two scenes the reference-shaped views as well)
    for lazy_obs in (True, False) if (name in EAGER and beams == 512) else (True,):
        monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", "1")                    # (read once, in mrca_create)
        env = hip.VecStageWorld(sc, lazy_obs=lazy_obs)
        env.reset()
        compare(env, not lazy_obs, run.snaps[-1], f"{name} {beams} lazy_obs {lazy_obs} reset")
        for k in range(TICKS):
            env.step(pool[k])
            compare(env, not lazy_obs, run.snaps[k], f"{name} {beams} lazy_obs {lazy_obs} tick {k}")
        env.check()
        env.close()
    # three ticks per launch: calls of 3 and 4 ticks (launches of 3, 3 and 1)
    monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", "3")
    env = hip.VecStageWorld(sc)
    env.reset()
    k = 0
    for K in (3, 4):
        env.step_many(pool, k, K, 1)
        env.invalidate_views()
        k += K
        compare(env, False, run.snaps[k - 1], f"{name} {beams} three ticks per launch, after the call of {K} ticks")
    env.check()
    env.close()
