"""The plain-C restatement of the oracle (oracle/mrca_oracle_c.c: CPU baseline + fast checker) must
agree bit-for-bit with the NumPy oracle's fp32 mode on every field."""
import numpy as np
import pytest

import util as U
from util import S


def _run(sc, steps, seed, every=1):
    o = U.oracle_env(sc)
    c = U.COracleEnv(sc)
    o.reset()
    c.reset()
    U.assert_state_equal(c, o, what=f"{sc.name} reset")
    rng = np.random.default_rng(seed)
    for k in range(steps):
        a = U.random_actions(rng, sc.num_robots)
        o.step(a)
        c.step(a)
        if k % every == 0 or k == steps - 1:
            U.assert_state_equal(c, o, what=f"{sc.name} step {k}")


def test_c_oracle_stage1():
    _run(S.stage1(num_worlds=3, robots_per_world=8, seed=4), 100, 1)


def test_c_oracle_stage2_groups():
    _run(S.stage2(num_worlds=1, seed=6), 210, 2, every=7)


def test_c_oracle_stage2_hold_velocity():
    _run(S.stage2(num_worlds=1, seed=6, hold_velocity=True), 90, 2, every=6)      # first group restart at step 46


def test_c_oracle_fidelity_mode_with_the_raster_lidar():
    """Stage's own resolutions: 0.2 m map cells, robots collide when their outlines share a 0.2 m raster cell AND are seen
    by each other's lidar through that raster (the C oracle marks a window of cells per robot, the NumPy oracle walks the
    full set: bit-identical)."""
    _run(S.stage1(num_worlds=2, robots_per_world=12, seed=3, stage_resolution=True), 40, 5, every=4)
    _run(S.stage2(num_worlds=1, seed=2, stage_resolution=True), 24, 6, every=6)


def test_c_oracle_circle():
    _run(S.circle(num_worlds=1, seed=1), 15, 3)


def test_c_oracle_world_slice_matches_full_batch():
    sc = S.stage1(num_worlds=4, robots_per_world=6, seed=9)
    full = U.COracleEnv(sc)
    sl_sc = S.stage1(num_worlds=1, robots_per_world=6, seed=9)
    sl = U.COracleEnv(sl_sc, first_world=3)
    full.reset()
    sl.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        a = U.random_actions(rng, sc.num_robots)
        full.step(a)
        sl.step(a[18:])
    assert (full.pose[18:].view(np.uint32) == sl.pose.view(np.uint32)).all()
    assert (full.scan[18:].view(np.uint32) == sl.scan.view(np.uint32)).all()


# The C oracle is the yardstick of tests/test_gpu_raycast_variants.py: pinned here, against the NumPy oracle, at the beam counts,
# frame counts and raster sizes it is newly used at (sized for the NumPy oracle: 10 robots, 15 ticks).
@pytest.mark.parametrize("raster, beams, frames", [(0.1, 192, 3), (0.1, 512, 3), (0.13, 192, 3), (0.13, 512, 3),
                                                  (0.0, 64, 1), (0.0, 320, 4)])
def test_c_oracle_at_the_beam_counts_and_rasters_of_the_variant_tests(raster, beams, frames):
    """Robots 0 / 1 and 2 / 3 start 1.4 m apart, face to face, and drive straight at each other; the other six stand round them,
    well inside lidar reach, with random commands.  Each pair collides inside the run -- at least the robot of a pair that moves into the other
    crashes -- and who crashed restarts (asserted): the restarts and
    every tick before and after them equal bit for bit on every field and every hit flag."""
    sc = S.stage1(num_worlds=1, robots_per_world=10, seed=12)
    sc.beams, sc.frames, sc.collision_raster = beams, frames, raster
    N = sc.num_robots
    ang = 2.0 * np.pi * np.arange(N - 4) / (N - 4)
    poses = np.concatenate([[[-0.7, 1.03, 0.0], [0.7, 0.97, np.pi - 0.05], [0.02, -1.7, np.pi / 2], [-0.02, -0.3, -np.pi / 2]],
                            np.stack([2.5 * np.cos(ang), 2.5 * np.sin(ang), ang + 2.0], 1)]).astype(np.float32)
    goals = np.stack([-poses[:, 0], -poses[:, 1]], 1) * np.float32(1.5)
    mask = np.ones(N, np.uint8)
    o, c = U.oracle_env(sc), U.COracleEnv(sc)
    o.reset(mask, poses, goals)
    c.reset(mask, poses, goals)
    what = f"raster {raster}, {beams} beams, {frames} frames"
    U.assert_state_equal(c, o, what=f"{what}: reset")
    assert (np.asarray(c.hit_robot) == np.asarray(o.hit_robot)).all() and c.hit_robot.any()
    rng = np.random.default_rng(5)
    crashed = np.zeros(N, bool)
    for k in range(15):
        a = U.random_actions(rng, N)
        a[:4] = (1.0, 0.0)
        o.step(a)
        c.step(a)
        U.assert_state_equal(c, o, what=f"{what}: step {k}")
        assert (np.asarray(c.hit_robot).astype(bool) == np.asarray(o.hit_robot).astype(bool)).all(), f"{what}: hit_robot, step {k}"
        crashed |= (c.result == 2) & (c.done != 0)
    assert crashed[:4].sum() >= 2, f"the pairs did not collide: {crashed[:4]}"
    assert (crashed[:4] <= (c.episode[:4] >= 2)).all(), f"a crashed robot did not restart: {c.episode[:4]}"
