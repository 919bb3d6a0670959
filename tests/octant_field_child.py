"""Child process of tests/test_gpu_octant_field.py: every shape of SHAPES, lazy and eager, through mrca_step and through
mrca_step_many, against the C oracle -- with whatever MRCA_FIELD_OCTANTS the parent set (mrca_create reads it).  Prints one line
per run and exits non-zero at the first difference."""
import sys

import numpy as np
import torch

import util as U
from util import S
from test_gpu_raycast_variants import compare, host_copy

TICKS = 12


def _fidelity():
    return S.stage1(num_worlds=2, robots_per_world=3, seed=53, stage_resolution=True)


# the smallest envs that reach every instantiation the field object goes through: the exact lidar (two beams per thread, one
# after the other), the raster lidar, the big-world variants; each lazy (VIEWS = false) and eager; mrca_step_many's launches of
# three ticks (frames = 3), over two world ranges where there are two worlds
SHAPES = {
    "stage1_2x3": lambda: S.stage1(num_worlds=2, robots_per_world=3, seed=51),
    "stage2_1": lambda: S.stage2(num_worlds=1, seed=52),
    "circle_1": lambda: S.circle(num_worlds=1, seed=54),
    "stage1_fidelity_2x3": _fidelity,
    "stage1_big_1x70": lambda: S.stage1(num_worlds=1, robots_per_world=70, seed=55),
}


def wall_pose(grid):
    """(x, y, heading) on a cell face, one cell from a wall and heading along it: the free cell nearest the map's middle row that
    has a wall cell to its east and free cells north of it -- x on the cell's west face, y mid-cell, heading north"""
    occ = grid.dense()
    free = ~occ
    ok = free[:-3, :-1] & occ[:-3, 1:] & free[1:-2, :-1] & free[2:-1, :-1] & free[3:, :-1]
    ys, xs = np.nonzero(ok)
    assert len(ys), "no free cell with a wall to its east"
    k = np.argmin(np.abs(ys - grid.height // 2) * 4 + np.abs(xs - grid.width // 2))
    x = np.float32(grid.x0) + np.float32(xs[k]) * np.float32(grid.cell)
    y = np.float32(grid.y0) + (np.float32(ys[k]) + np.float32(0.5)) * np.float32(grid.cell)
    return float(x), float(y), float(np.float32(np.pi / 2))


def run(hip, name, lazy):
    sc = SHAPES[name]()
    N = sc.num_robots
    ora = U.COracleEnv(sc)
    stepped, many = hip.VecStageWorld(sc, lazy_obs=lazy), hip.VecStageWorld(sc, lazy_obs=lazy)
    mask = np.zeros(N, np.uint8)
    mask[0] = 1
    poses = np.zeros((N, 3), np.float32)
    poses[0] = wall_pose(sc.grid)
    goals = np.zeros((N, 2), np.float32)
    for e in (ora, stepped, many):
        e.reset()
    ora.reset(mask, poses, goals)
    for e in (stepped, many):
        e.reset(torch.from_numpy(mask).cuda(), torch.from_numpy(poses).cuda(), torch.from_numpy(goals).cuda())
    what = f"{name} {'lazy' if lazy else 'eager'}"
    want = host_copy(ora)
    assert (np.asarray(want.pose)[0] == poses[0]).all()
    assert float(np.asarray(want.scan)[0].min()) < 3 * sc.grid.cell          # the robot does stand at the wall
    compare(stepped, not lazy, want, f"{what}: reset onto a cell face along a wall")
    rng = np.random.default_rng(56)
    host = [U.random_actions(rng, N) for _ in range(TICKS)]
    pool = [torch.from_numpy(a).cuda() for a in host]
    for k in range(TICKS):
        stepped.step(pool[k])
        ora.step(host[k])
        compare(stepped, not lazy, host_copy(ora), f"{what}: mrca_step, tick {k}")
    many.step_many(pool, 0, TICKS, 2)
    many.invalidate_views()
    compare(many, not lazy, host_copy(ora), f"{what}: mrca_step_many, {TICKS} ticks in two ranges")
    for e in (stepped, many):
        e.check()
        e.close()
    print(f"ok {what}", flush=True)


def main():
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    for name in SHAPES:
        for lazy in (True, False):
            run(vec_env, name, lazy)
    print("all ok", flush=True)


if __name__ == "__main__":
    sys.exit(main())
