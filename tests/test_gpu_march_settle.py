"""The march's one-candidate settlement of the secondary axis (csrc/mrca_device.h: settle_secondary) on the device, against the C
oracle, every field bit for bit (run with -m gpu on an MI355X).

The map is the 48 x 40-cell one of tests/test_march_trip_host.py (a rink, a pillar, a thin wall, a staircase), at its
power-of-two cell (corners and boundary times are exact floats: beams through corners are exact ties) and at 0.05 m (they round).
The robots are reset onto cell corners and onto grid lines, with headings that put the lidar's first and last beam on a
small-integer slope -- a beam from a corner along (p, q) passes through a corner every few cells, where the estimate of the
position on the secondary axis lands on a boundary --, or along an axis.  Robot 0 of every world is commanded to stand still,
so the ticks after the reset cast from the same corner again: one tick by mrca_step (the single-tick kernel), three ticks by one
mrca_step_many call (one launch of three ticks); the others drive.  Shapes: 1 world x 2 robots and 2 worlds x 3 robots (the
smallest row and hit-word offsets), MRCA_FIELD_OCTANTS 0 and 1.  After every call every field of U.STATE_FIELDS, the hit
flags, the scan ring's rows, the hit words of every slot and the ring heads equal the oracle's (the ring replayed from the
oracle's scans with the ring's rule, tests/test_gpu_ray_addressing.Ring)."""
import types

import numpy as np
import pytest
import torch

import util as U
from test_gpu_ray_addressing import Ring, compare, dev
from test_gpu_raycast_variants import host_copy
from test_march_trip_host import GEOMS, H, W, _bitmap
from util import S

pytestmark = pytest.mark.gpu

f32 = np.float32
TICKS = 3
# (ix, iy, on): a free corner of the map well inside it; on = 0 the corner itself, 1 / 2 the grid line through it with x / y mid-cell
SPOTS = [(24, 14, 0), (12, 16, 0), (40, 30, 0), (22, 24, 1), (38, 12, 2), (26, 34, 0), (42, 20, 0), (10, 22, 1)]
# beam 0 looks along (p, q) and the last beam along (-p, -q): heading = atan2(q, p) + pi / 2
SLOPES = [(1, 1), (-1, 1), (2, 1), (1, -2), (1, 0), (0, 1), (-3, 1), (-1, -1), (3, 2), (-2, -3)]


def grid(cell, x0, y0):
    occ, _, _ = _bitmap()
    assert occ.shape == (H, W)
    for ix, iy, _ in SPOTS:
        assert not occ[iy - 1:iy + 1, ix - 1:ix + 1].any(), (ix, iy)
    return S.GridData.from_dense(occ, cell, x0, y0)


def poses_of_round(cell, x0, y0, n_robots, rnd):
    p = np.zeros((n_robots, 3), f32)
    for n in range(n_robots):
        k = rnd * n_robots + n
        ix, iy, on = SPOTS[k % len(SPOTS)]
        sp, sq = SLOPES[k % len(SLOPES)]
        p[n] = (f32(x0) + f32(ix + (0.5 if on == 2 else 0.0)) * f32(cell), f32(y0) + f32(iy + (0.5 if on == 1 else 0.0)) * f32(cell),
                f32(np.arctan2(sq, sp) + np.pi / 2))
    goals = np.stack([p[:, 0] + f32(3.0), p[:, 1] - f32(2.0)], 1).astype(f32)      # (far enough that nobody arrives)
    return p, goals


SHAPES = {"w1x2": (1, 2, 4), "w2x3": (2, 3, 3)}       # worlds, robots per world, rounds


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


_runs = {}


def oracle_run(name, geom):
    """the C oracle's run of a shape on a geometry, computed once and shared: per round the poses, the commands and, after the
    reset and after each tick, the state and what the ring's rule needs"""
    if (name, geom) not in _runs:
        worlds, R, n_rounds = SHAPES[name]
        cell, x0, y0 = GEOMS[geom]
        sc = S.stage1(num_worlds=worlds, robots_per_world=R, seed=61, grid=grid(cell, x0, y0))
        ora = U.COracleEnv(sc)
        rng = np.random.default_rng(62)
        rounds = []
        for r in range(n_rounds):
            poses, goals = poses_of_round(cell, x0, y0, sc.num_robots, r)
            ora.reset(None, poses, goals)
            rec = types.SimpleNamespace(poses=poses, goals=goals, actions=[], snaps=[], marks=[])

            def mark(fresh):
                rec.snaps.append(host_copy(ora))
                rec.marks.append((np.array(ora.scan), np.array(ora.hit_robot).astype(bool), fresh))
            mark(np.ones(sc.num_robots, bool))
            assert (np.asarray(ora.pose) == poses).all()
            for _ in range(TICKS):
                a = U.random_actions(rng, sc.num_robots)
                a[:, 0] *= f32(0.3)
                a[::R] = 0.0                                   # robot 0 of every world stands on its corner
                rec.actions.append(a)
                ora.step(a)
                mark(np.array(ora.fresh) != 0)
            rounds.append(rec)
        _runs[(name, geom)] = (sc, rounds)
    return _runs[(name, geom)]


@pytest.mark.parametrize("octants", [0, 1])
@pytest.mark.parametrize("mode", ["step", "many3"])
@pytest.mark.parametrize("geom", [0, 1], ids=["cell_0.125", "cell_0.05"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_corner_poses_bit_exact_against_the_c_oracle(hip, monkeypatch, name, geom, mode, octants):
    monkeypatch.setenv("MRCA_FIELD_OCTANTS", str(octants))
    monkeypatch.delenv("MRCA_TICKS_PER_LAUNCH", raising=False)
    sc, rounds = oracle_run(name, geom)
    R = sc.robots_per_world
    # what the poses are there for: the standing robots still stand where they were put, and their scans see the map
    for rec in rounds:
        last = np.asarray(rec.snaps[-1].pose)
        alive = np.asarray(rec.snaps[-1].episode)[::R] == np.asarray(rec.snaps[0].episode)[::R]
        assert (last[::R][alive] == rec.poses[::R][alive]).all()
    assert any((np.asarray(rec.snaps[-1].episode)[::R] == np.asarray(rec.snaps[0].episode)[::R]).any() for rec in rounds)
    assert all((rec.marks[0][0] < f32(6.0)).any() for rec in rounds)
    env = hip.VecStageWorld(sc, lazy_obs=True)                 # (the switches are read here, once)
    ring = Ring(sc)
    for r, rec in enumerate(rounds):
        what = f"{name} cell {sc.grid.cell} {mode} octants {octants} round {r}"
        env.reset(None, dev(rec.poses), dev(rec.goals))
        ring.tick(*rec.marks[0])
        compare(env, False, ring, rec.snaps[0], what + " reset")
        if mode == "step":
            env.step(dev(rec.actions[0]))
            ring.tick(*rec.marks[1])
            compare(env, False, ring, rec.snaps[1], what + " one tick by mrca_step")
        else:
            env.step_many([dev(a) for a in rec.actions], 0, TICKS, 1)
            env.invalidate_views()
            for k in range(1, TICKS + 1):
                ring.tick(*rec.marks[k])
            compare(env, False, ring, rec.snaps[TICKS], what + " three ticks by one mrca_step_many call")
    env.check()
    env.close()
