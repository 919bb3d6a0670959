"""What the ray cast reads and writes through the view -- the free-rectangle field, the ring rows, the hit words, the heads,
local_goal, the eager views -- is addressed as a base in scalar registers plus a 32-bit byte offset (csrc/mrca_device.h:
global_load / global_store; run with -m gpu on an MI355X).  An offset that is wrong is wrong first where the index is smallest or
the clamp acts: the smallest worlds (one world of 2 robots, two worlds of 3), on a map WITHOUT walls round it, with the robots

* in the map's four corner cells, looking out over the corner (every lookup behind the first clamps into the zero border, on
  both axes);
* one cell inside each of the four edges, facing out;
* on the face of a block, looking into it (ranges of -0.0: the first boundary's time, the first lookup's hit).

Round after round the robots are reset onto the next poses of that list and a few ticks are taken: with mrca_step, and with
mrca_step_many for 3 and for 4 ticks (a launch of three ticks; one of three and a single one), MRCA_FIELD_OCTANTS=0 and 1, lazy_obs
0 and 1; plus one fidelity-mode case (the raster lidar's kernels) and one world of 65 robots (the big-world kernel, its hash
tables read the same way).  After every call EVERY field of U.STATE_FIELDS and the hit flags equal the C oracle's bit for bit,
and so do the scan ring's rows, the ring heads and the hit words of every slot -- replayed from the oracle's scans of the ticks
before with the ring's rule (a restart writes every slot and leaves the head; any other tick advances the head and writes that
slot)."""
import types

import numpy as np
import pytest
import torch

import util as U
from test_gpu_raycast_variants import RawView, host_copy
from util import S

pytestmark = pytest.mark.gpu

f32 = np.float32
CELL, X0, Y0, W, H = 0.0625, -1.25, -1.125, 40, 36           # a power-of-two cell: the block's face is a float
BLOCK = (18, 16, 22, 20)                                     # cells [18, 22) x [16, 20)


def grid():
    occ = np.zeros((H, W), bool)
    occ[BLOCK[1]:BLOCK[3], BLOCK[0]:BLOCK[2]] = True
    return S.GridData.from_dense(occ, CELL, X0, Y0)


def centre(ix, iy):
    return X0 + (ix + 0.5) * CELL, Y0 + (iy + 0.5) * CELL


# (x, y, heading): the lidar covers the half circle in front
POSES = [
    (*centre(0, 0), -0.75 * np.pi), (*centre(W - 1, H - 1), 0.25 * np.pi),          # corners, looking out over the corner
    (*centre(W - 1, 0), -0.25 * np.pi), (*centre(0, H - 1), 0.75 * np.pi),
    (*centre(1, 11), np.pi), (*centre(W - 2, 25), 0.0),                             # one cell inside an edge, facing out
    (*centre(9, 1), -0.5 * np.pi), (*centre(30, H - 2), 0.5 * np.pi),
    (X0 + BLOCK[2] * CELL, Y0 + 17.5 * CELL, np.pi),                                # on the block's east face, looking in
]


def poses_of_round(n_robots, rnd):
    """robot n of round rnd stands on POSES[(rnd * n_robots + n) % 9]: every robot count walks the whole list"""
    p = np.array([POSES[(rnd * n_robots + n) % len(POSES)] for n in range(n_robots)], f32)
    goals = np.stack([-p[:, 0] * f32(0.5), -p[:, 1] * f32(0.5)], 1).astype(f32)
    return p, goals


def big_poses(n_robots, rnd):
    """the world of 65: the nine poses, and the others on a lattice beside the map (0.7 m apart: nobody touches)"""
    p, g = poses_of_round(n_robots, rnd)
    for n in range(len(POSES), n_robots):
        k = n - len(POSES)
        p[n] = (X0 - 1.0 - 0.7 * (k % 8), Y0 + 0.7 * (k // 8), 0.3 * k)
        g[n] = (p[n, 0] + 1.0, p[n, 1])
    return p, g


def _scenario(worlds, R, beams=512, raster=0.0, seed=5):
    sc = S.stage1(num_worlds=worlds, robots_per_world=R, seed=seed, grid=grid())
    sc.beams, sc.collision_raster = beams, raster
    return sc


SHAPES = {
    "w1x2": dict(make=lambda: _scenario(1, 2), rounds=5, poses=poses_of_round),
    "w2x3": dict(make=lambda: _scenario(2, 3), rounds=2, poses=poses_of_round),
    "fidelity_w2x3": dict(make=lambda: _scenario(2, 3, raster=0.2), rounds=2, poses=poses_of_round),
    "big_w1x65": dict(make=lambda: _scenario(1, 65), rounds=1, poses=big_poses),
}
TICKS = 4          # per round in the oracle's run: what the longest call takes


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


_runs = {}


def oracle_run(name):
    """the C oracle's run of a shape, computed once: per round the poses and goals, the commands, and after the reset (index 0)
    and after every tick (1..TICKS) the state and what the ring's rule needs: the scan, the hit flags, who restarted"""
    if name not in _runs:
        sh = SHAPES[name]
        sc = sh["make"]()
        ora = U.COracleEnv(sc)
        rng = np.random.default_rng(17)
        rounds = []
        for r in range(sh["rounds"]):
            poses, goals = sh["poses"](sc.num_robots, r)
            ora.reset(None, poses, goals)
            rec = types.SimpleNamespace(poses=poses, goals=goals, actions=[], snaps=[], marks=[])

            def mark(fresh):
                rec.snaps.append(host_copy(ora))
                rec.marks.append((np.array(ora.scan), np.array(ora.hit_robot).astype(bool), fresh))
            mark(np.ones(sc.num_robots, bool))
            for _ in range(TICKS):
                a = U.random_actions(rng, sc.num_robots)
                a[:, 0] *= f32(0.5)
                rec.actions.append(a)
                ora.step(a)
                mark(np.array(ora.fresh) != 0)
            rounds.append(rec)
        _runs[name] = (sc, rounds)
    return _runs[name]


class Ring:
    """the scan ring, its hit words and heads as the oracle's scans say they are"""

    def __init__(self, sc):
        N, F, B = sc.num_robots, sc.frames, sc.beams
        self.F = F
        self.rows = np.zeros((N, F, B), f32)
        self.words = np.zeros((N, F, B // 64), np.uint64)
        self.head = np.zeros(N, np.int64)

    def tick(self, scan, hit, fresh):
        words = np.packbits(hit, axis=1, bitorder="little").view(np.uint64)
        ar = np.arange(len(self.head))
        self.head = np.where(fresh, self.head, (self.head + 1) % self.F)
        self.rows[ar, self.head], self.words[ar, self.head] = scan, words
        self.rows[fresh], self.words[fresh] = scan[fresh, None, :], words[fresh, None, :]


def compare(env, eager, ring, want, what):
    torch.cuda.synchronize()
    U.assert_state_equal(RawView(env, eager), want, what=what)
    U.assert_hits_equal(env, want, what=what)
    rows = env.scan_ring.cpu().numpy()
    same = rows.view(np.uint32) == ring.rows.view(np.uint32)
    assert same.all(), f"{what}: scan_ring differs at {int((~same).sum())} of {same.size} entries, first {np.argwhere(~same)[0]}"
    assert np.array_equal(env.ring_head.cpu().numpy().astype(np.int64), ring.head), f"{what}: ring_head"
    words = env.hit_bits.cpu().numpy().view(np.uint64)
    assert np.array_equal(words, ring.words), f"{what}: hit words differ at {np.argwhere(words != ring.words)[:1]}"


def drive(hip, monkeypatch, name, mode, octants, lazy_obs, ticks_per_launch=None):
    monkeypatch.setenv("MRCA_FIELD_OCTANTS", str(octants))
    if ticks_per_launch is None:
        monkeypatch.delenv("MRCA_TICKS_PER_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", str(ticks_per_launch))
    sc, rounds = oracle_run(name)
    assert any((r.marks[0][0].view(np.uint32) == 0x80000000).any() for r in rounds), "no -0.0 range: nobody is on the face"
    assert all((r.marks[0][0] == f32(6.0)).any() for r in rounds), "no beam leaves the map"
    env = hip.VecStageWorld(sc, lazy_obs=bool(lazy_obs))                # (the switches are read here, once)
    ring = Ring(sc)
    eager = not lazy_obs
    for r, rec in enumerate(rounds):
        what = f"{name} {mode} octants {octants} lazy_obs {lazy_obs} round {r}"
        env.reset(None, dev(rec.poses), dev(rec.goals))
        ring.tick(*rec.marks[0])
        compare(env, eager, ring, rec.snaps[0], what + " reset")
        if mode == "step":
            for k in (1, 2):
                env.step(dev(rec.actions[k - 1]))
                ring.tick(*rec.marks[k])
                compare(env, eager, ring, rec.snaps[k], what + f" tick {k}")
        else:
            K = int(mode[4:])
            pool = [dev(a) for a in rec.actions]
            env.step_many(pool, 0, K, 1)
            env.invalidate_views()
            for k in range(1, K + 1):
                ring.tick(*rec.marks[k])
            compare(env, False, ring, rec.snaps[K], what + f" after the call of {K} ticks")
    env.check()
    env.close()


@pytest.mark.parametrize("lazy_obs", [0, 1])
@pytest.mark.parametrize("octants", [0, 1])
@pytest.mark.parametrize("mode", ["step", "many3", "many4"])
@pytest.mark.parametrize("name", ["w1x2", "w2x3"])
def test_smallest_worlds_bit_exact_against_the_c_oracle(hip, monkeypatch, name, mode, octants, lazy_obs):
    drive(hip, monkeypatch, name, mode, octants, lazy_obs)


@pytest.mark.parametrize("mode", ["step", "many4"])
def test_fidelity_mode(hip, monkeypatch, mode):
    # (the raster lidar's launches take several ticks only when told to)
    drive(hip, monkeypatch, "fidelity_w2x3", mode, 1, 1, ticks_per_launch=3)


@pytest.mark.parametrize("mode", ["step", "many3"])
def test_a_world_of_65_robots(hip, monkeypatch, mode):
    drive(hip, monkeypatch, "big_w1x65", mode, 1, 1)
