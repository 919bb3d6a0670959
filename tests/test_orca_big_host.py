"""The ORCA baseline on worlds of more than 64 robots, on the host: the neighbour selection through the lidar hash
(csrc/mrca_orca_device.h: orca_neighbours_hashed, orca_rings, orca_key) compiled with g++ -ffp-contract=off and held EQUAL, as
lists of indices, to the all-pairs selection of the same header (orca_neighbours) and to tests/orca_ref.py -- on a lattice that
straddles cell borders and the sign change of floor, on robots exactly on a border and one ulp off it, on heaps of robots on one
spot, at the ring thresholds, with hash masks under which everything aliases, with two worlds in one hash and 250 km from the
origin.  The hash is built here with hash_bucket and a counting sort whose order INSIDE every bucket is shuffled: the answer may
not depend on it.  Then the whole rule (orca_robot_with fed by the hashed list) against orca_ref.robot, on bits.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orca_ref as R
import util as U
from test_orca_host import Params, _fp, _ip, cparams, pack_hits, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32
CELL = 6.5

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "mrca_orca_device.h"
using namespace mrca;
extern "C" int big_rings(float nd) { return orca_rings(nd); }
extern "C" void big_buckets(const float* pose, int N, int Rn, int lmask, int* bucket, int* cell) {
    for (int n = 0; n < N; ++n) {
        bucket[n] = (int)hash_bucket(pose[3 * n], pose[3 * n + 1], kLidarCell, n / Rn, lmask);
        cell[2 * n] = hash_cell_coord(pose[3 * n], kLidarCell);
        cell[2 * n + 1] = hash_cell_coord(pose[3 * n + 1], kLidarCell);
    }
}
extern "C" int big_neighbours(const float* xy, int Rn, int local, float nd, int maxn, int* out) {
    return orca_neighbours(xy, Rn, local, nd, maxn, out);
}
extern "C" int big_neighbours_hashed(const int32_t* lstart, const int32_t* lsorted, int lmask, const float* pose, int world, int Rn,
                                     int n, float nd, int maxn, int* out) {
    return orca_neighbours_hashed(lstart, lsorted, lmask, pose, world, Rn, n, nd, maxn, out);
}
extern "C" unsigned long long big_key(float d2, int j) { return orca_key(d2, j); }
// the whole rule for robot n of an env, its neighbours taken from the hash; the head record is sincos_det of the heading
extern "C" void big_robot(const OrcaParams* q, const int32_t* lstart, const int32_t* lsorted, int lmask, int Rn, int n, uint32_t k0,
                          uint32_t k1, const float* pose, const float* speed_gt, const float* goal, const float* ranges,
                          const unsigned long long* hits, int beams, const float* bc, const float* bs, float* act, float* vel,
                          int* diag, int* nb_out, int* kept_out) {
    const int world = n / Rn;
    std::vector<float> sc(2 * (size_t)Rn);
    for (int j = 0; j < Rn; ++j) sincos_det(pose[3 * (size_t)(world * Rn + j) + 2], &sc[2 * j], &sc[2 * j + 1]);
    int nb[kOrcaMaxNeighbors];
    const int kept = orca_neighbours_hashed(lstart, lsorted, lmask, pose, world, Rn, n, q->neighbor_dist, q->max_neighbors, nb);
    for (int k = 0; k < kept; ++k) nb_out[k] = nb[k];
    *kept_out = kept;
    orca_robot_with(*q, nb, kept, n - world * Rn, (uint32_t)n, k0, k1, pose + 3 * (size_t)world * Rn, sc.data(),
                    speed_gt + 2 * (size_t)world * Rn, goal, ranges, hits, beams, bc, bs, act, vel, nullptr, nullptr, diag);
}
"""


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    d = tmp_path_factory.mktemp("orca_big_host")
    src, so = d / "shim.cpp", d / "liborca_big_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    lib.big_rings.argtypes = [C.c_float]
    lib.big_buckets.argtypes = [fp, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.big_neighbours.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_int, ip]
    lib.big_neighbours_hashed.argtypes = [ip, ip, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, ip]
    lib.big_key.argtypes = [C.c_float, C.c_int]
    lib.big_key.restype = C.c_uint64
    lib.big_robot.argtypes = [C.POINTER(Params), ip, ip, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, fp, fp, fp, fp, vp, C.c_int,
                              fp, fp, fp, fp, ip, ip, ip]
    return lib


# ------------------------------------------------------------------------------------------------ the scenes (shared with the GPU test)
LATTICE_COLS, LATTICE_ROWS, LATTICE_PITCH = 20, 15, 0.7


def lattice_xy(cx=0.0, cy=0.0):
    """300 robots, 0.7 m apart, centred on (cx, cy): x in [-6.65, 6.65] crosses the cell borders at -6.5, 0 and 6.5, y in
    [-4.9, 4.9] the one at 0 (where floor changes sign); robot i + 20 * j stands in column i of row j."""
    i, j = np.meshgrid(np.arange(LATTICE_COLS), np.arange(LATTICE_ROWS))
    x = cx + (i - (LATTICE_COLS - 1) / 2.0) * LATTICE_PITCH
    y = cy + (j - (LATTICE_ROWS - 1) / 2.0) * LATTICE_PITCH
    return np.stack([x.ravel(), y.ravel()], 1).astype(f32)


def lattice_poses(seed=11, cx=0.0, cy=0.0):
    """-> (poses f32[300,3] with seeded headings, goals f32[300,2]: the point across the lattice's centre)"""
    xy = lattice_xy(cx, cy)
    th = np.random.default_rng(seed).uniform(-np.pi, np.pi, len(xy)).astype(f32)
    centre = np.array([cx, cy], f32)
    return np.concatenate([xy, th[:, None]], 1).astype(f32), (centre + centre - xy).astype(f32)


def rule_robots(seed=12):
    """The 48 robots of the lattice the whole rule is checked on: the four corners, the edge midpoints, the centre, the robots
    around the points where the cell borders x = -6.5, 0, 6.5 cross the border y = 0 (all robots beside a border would be 110),
    and seeded ones up to 48."""
    at = lambda i, j: i + LATTICE_COLS * j  # noqa: E731
    c, r = LATTICE_COLS, LATTICE_ROWS
    pick = [at(0, 0), at(c - 1, 0), at(0, r - 1), at(c - 1, r - 1), at(c // 2, 0), at(c // 2, r - 1), at(0, r // 2), at(c - 1, r // 2),
            at(c // 2, r // 2)]
    for i in (0, 1, c // 2 - 1, c // 2, c - 2, c - 1):
        for j in (r // 2 - 1, r // 2, r // 2 + 1):
            if at(i, j) not in pick:
                pick.append(at(i, j))
    rng = np.random.default_rng(seed)
    while len(pick) < 48:
        k = int(rng.integers(0, c * r))
        if k not in pick:
            pick.append(k)
    return sorted(pick)


def synthetic_rows(n, beams=64, seed=13):
    """Scan rows of 6.0 m with a few wall returns below obst_dist and a few robot hits: -> (rows f32[n,B], hit bool[n,B])"""
    rng = np.random.default_rng(seed)
    rows = np.full((n, beams), 6.0, f32)
    hit = np.zeros((n, beams), bool)
    for k in range(n):
        for b in rng.choice(beams, 3, replace=False):
            rows[k, b] = f32(rng.uniform(0.5, 2.8))
        for b in rng.choice(beams, 2, replace=False):
            rows[k, b] = f32(rng.uniform(0.4, 2.0))
            hit[k, b] = True
    return rows, hit


# ------------------------------------------------------------------------------------------------ the hash, built on the host
def build_hash(big, pose, Rn, lmask, seed):
    """Counting sort of the robots by bucket, the order inside every bucket shuffled -> (lstart i32[lmask+2], lsorted i32[N])"""
    pose = np.ascontiguousarray(pose, f32)
    N = len(pose)
    bucket, cell = np.zeros(N, np.int32), np.zeros((N, 2), np.int32)
    big.big_buckets(_fp(pose), N, Rn, lmask, _ip(bucket), _ip(cell))
    counts = np.bincount(bucket, minlength=lmask + 1)
    lstart = np.zeros(lmask + 2, np.int32)
    lstart[1:] = np.cumsum(counts)
    rng = np.random.default_rng(seed)
    order = np.lexsort((rng.random(N), bucket))          # by bucket, random inside one
    return lstart, np.ascontiguousarray(order, np.int32), cell


def as_pose(xy):
    return np.ascontiguousarray(np.concatenate([xy, np.zeros((len(xy), 1), f32)], 1), f32)


def hashed(big, h, pose, Rn, n, nd, maxn):
    lstart, lsorted, lmask = h
    out = np.full(48, -1, np.int32)
    k = big.big_neighbours_hashed(_ip(lstart), _ip(lsorted), lmask, _fp(pose), n // Rn, Rn, n, nd, maxn, _ip(out))
    return out[:k].tolist()


def all_pairs(big, xy, local, nd, maxn):
    out = np.full(48, -1, np.int32)
    k = big.big_neighbours(_fp(xy), len(xy), local, nd, maxn, _ip(out))
    return out[:k].tolist()


def check_world(big, xy, nd, maxns, lmask=1023, seed=0, robots=None):
    """hashed == all pairs == orca_ref for the robots of one world (default: all of them)"""
    xy = np.ascontiguousarray(xy, f32)
    pose = as_pose(xy)
    lstart, lsorted, _cell = build_hash(big, pose, len(xy), lmask, seed)
    longest = 0
    for n in (range(len(xy)) if robots is None else robots):
        want_all = R.neighbours(xy, n, nd, 48)          # (the reference sorts and cuts: its list for fewer is this one's head)
        for maxn in maxns:
            want = R.neighbours(xy, n, nd, maxn) if maxn == maxns[-1] else want_all[:maxn]
            assert want == want_all[:maxn]
            assert all_pairs(big, xy, n, nd, maxn) == want, (n, nd, maxn)
            assert hashed(big, (lstart, lsorted, lmask), pose, len(xy), n, nd, maxn) == want, (n, nd, maxn, lmask)
        longest = max(longest, len(want_all))
    return longest


# ------------------------------------------------------------------------------------------------ the selection
def test_ring_count_and_key_order(big):
    nd = [f32(6.3), np.nextafter(f32(6.3), f32(np.inf)), f32(12.8), f32(19.3)]
    assert [big.big_rings(v) for v in nd] == [1, 2, 2, 3]
    assert big.big_rings(np.nextafter(f32(19.3), f32(np.inf))) == 0 and big.big_rings(f32(100.0)) == 0
    assert big.big_rings(f32(0.1)) == 1 and big.big_rings(np.nextafter(f32(12.8), f32(np.inf))) == 3
    # the packed key orders like (dist2, index): float bits of non-negative numbers are monotonic, ties go to the index
    rng = np.random.default_rng(1)
    d2 = np.concatenate([rng.uniform(0, 400, 200), [0.0, 0.0, 1.0, 1.0, 1e-38, 3e38]]).astype(f32)
    idx = rng.integers(0, 500000, len(d2))
    keys = [big.big_key(float(d), int(j)) for d, j in zip(d2, idx)]
    order = sorted(range(len(d2)), key=lambda k: keys[k])
    assert order == sorted(range(len(d2)), key=lambda k: (d2[k], idx[k]))
    assert max(keys) < 0xFFFFFFFFFFFFFFFF


def test_lattice_across_cell_borders(big):
    xy = lattice_xy()
    assert len(xy) == 300 and xy[:, 0].min() < -CELL and xy[:, 0].max() > CELL and xy[:, 1].min() < 0 < xy[:, 1].max()
    _s, _o, cell = build_hash(big, as_pose(xy), 300, 1023, 0)
    assert set(map(tuple, cell)) == {(i, j) for i in (-2, -1, 0, 1) for j in (-1, 0)}
    # every robot's 3 x 3 cells hold more than 64 robots: the kernel needs more than one chunk for each of them
    for cx, cy in set(map(tuple, cell)):
        assert (np.abs(cell[:, 0] - cx) <= 1).sum() > 64 and (np.abs(cell[:, 1] - cy) <= 1).all()
    assert check_world(big, xy, f32(6.0), [0, 1, 10, 48]) == 48


def test_robots_on_a_cell_border_and_one_ulp_off_it(big):
    c, r = LATTICE_COLS, LATTICE_ROWS
    i, j = np.meshgrid(np.arange(c), np.arange(r))
    xy = np.stack([(CELL - LATTICE_PITCH * (c - 1 - i)).ravel(), (-CELL + LATTICE_PITCH * j).ravel()], 1).astype(f32)
    up, down = f32(np.inf), f32(-np.inf)
    col = [c - 1 + c * k for k in range(r)]             # the column at x = 6.5, the row at y = -6.5
    for k, n in enumerate(col):
        xy[n, 0] = [f32(CELL), np.nextafter(f32(CELL), up), np.nextafter(f32(CELL), down)][k % 3]
    for k in range(c):
        xy[k, 1] = [f32(-CELL), np.nextafter(f32(-CELL), up), np.nextafter(f32(-CELL), down)][k % 3]
    xy[c * 9 + 5] = (f32(0.0), f32(0.0))                 # and the border 6.5 * 0 itself, with the smallest normal numbers beside it
    xy[c * 9 + 6] = (np.finfo(f32).tiny, -np.finfo(f32).tiny)
    xy[c * 9 + 7] = (-np.finfo(f32).tiny, np.finfo(f32).tiny)
    _s, _o, cell = build_hash(big, as_pose(xy), 300, 1023, 0)
    assert {cell[col[0], 0], cell[col[1], 0], cell[col[2], 0]} == {0, 1} and {cell[0, 1], cell[1, 1], cell[2, 1]} == {-1, -2}
    assert tuple(cell[c * 9 + 6]) == (0, -1) and tuple(cell[c * 9 + 7]) == (-1, 0)
    check_world(big, xy, f32(6.0), [10, 48], seed=1)
    check_world(big, xy, f32(6.3), [10], seed=2)


def test_heaps_on_one_spot_are_decided_by_index(big):
    rng = np.random.default_rng(3)
    xy = rng.uniform(-8, 8, (100, 2)).astype(f32)
    three, seventy = rng.choice(100, 3, replace=False), None
    rest = np.setdiff1d(np.arange(100), three)
    seventy = rng.choice(rest, 70, replace=False)
    xy[three] = (f32(1.0), f32(1.0))
    xy[seventy] = (f32(3.0), f32(2.0))
    assert check_world(big, xy, f32(6.0), [1, 10, 48], seed=4) == 48
    n = int(seventy[0])                                  # 69 others at distance 0: the 48 lowest indices, in order
    lstart, lsorted, _c = build_hash(big, as_pose(xy), 100, 1023, 5)
    got = hashed(big, (lstart, lsorted, 1023), as_pose(xy), 100, n, f32(6.0), 48)
    assert got == sorted(int(k) for k in seventy if k != n)[:48]


@pytest.mark.parametrize("nd,rings", [(f32(6.3), 1), (np.nextafter(f32(6.3), f32(np.inf)), 2), (f32(12.8), 2), (f32(19.3), 3)])
def test_ring_thresholds_on_random_robots(big, nd, rings):
    assert big.big_rings(nd) == rings
    xy = np.random.default_rng(6).uniform(-30, 30, (400, 2)).astype(f32)
    longest = check_world(big, xy, nd, [10, 48], seed=7)
    assert longest >= 10


@pytest.mark.parametrize("lmask", [0, 1, 3])
def test_every_bucket_aliases(big, lmask):
    xy = lattice_xy()
    check_world(big, xy, f32(6.0), [10, 48], lmask=lmask, seed=8)
    check_world(big, np.random.default_rng(9).uniform(-30, 30, (200, 2)).astype(f32), f32(12.8), [10], lmask=lmask, seed=10)


@pytest.mark.parametrize("lmask", [1023, 1])
def test_two_worlds_laid_over_each_other(big, lmask):
    one = lattice_xy()[:150]
    pose = as_pose(np.concatenate([one, one]))
    lstart, lsorted, _c = build_hash(big, pose, 150, lmask, 11)
    for n in range(300):
        want = R.neighbours(one, n % 150, f32(6.0), 10)
        got = hashed(big, (lstart, lsorted, lmask), pose, 150, n, f32(6.0), 10)
        assert got == want and all(0 <= j < 150 for j in got), n


def test_far_from_the_origin(big):
    xy = lattice_xy(2.5e5, -2.5e5)                       # (an ulp is 1/64 m there: the lattice is what fp32 makes of it)
    assert np.abs(xy).min() > 2.4e5
    check_world(big, xy, f32(6.0), [10, 48], seed=12)
    check_world(big, xy, f32(6.3), [10], seed=13, robots=range(0, 300, 7))
    check_world(big, xy, f32(19.3), [48], seed=14, robots=range(0, 300, 7))


def test_a_robot_with_nobody_in_range(big):
    xy = np.concatenate([lattice_xy()[:80], np.array([[40.0, 40.0], [-300.0, 7.0]], f32)]).astype(f32)
    lstart, lsorted, _c = build_hash(big, as_pose(xy), len(xy), 1023, 15)
    for n in (80, 81):
        assert R.neighbours(xy, n, f32(6.0), 10) == []
        assert hashed(big, (lstart, lsorted, 1023), as_pose(xy), len(xy), n, f32(6.0), 10) == []
        assert all_pairs(big, xy, n, f32(6.0), 10) == []
    assert hashed(big, (lstart, lsorted, 1023), as_pose(xy), len(xy), 0, f32(6.0), 0) == []


# ------------------------------------------------------------------------------------------------ the whole rule
def test_whole_rule_through_the_hash_equals_the_reference(big):
    poses, goals = lattice_poses()
    N, B = len(poses), 64
    rng = np.random.default_rng(14)
    speed_gt = np.stack([rng.uniform(0.0, 1.0, N), rng.uniform(-1.0, 1.0, N)], 1).astype(f32)
    speed_gt[::5, 0] = 0.0
    rows, hit = synthetic_rows(N, B)
    hits = pack_hits(hit)
    bc, bs = (np.ascontiguousarray(t, f32) for t in U.O.beam_table(f32, B))
    s, c = U.O.sincos(poses[:, 2], f32)
    sincos = np.stack([s, c], 1).astype(f32)
    lstart, lsorted, _c = build_hash(big, poses, N, 1023, 16)
    seed = (7 << 32) | 5
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    seen, lp3, static = set(), 0, 0
    for p in (R.params(), R.params(max_neighbors=48, jitter=0.2, neighbor_dist=12.8)):
        q = cparams(p)
        for n in rule_robots():
            act, vel, diag = np.zeros(2, f32), np.zeros(2, f32), np.zeros(3, np.int32)
            nb, kept = np.zeros(48, np.int32), C.c_int(0)
            big.big_robot(C.byref(q), _ip(lstart), _ip(lsorted), 1023, N, n, k0, k1, _fp(poses), _fp(speed_gt), _fp(goals[n]),
                          _fp(rows[n]), hits[n].ctypes.data, B, _fp(bc), _fp(bs), _fp(act), _fp(vel), _ip(diag), _ip(nb),
                          C.byref(kept))
            wcmd, wvel, d = R.robot(p, n, n, k0, k1, poses, sincos, speed_gt, goals[n], rows[n], hit[n], bc, bs)
            assert same_bits(wcmd, act) and same_bits(wvel, vel), (n, wcmd, act, wvel, vel)
            assert (bool(diag[0]), bool(diag[1])) == (d["lp2_short"], d["lp3_changed"])
            assert kept.value == len(d["branches"]) - d["n_static"]
            seen |= set(d["branches"][d["n_static"]:])
            lp3 += d["lp3_changed"]
            static += d["n_static"] > 0
    assert R.CIRCLE in seen and (R.LEG_LEFT in seen or R.LEG_RIGHT in seen), seen
    assert lp3 >= 1 and static >= 1
