"""The ORCA baseline controller's rule (csrc/mrca_orca_device.h) compiled for the host with g++ -ffp-contract=off: the very
functions the gfx950 kernel calls, held EQUAL bit for bit to the NumPy float32 restatement of tests/orca_ref.py (constraint
construction, LP1 / LP2 / LP3, sector reduction, neighbour ranking, command mapping -- with the coverage of the branches
asserted from the diagnostics, not hoped for), checked against brute force for what a linear program promises, and driven in
closed loop on the C oracle's env: the three behaviour gates of the controller's defaults.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orca_cases as K
import orca_ref as R
import util as U
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include "mrca_orca_device.h"
using namespace mrca;
extern "C" void shim_constraint(int n, const float* in, const float* resp, float* lines, int* branch) {
    for (int i = 0; i < n; ++i) {
        const float* a = in + 8 * i;
        OrcaLine l;
        branch[i] = orca_constraint(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], resp[i], &l);
        lines[4 * i] = l.px; lines[4 * i + 1] = l.py; lines[4 * i + 2] = l.dx; lines[4 * i + 3] = l.dy;
    }
}
extern "C" int shim_lp1(const float* lines, int k, float ms, float ox, float oy, int dir_opt, float* res) {
    return orca_lp1(reinterpret_cast<const OrcaLine*>(lines), k, ms, ox, oy, dir_opt != 0, res, res + 1, nullptr);
}
extern "C" int shim_lp2(const float* lines, int n, float ms, float ox, float oy, int dir_opt, float* res) {
    return orca_lp2(reinterpret_cast<const OrcaLine*>(lines), n, ms, ox, oy, dir_opt != 0, res, res + 1, nullptr);
}
extern "C" void shim_solve(const float* lines, int n, int n_static, float ms, float ox, float oy, float* res, int* diag) {
    orca_solve(reinterpret_cast<const OrcaLine*>(lines), n, n_static, ms, ox, oy, res, res + 1, diag);
}
extern "C" void shim_sectors(const float* ranges, const unsigned long long* hits, int beams, float obst_dist, float* r, int* b) {
    orca_sectors(ranges, hits, beams, obst_dist, r, b);
}
extern "C" int shim_neighbours(const float* xy, int Rn, int local, float nd, int maxn, int* out) {
    return orca_neighbours(xy, Rn, local, nd, maxn, out);
}
extern "C" void shim_command(float vx, float vy, float s, float c, float ms, float ko, float* out) {
    orca_command(vx, vy, s, c, ms, ko, out, out + 1);
}
extern "C" void shim_pref(const OrcaParams* q, uint32_t gid, uint32_t k0, uint32_t k1, float px, float py, float gx, float gy, float* out) {
    orca_pref_velocity(*q, gid, k0, k1, px, py, gx, gy, out, out + 1);
}
// every robot of an env from host copies of its fields; the head record is sincos_det of the stored heading
// diag[N][3] as orca_solve's; lines / counts (or NULL): [N][64][4] and [N][2]
extern "C" void shim_env(const OrcaParams* q, int N, int Rn, uint32_t k0, uint32_t k1, const float* pose, const float* speed_gt,
                         const float* goal, const float* rows, const unsigned long long* hits, int beams, const float* bc,
                         const float* bs, float* act, float* vel, int* diag, float* lines, int* counts) {
    float sc[2 * kOrcaMaxRobots];
    for (int w = 0; w < N / Rn; ++w) {
        for (int j = 0; j < Rn; ++j) sincos_det(pose[3 * (w * Rn + j) + 2], &sc[2 * j], &sc[2 * j + 1]);
        for (int j = 0; j < Rn; ++j) {
            const int n = w * Rn + j;
            orca_robot(*q, Rn, j, (uint32_t)n, k0, k1, pose + 3 * w * Rn, sc, speed_gt + 2 * w * Rn, goal + 2 * n,
                       rows + (size_t)n * beams, hits + (size_t)n * (beams / 64), beams, bc, bs, act + 2 * n, vel + 2 * n,
                       lines ? reinterpret_cast<OrcaLine*>(lines) + (size_t)n * kOrcaMaxLines : nullptr,
                       counts ? counts + 2 * n : nullptr, diag + 3 * n);
        }
    }
}
"""


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in R.FIELDS[:-1]] + [("max_neighbors", C.c_int32)]


def cparams(p):
    return Params(**{k: (int(v) if k == "max_neighbors" else float(v)) for k, v in p.items()})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("orca_host")
    src, so = d / "shim.cpp", d / "liborca_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    lib.shim_constraint.argtypes = [C.c_int, fp, fp, fp, ip]
    lib.shim_lp1.argtypes = [fp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, fp]
    lib.shim_lp2.argtypes = [fp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, fp]
    lib.shim_solve.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp, ip]
    lib.shim_sectors.argtypes = [fp, vp, C.c_int, C.c_float, fp, ip]
    lib.shim_neighbours.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_int, ip]
    lib.shim_command.argtypes = [C.c_float] * 6 + [fp]
    lib.shim_pref.argtypes = [C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_float] * 4 + [fp]
    lib.shim_env.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_uint32, C.c_uint32, fp, fp, fp, fp, vp, C.c_int, fp, fp, fp, fp, ip,
                             fp, ip]
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, f32)), bits(np.asarray(b, f32)))


def pack_hits(hit):
    """bool[N,B] -> u64[N,B/64]: bit (b & 63) of word b >> 6"""
    return np.ascontiguousarray(np.packbits(np.asarray(hit, bool), axis=-1, bitorder="little")).view(np.uint64)


def host_env_actions(shim, p, Rn, seed, pose, speed_gt, goal, rows, hit, want_lines=False):
    N, B = rows.shape
    bc, bs = (np.ascontiguousarray(t, f32) for t in U.O.beam_table(f32, B))
    pose, speed_gt, goal, rows = (np.ascontiguousarray(t, f32) for t in (pose, speed_gt, goal, rows))
    hits = pack_hits(hit)
    act, vel, diag = np.zeros((N, 2), f32), np.zeros((N, 2), f32), np.zeros((N, 3), np.int32)
    lines = np.zeros((N, 64, 4), f32) if want_lines else None
    counts = np.zeros((N, 2), np.int32) if want_lines else None
    q = cparams(p)
    shim.shim_env(C.byref(q), N, Rn, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, _fp(pose), _fp(speed_gt), _fp(goal), _fp(rows),
                  hits.ctypes.data, B, _fp(bc), _fp(bs), _fp(act), _fp(vel), _ip(diag), None if lines is None else _fp(lines),
                  None if counts is None else _ip(counts))
    return act, vel, diag, lines, counts


# ------------------------------------------------------------------------------------------------ equality with orca_ref
def constraint_cases(rng):
    """[rpx, rpy, rvx, rvy, vx, vy, R, inv_t] per row: random pairs near and far, discs that overlap, two robots on one spot with
    and without a relative velocity (|w| = 0), velocities straight at and straight away from the other."""
    n = 400
    rp = rng.uniform(-4, 4, (n, 2))
    rp[:60] *= 0.1                                       # many overlaps
    v = rng.uniform(-1, 1, (n, 2))
    vj = rng.uniform(-1, 1, (n, 2))
    vj[::7] = 0.0                                        # static points: V_j = 0
    a = np.concatenate([rp, v - vj, v, rng.choice([0.35, 0.7], (n, 1)), rng.choice([0.25, 1 / 1.5, 2.0], (n, 1))], 1)
    special = [[0, 0, 0, 0, 0.3, 0.1, 0.7, 0.25], [0, 0, 0.5, -0.2, 0.5, -0.2, 0.7, 0.25], [2, 0, 1, 0, 1, 0, 0.7, 0.25],
               [2, 0, -1, 0, -1, 0, 0.7, 0.25], [0.7, 0, 0, 0, 0, 0, 0.7, 0.25], [1e-3, -1e-3, 0.01, 0.01, 0, 0, 0.35, 2.0]]
    return np.ascontiguousarray(np.concatenate([a, np.array(special)]), f32)


def test_constraints_equal_the_reference_and_take_every_branch(shim):
    a = constraint_cases(np.random.default_rng(1))
    resp = np.ascontiguousarray(np.where(np.arange(len(a)) % 7 == 0, 1.0, 0.5), f32)
    lines, branch = np.zeros((len(a), 4), f32), np.zeros(len(a), np.int32)
    shim.shim_constraint(len(a), _fp(a), _fp(resp), _fp(lines), _ip(branch))
    seen = set()
    with np.errstate(all="ignore"):
        for i, row in enumerate(a):
            want, br = R.constraint(*row, resp[i])
            assert br == branch[i] and same_bits(want, lines[i]), (i, row, want, lines[i])
            seen.add(br)
    assert seen == {R.CIRCLE, R.LEG_LEFT, R.LEG_RIGHT, R.OVERLAP}
    assert np.isfinite(lines).all()                     # |w| = 0 took unitW = (1, 0): no NaN
    assert np.abs(np.hypot(lines[:, 2], lines[:, 3]) - 1.0).max() < 1e-5


def random_lines(rng, n, n_static, feasible):
    """n lines, the first n_static of them with the origin strictly inside (static constraints that can all hold).  feasible:
    every line keeps a common point inside; otherwise random half planes, most sets of more than a few then conflict."""
    th = rng.uniform(-np.pi, np.pi, n)
    d = np.stack([np.cos(th), np.sin(th)], 1)
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)              # the permitted side: p + t * nrm, t >= 0
    q = rng.uniform(-0.4, 0.4, 2) if feasible else None
    p = np.zeros((n, 2))
    for i in range(n):
        if i < n_static:
            p[i] = -nrm[i] * rng.uniform(0.05, 0.6) + d[i] * rng.uniform(-1, 1)
        elif feasible:
            p[i] = q - nrm[i] * rng.uniform(0.0, 0.8) + d[i] * rng.uniform(-1, 1)
        else:
            p[i] = rng.uniform(-0.9, 0.9, 2)
    lines = np.concatenate([p, d], 1).astype(f32)
    ln = np.sqrt(lines[:, 2] * lines[:, 2] + lines[:, 3] * lines[:, 3])
    lines[:, 2] /= ln
    lines[:, 3] /= ln
    return np.ascontiguousarray(lines)


def line_sets():
    """(lines, n_static, opt) cases: 1 to 40 lines, feasible and infeasible, with and without static lines, parallel pairs."""
    rng = np.random.default_rng(7)
    out = []
    for n in list(range(1, 41)) + [5, 9, 17, 26, 40] * 3:
        for feasible in (True, False):
            ns = int(rng.integers(0, min(n, 16) + 1)) if rng.random() < 0.6 else 0
            out.append((random_lines(rng, n, ns, feasible), ns, rng.uniform(-1.3, 1.3, 2).astype(f32)))
    # antiparallel pairs that exclude each other (vy >= 0.3 and vy <= -0.3), alone and among others; and a parallel pair that agrees
    pair = np.array([[0, 0.3, 1, 0], [0, -0.3, -1, 0]], f32)
    agree = np.array([[0, 0.3, 1, 0], [0, 0.5, 1, 0]], f32)
    out.append((pair, 0, np.array([0.2, 0.0], f32)))
    out.append((pair[::-1].copy(), 0, np.array([0.2, 0.0], f32)))
    out.append((agree, 0, np.array([0.2, 0.0], f32)))
    out.append((np.concatenate([random_lines(rng, 6, 2, True), pair, random_lines(rng, 4, 0, True)]), 2, np.array([0.5, 0.5], f32)))
    out.append((np.concatenate([pair[:1], random_lines(rng, 3, 0, True), pair[1:]]), 1, np.array([-0.5, 0.1], f32)))
    return out


def as_tuples(lines):
    return [tuple(f32(v) for v in row) for row in lines]


def test_solve_equals_the_reference_with_every_outcome(shim):
    seen = {"ok": 0, "short": 0, "changed": 0, "parallel": 0, "static_short": 0}
    for lines, ns, opt in line_sets():
        n = len(lines)
        res, diag = np.zeros(2, f32), np.zeros(3, np.int32)
        shim.shim_solve(_fp(lines), n, ns, 1.0, opt[0], opt[1], _fp(res), _ip(diag))
        (rx, ry), d = R.solve(as_tuples(lines), ns, 1.0, opt[0], opt[1])
        assert same_bits([rx, ry], res), (n, ns, opt, (rx, ry), res)
        assert (bool(diag[0]), bool(diag[1]), int(diag[2])) == (d["lp2_short"], d["lp3_changed"], d["parallel_fail"])
        seen["ok"] += not d["lp2_short"]
        seen["short"] += d["lp2_short"]
        seen["changed"] += d["lp3_changed"]
        seen["parallel"] += d["parallel_fail"] > 0
        seen["static_short"] += bool(d["lp2_short"] and ns > 0)
        # LP1 and LP2 on their own, both optimisation modes, on every prefix end
        for dir_opt in (0, 1):
            o = opt if not dir_opt else (opt / np.sqrt(opt[0] * opt[0] + opt[1] * opt[1])).astype(f32)
            got = np.zeros(2, f32)
            k = shim.shim_lp2(_fp(lines), n, 1.0, o[0], o[1], dir_opt, _fp(got))
            with np.errstate(all="ignore"):
                wk, wres = R.lp2(as_tuples(lines), f32(1.0), o[0], o[1], bool(dir_opt))
            assert k == wk and same_bits(wres, got)
            got1 = np.zeros(2, f32)
            ok = shim.shim_lp1(_fp(lines), n - 1, 1.0, o[0], o[1], dir_opt, _fp(got1))
            with np.errstate(all="ignore"):
                wok, wres1, _par = R.lp1(as_tuples(lines), n - 1, f32(1.0), o[0], o[1], bool(dir_opt))
            assert bool(ok) == wok and (not wok or same_bits(wres1, got1))
    assert min(seen.values()) > 0, seen                  # a success, an LP2 that fell short, an LP3 that moved, a parallel failure


def test_lp2_against_brute_force(shim):
    """Where LP2 succeeds: every line holds within 1e-5, the point lies in the disc within 1e-6 relative, and no point of a
    201 x 201 grid over the disc that satisfies all lines is closer to opt by more than the grid's pitch."""
    g = np.linspace(-1.0, 1.0, 201)
    gx, gy = np.meshgrid(g, g)
    pitch = g[1] - g[0]
    checked = 0
    for lines, _ns, opt in line_sets():
        res = np.zeros(2, f32)
        if shim.shim_lp2(_fp(lines), len(lines), 1.0, opt[0], opt[1], 0, _fp(res)) < len(lines):
            continue
        L = lines.astype(np.float64)
        r = res.astype(np.float64)
        viol = L[:, 2] * (L[:, 1] - r[1]) - L[:, 3] * (L[:, 0] - r[0])
        assert viol.max() <= 1e-5, (viol.max(), lines)
        assert np.hypot(*r) <= 1.0 * (1 + 1e-6)
        ok = gx * gx + gy * gy <= 1.0
        for px, py, dx, dy in L:
            ok &= dx * (py - gy) - dy * (px - gx) <= 0.0
        if ok.any():
            best = np.hypot(gx[ok] - opt[0], gy[ok] - opt[1]).min()
            assert np.hypot(r[0] - opt[0], r[1] - opt[1]) <= best + pitch, (best, r, opt)
        checked += 1
    assert checked >= 40


def test_lp3_keeps_static_lines_hard(shim):
    ran = 0
    for lines, ns, opt in line_sets():
        res, diag = np.zeros(2, f32), np.zeros(3, np.int32)
        shim.shim_solve(_fp(lines), len(lines), ns, 1.0, opt[0], opt[1], _fp(res), _ip(diag))
        if not diag[0] or ns == 0:
            continue
        L, r = lines[:ns].astype(np.float64), res.astype(np.float64)
        viol = L[:, 2] * (L[:, 1] - r[1]) - L[:, 3] * (L[:, 0] - r[0])
        assert viol.max() <= 1e-5, (viol, lines, ns)
        ran += 1
    assert ran >= 5


def test_sector_reduction_with_ties_and_empty_rows(shim):
    rng = np.random.default_rng(3)
    for B in (64, 192, 512, 1024):
        rows = K.sector_rows(rng, B)                      # (tests/orca_cases.py)
        for obst in (3.0, 6.0, 0.0):
            for r, hit in rows:
                br, bb = np.zeros(16, f32), np.zeros(16, np.int32)
                hw = pack_hits(hit[None])[0]
                shim.shim_sectors(_fp(r), hw.ctypes.data, B, obst, _fp(br), _ip(bb))
                want = R.sectors(r, hit, f32(obst))
                assert [b for _r, b in want] == bb.tolist()
                assert all(b < 0 or same_bits(wr, br[s]) for s, (wr, b) in enumerate(want))
    K.sector_expectations(rows, B)                        # the tie went to the lower beam; a row of 6.0 gives nothing


def test_neighbour_ranking_with_equal_distances(shim):
    rng = np.random.default_rng(5)
    for Rn in (1, 2, 7, 33, 64):
        xy = rng.uniform(-5, 5, (Rn, 2)).astype(f32)
        if Rn >= 7:
            K.place_ties(xy)                              # two on one spot; equal distances from robot 0, four ways
        for local in range(0, Rn, max(1, Rn // 5)):
            for maxn, nd in [(10, 6.0), (48, 6.0), (3, 100.0), (0, 6.0), (48, 0.5)]:
                out = np.full(48, -1, np.int32)
                n = shim.shim_neighbours(_fp(xy), Rn, local, nd, maxn, _ip(out))
                want = R.neighbours(xy, local, nd, maxn)
                assert out[:n].tolist() == want, (Rn, local, maxn, nd)
    K.tie_expectations(xy)                                # equal distances: by index


def test_command_mapping_and_preferred_velocity(shim):
    rng = np.random.default_rng(9)
    cases = list(K.COMMAND_CASES)
    for _ in range(200):
        th = rng.uniform(-np.pi, np.pi)
        cases.append((*rng.uniform(-1.2, 1.2, 2), np.sin(th), np.cos(th)))
    kinds = set()
    for vx, vy, s, c in cases:
        for ms, ko in [(1.0, 2.0), (0.6, 0.5)]:
            out = np.zeros(2, f32)
            shim.shim_command(vx, vy, s, c, ms, ko, _fp(out))
            with np.errstate(all="ignore"):
                want = R.command(vx, vy, s, c, ms, ko)
            assert same_bits(want, out), (vx, vy, s, c)
            assert 0.0 <= out[0] <= ms and -1.0 <= out[1] <= 1.0
            fwd, lat = f32(c) * f32(vx) + f32(s) * f32(vy), f32(c) * f32(vy) - f32(s) * f32(vx)
            kinds.add("still" if np.hypot(vx, vy) < 1e-4 else ("back" if fwd <= 0 else ("straight" if lat == 0 else "turn")))
    assert kinds == K.COMMAND_KINDS
    for jitter in (0.0, 0.1, 0.5):
        q = R.params(jitter=jitter, v_pref=0.8)
        cq = cparams(q)
        for gid in (0, 1, 7, 4099):
            for px, py, gx, gy in [(0, 0, 3, 4), (1, 1, 1.2, 1.3), (-5, 2, 6, -1), (0, 0, 0.5, 0)]:
                out = np.zeros(2, f32)
                shim.shim_pref(C.byref(cq), gid, 11, 22, px, py, gx, gy, _fp(out))
                with np.errstate(all="ignore"):
                    want = R.pref_velocity(q, gid, 11, 22, px, py, gx, gy)
                assert same_bits(want, out), (jitter, gid, want, out)
    out = np.zeros(2, f32)
    q0 = cparams(R.params(v_pref=1.0))
    shim.shim_pref(C.byref(q0), 3, 1, 2, 0, 0, 3, 4, _fp(out))
    assert same_bits(out, [f32(3.0) / f32(5.0), f32(4.0) / f32(5.0)])       # jitter 0: no rotation at all


@pytest.mark.parametrize("robots,beams", [(34, 64), (34, 192), (64, 1024)])
def test_the_device_world_stands_on_every_edge(shim, robots, beams):
    """``orca_cases.device_world`` -- the crafted inputs above as ONE world, which tests/test_gpu_orca.py and
    tests/test_gpu_orca_big.py put into an env -- through the whole rule: host build == restatement, and every edge occurs"""
    pose, speed_gt, goal, rows, hit = K.world_arrays(robots, beams)
    for p in K.device_params():
        act, vel, _d, _l, _c = host_env_actions(shim, p, robots, 5, pose, speed_gt, goal, rows, hit)
        wact, wvel, diags = R.env_actions(p, robots, 5, pose, speed_gt, goal, rows, hit)
        assert same_bits(wact, act) and same_bits(wvel, vel)
        K.device_expectations(p, 0, beams, pose, speed_gt, goal, rows, hit, diags)


# ------------------------------------------------------------------------------------------------ closed loop on the C oracle
def closed_loop(shim, sc, p, ticks, poses=None, goals=None, check=None):
    env = U.COracleEnv(sc)
    env.reset(None, poses, goals)
    for k in range(ticks):
        act, vel, diag, lines, counts = host_env_actions(shim, p, sc.robots_per_world, sc.seed, env.pose, env.speed_gt, env.goal,
                                                         env.scan, env.hit_robot, want_lines=check is not None)
        if check is not None:
            check(k, env, vel, lines, counts)
        env.step(act)
        if (env.first_result != 0).all():
            break
    return env


def test_whole_robot_equals_the_reference_in_a_walled_world(shim):
    """The full rule (scan row -> sectors -> static lines, neighbours -> robot lines, solve, command) on an env's fields."""
    occ = np.zeros((40, 40), bool)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = True
    occ[8:11, 25:33] = occ[28:34, 6:8] = True
    sc = S.stage1(num_worlds=2, robots_per_world=5, seed=(9 << 32) | 4, grid=S.GridData.from_dense(occ, 0.5, -10.0, -10.0))
    sc.beams, sc.frames = 64, 1
    env = U.COracleEnv(sc)
    rng = np.random.default_rng(4)
    poses = np.concatenate([rng.uniform(-7, 7, (10, 2)), rng.uniform(-np.pi, np.pi, (10, 1))], 1).astype(f32)
    poses[1, :2] = poses[0, :2] + f32(0.3)
    poses[3] = (-8.9, 0.0, np.pi)                        # 0.6 m from the wall at x = -9.5, facing it
    env.reset(None, poses, rng.uniform(-7, 7, (10, 2)).astype(f32))
    for _ in range(4):
        env.step(U.random_actions(rng, 10))
    for p in (R.params(), R.params(jitter=0.3, max_neighbors=2, obst_dist=6.0)):
        act, vel, diag, _l, _c = host_env_actions(shim, p, 5, sc.seed, env.pose, env.speed_gt, env.goal, env.scan, env.hit_robot)
        wact, wvel, wd = R.env_actions(p, 5, sc.seed, env.pose, env.speed_gt, env.goal, env.scan, env.hit_robot.astype(bool))
        assert same_bits(wact, act) and same_bits(wvel, vel)
        assert any(d["n_static"] > 0 for d in wd.values())


def test_gate_two_robots_pass_each_other(shim):
    sc = S.circle_n(2, 4.0, grid=S.empty_grid())
    poses = np.asarray(sc.init_table, f32).copy()
    poses[1, 1] += f32(0.2)                              # 0.2 m off the axis
    env = closed_loop(shim, sc, R.params(), 300, poses, np.asarray(sc.goal_table, f32))
    assert (env.first_result == 1).all() and not env.crashed.any(), (env.first_result, env.pose)


def test_gate_one_robot_never_hits_the_block(shim):
    # a 1 m wide block (y in [-0.5, 0.5]) across the way; the robot drives along y = 0.4, its goal 3 m behind the block
    grid = U.small_grid(blocks=[(0.0, -0.5, 0.5, 0.5)])
    sc = S.circle_n(1, 4.0, grid=grid)
    active = []

    def check(k, env, vel, lines, counts):
        ns = counts[0, 1]
        if ns:
            L, r = lines[0, :ns].astype(np.float64), vel[0].astype(np.float64)
            viol = L[:, 2] * (L[:, 1] - r[1]) - L[:, 3] * (L[:, 0] - r[0])
            assert viol.max() <= 1e-5, (k, viol.max())
            active.append(k)
    env = closed_loop(shim, sc, R.params(), 400, np.array([[-3.0, 0.4, 0.0]], f32), np.array([[3.5, 0.4]], f32), check)
    assert not env.crashed.any() and env.first_result[0] != 2
    assert len(active) > 10                              # the block was seen


def test_gate_four_robots_cross(shim):
    sc = S.circle_n(4, 3.0, grid=S.empty_grid())
    env = closed_loop(shim, sc, R.params(jitter=0.1), 400)
    assert (env.first_result == 1).all() and not env.crashed.any(), (env.first_result, env.pose)


# ------------------------------------------------------------------------------------------------ the library's own defaults
def test_default_params_and_their_validation(built_lib):
    from mrca import _lib
    from mrca.orca import OrcaParams
    assert built_lib.mrca_orca_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.OrcaParamsStruct()
    assert built_lib.mrca_orca_default_params(C.byref(st)) == 0
    got = {k: getattr(st, k) for k in R.FIELDS}
    assert got == {k: (v if k == "max_neighbors" else float(f32(v))) for k, v in R.DEFAULTS.items()}
    assert [n for n, _t in _lib.OrcaParamsStruct._fields_] == R.FIELDS and C.sizeof(st) == 44
    p = OrcaParams(radius=0.4)
    assert p.radius == 0.4 and p.max_neighbors == 10 and p.struct().time_horizon == 2.0
    assert OrcaParams.from_assignments(["jitter=0.1", "max_neighbors=12"]).max_neighbors == 12
    with pytest.raises(ValueError):
        OrcaParams.from_assignments(["nonsense=1"])
    # what can be judged without an env is judged before the env is looked at
    assert built_lib.mrca_orca_actions(None, None, None, C.c_void_p(0x1000), None, None) == -1
    assert b"env is NULL" in built_lib.mrca_last_error()
    assert built_lib.mrca_orca_actions(None, None, None, None, None, None) == -1 and b"actions_dev" in built_lib.mrca_last_error()
    bad = _lib.OrcaParamsStruct()
    built_lib.mrca_orca_default_params(C.byref(bad))
    bad.radius = float("nan")
    assert built_lib.mrca_orca_actions(None, C.byref(bad), None, C.c_void_p(0x1000), None, None) == -1
    assert b"radius" in built_lib.mrca_last_error()
