"""The NH-ORCA baseline controller's rule (csrc/mrca_nhorca_device.h) compiled for the host with g++ -ffp-contract=off: the very
functions the gfx950 kernel calls, held EQUAL bit for bit to the NumPy float32 restatement of tests/nhorca_ref.py (derived values,
atan2_approx, heading lines, the two solves, the command, the modes -- every mode asserted to occur), checked for what the rule
promises (the tracked velocity lies in the cone and the disc; the unicycle that follows the command stays within track_error of
it), and driven in closed loop on the C oracle's env with the library's defaults: the four behaviour gates.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import nhorca_ref as NR
import orca_cases as K
import orca_ref as R
import util as U
from orca_cases import crafted_solves  # noqa: F401  (the crafted solves live in tests/orca_cases.py)
from test_orca_host import CSRC, _fp, _ip, as_tuples, bits, line_sets, pack_hits, same_bits  # noqa: F401
from util import S

f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include "mrca_nhorca_device.h"
using namespace mrca;
extern "C" float shim_atan2(float y, float x) { return atan2_approx(y, x); }
extern "C" void shim_derive(const NhOrcaParams* q, float* out) {
    const NhOrcaDerived d = nhorca_derive(*q);
    out[0] = d.sm; out[1] = d.cm; out[2] = d.u_cap; out[3] = d.radius;
}
extern "C" void shim_heading(float s, float c, float sm, float cm, float* out) {
    nhorca_heading_lines(s, c, sm, cm, reinterpret_cast<OrcaLine*>(out), reinterpret_cast<OrcaLine*>(out) + 1);
}
extern "C" int shim_command(float x, float y, float s, float c, int track, float turn, float ms, float T, float* out) {
    return nhorca_command(x, y, s, c, track != 0, turn, ms, T, out, out + 1);
}
// lines[n]: the static ones, then the robots' (the heading lines are put in front here) -> the mode; out: cmd, S2, S1
extern "C" int shim_solve(const NhOrcaParams* q, const float* lines, int n, int n_static, float s, float c, float ox, float oy,
                          float* out) {
    OrcaLine all[kOrcaMaxLines];
    const NhOrcaDerived d = nhorca_derive(*q);
    nhorca_heading_lines(s, c, d.sm, d.cm, &all[0], &all[1]);
    for (int k = 0; k < n; ++k) all[kNhHeadingLines + k] = reinterpret_cast<const OrcaLine*>(lines)[k];
    return nhorca_solve(*q, d, all, n + kNhHeadingLines, n_static, s, c, ox, oy, out, out + 2, out + 4, nullptr);
}
// every robot of an env from host copies of its fields; the head record is sincos_det of the stored heading
// lines / counts (or NULL): [N][64][4] and [N][2]
extern "C" void shim_env(const NhOrcaParams* q, int N, int Rn, uint32_t k0, uint32_t k1, const float* pose, const float* speed_gt,
                         const float* goal, const float* rows, const unsigned long long* hits, int beams, const float* bc,
                         const float* bs, float* act, float* vel, int* mode, float* s1, float* lines, int* counts) {
    float* sc = new float[2 * Rn];
    for (int w = 0; w < N / Rn; ++w) {
        for (int j = 0; j < Rn; ++j) sincos_det(pose[3 * (w * Rn + j) + 2], &sc[2 * j], &sc[2 * j + 1]);
        for (int j = 0; j < Rn; ++j) {
            const int n = w * Rn + j;
            mode[n] = nhorca_robot(*q, Rn, j, (uint32_t)n, k0, k1, pose + 3 * w * Rn, sc, speed_gt + 2 * w * Rn, goal + 2 * n,
                                   rows + (size_t)n * beams, hits + (size_t)n * (beams / 64), beams, bc, bs, act + 2 * n, vel + 2 * n,
                                   s1 + 2 * n, lines ? reinterpret_cast<OrcaLine*>(lines) + (size_t)n * kOrcaMaxLines : nullptr,
                                   counts ? counts + 2 * n : nullptr, nullptr);
        }
    }
    delete[] sc;
}
"""


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in R.FIELDS[:-1]] + [("max_neighbors", C.c_int32), ("track_error", C.c_float), ("track_time", C.c_float)]


def cparams(p):
    return Params(**{k: (int(v) if k == "max_neighbors" else float(v)) for k, v in p.items()})


@pytest.fixture(scope="module")
def nhshim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("nhorca_host"))


def build_shim(d):
    """the host build in directory ``d`` (a pathlib.Path) -> the loaded library (tools/nhorca_defaults.py sweeps with it)"""
    src, so = d / "shim.cpp", d / "libnhorca_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip, vp, pp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(Params)
    lib.shim_atan2.argtypes, lib.shim_atan2.restype = [C.c_float, C.c_float], C.c_float
    lib.shim_derive.argtypes = [pp, fp]
    lib.shim_heading.argtypes = [C.c_float] * 4 + [fp]
    lib.shim_command.argtypes = [C.c_float] * 4 + [C.c_int] + [C.c_float] * 3 + [fp]
    lib.shim_solve.argtypes = [pp, fp, C.c_int, C.c_int] + [C.c_float] * 4 + [fp]
    lib.shim_env.argtypes = [pp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, fp, fp, fp, fp, vp, C.c_int, fp, fp, fp, fp, ip, fp, fp, ip]
    return lib


def host_env_actions(nhshim, p, Rn, seed, pose, speed_gt, goal, rows, hit, want_lines=False):
    """-> (act, vel, mode, s1, lines, counts) of the host build for every robot of an env"""
    N, B = rows.shape
    bc, bs = (np.ascontiguousarray(t, f32) for t in U.O.beam_table(f32, B))
    pose, speed_gt, goal, rows = (np.ascontiguousarray(t, f32) for t in (pose, speed_gt, goal, rows))
    hits = pack_hits(hit)
    act, vel, s1, mode = np.zeros((N, 2), f32), np.zeros((N, 2), f32), np.zeros((N, 2), f32), np.zeros(N, np.int32)
    lines = np.zeros((N, 64, 4), f32) if want_lines else None
    counts = np.zeros((N, 2), np.int32) if want_lines else None
    q = cparams(p)
    nhshim.shim_env(C.byref(q), N, Rn, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, _fp(pose), _fp(speed_gt), _fp(goal), _fp(rows),
                    hits.ctypes.data, B, _fp(bc), _fp(bs), _fp(act), _fp(vel), _ip(mode), _fp(s1), None if lines is None else _fp(lines),
                    None if counts is None else _ip(counts))
    return act, vel, mode, s1, lines, counts


SWEEP = [(eps, T) for eps in (0.05, 0.1, 0.2) for T in (0.3, 0.5, 1.0)]
MODES_SEEN = set()          # across the equality tests below; test_every_mode_occurred reads it


def check_s2(p, s, c, vel, what=""):
    """S2 violates neither heading line by more than 1e-5 and lies in the disc of u_cap"""
    sm, cm, u_cap, _rr = (float(v) for v in NR.derive(p))
    s, c, x, y = float(s), float(c), float(vel[0]), float(vel[1])
    for dx, dy in ((-(c * cm - s * sm), -(s * cm + c * sm)), (c * cm + s * sm, s * cm - c * sm)):
        assert dx * (0.0 - y) - dy * (0.0 - x) <= 1e-5, (what, vel)
    assert np.hypot(x, y) <= u_cap * (1 + 1e-6), (what, vel, u_cap)


# ------------------------------------------------------------------------------------------------ equality with nhorca_ref
def test_atan2_and_derived_values_equal_the_reference(nhshim):
    rng = np.random.default_rng(1)
    pts = rng.uniform(-1.5, 1.5, (500, 2)).astype(f32)
    pts = np.concatenate([pts, np.array([[0, 0], [0, 1], [1, 0], [-1, 0], [0, -1], [1, 1], [-1, 1], [1e-8, 1], [1, 1e-8], [-0.0, -1]], f32)])
    worst = 0.0
    with np.errstate(all="ignore"):
        for y, x in pts:
            got = f32(nhshim.shim_atan2(y, x))
            assert same_bits(NR.atan2_approx(y, x), got), (y, x)
            d = float(got) - np.arctan2(float(y), float(x))
            worst = max(worst, abs(np.arctan2(np.sin(d), np.cos(d))))          # (as angles: y = -0 behind the robot is +pi here)
    # what the tracking test below can afford: its 1e-3 m over at most 1.5 m of arc is 6.7e-4 rad (measured here: 2.0e-4 rad,
    # near |y| = |x| -- more than the 1.2e-4 the comment in mrca_device.h states for the polynomial)
    assert worst < 6e-4
    for eps, T in SWEEP + [(0.5, 1.5), (0.5, 0.1), (0.01, 1.5), (0.05, 1.5707964)]:
        for ms in (1.0, 0.6):
            p = NR.params(track_error=eps, track_time=T, max_speed=ms)
            out = np.zeros(4, f32)
            q = cparams(p)
            nhshim.shim_derive(C.byref(q), _fp(out))
            assert same_bits(NR.derive(p), out), (eps, T)
            th_max = min(T, np.pi / 2)
            assert abs(out[2] - min(ms, eps / (T * np.sin(th_max / 2)))) < 1e-5 and abs(out[1] - np.cos(th_max)) < 1e-6
            for h in (0.0, 1.0, -2.5, 3.1):
                s, c = NR.sincos(h)
                hl = np.zeros(8, f32)
                nhshim.shim_heading(s, c, out[0], out[1], _fp(hl))
                left, right = NR.heading_lines(s, c, out[0], out[1])
                assert same_bits(left + right, hl)
                # the cone's inside: a velocity along the heading satisfies both, one behind the robot violates one
                for vx, vy, ok in ((c, s, True), (-c, -s, False), (f32(np.cos(h + 0.9 * th_max)), f32(np.sin(h + 0.9 * th_max)), True),
                                   (f32(np.cos(h + th_max + 0.1)), f32(np.sin(h + th_max + 0.1)), False),
                                   (f32(np.cos(h - th_max - 0.1)), f32(np.sin(h - th_max - 0.1)), False)):
                    viol = max(R.violation(l, f32(0.5) * vx, f32(0.5) * vy) for l in (left, right))
                    assert (viol <= 1e-6) == ok, (h, T, vx, vy, viol)


def run_solve(nhshim, p, lines, ns, h, o):
    """one set of lines through the host build and through nhorca_ref, compared -> (mode, S2, diag)"""
    s, c = NR.sincos(h)
    L = np.ascontiguousarray(np.asarray(lines, f32).reshape(-1, 4))
    out = np.zeros(6, f32)
    q = cparams(p)
    mode = nhshim.shim_solve(C.byref(q), _fp(L) if len(L) else None, len(L), ns, s, c, o[0], o[1], _fp(out))
    cmd, v, wmode, diag = NR.solve(p, as_tuples(L), ns, s, c, f32(o[0]), f32(o[1]))
    assert mode == wmode and same_bits(cmd, out[:2]) and same_bits(v, out[2:4]) and same_bits(diag["s1"], out[4:]), \
        (lines, h, o, mode, wmode, cmd, out)
    assert 0.0 <= out[0] <= p["max_speed"] and -1.0 <= out[1] <= 1.0
    check_s2(p, s, c, out[2:4], (h, o))
    MODES_SEEN.add(mode)
    return mode, out[2:4].copy(), diag


def test_crafted_cases_take_the_modes_they_are_made_for(nhshim):
    for eps, T in [(0.05, 0.3), (0.2, 1.0), (0.1, 1.5)]:
        p = NR.params(track_error=eps, track_time=T)
        for what, lines, ns, h, o, want in crafted_solves():
            mode, s2, diag = run_solve(nhshim, p, lines, ns, h, o)
            K.solve_expectations(what, want, T, mode, s2, diag, lines)


def test_the_two_solves_equal_the_reference_on_random_lines(nhshim):
    """test_orca_host's line sets (1 to 40 lines, feasible and not, static and robot lines, parallel pairs) under random headings:
    LP3 decides in many of them, with the heading lines among the hard ones."""
    rng = np.random.default_rng(11)
    lp3 = 0
    for eps, T in [(0.05, 0.3), (0.2, 1.0)]:
        p = NR.params(track_error=eps, track_time=T)
        for lines, ns, opt in line_sets():
            _mode, s2, diag = run_solve(nhshim, p, lines, ns, rng.uniform(-np.pi, np.pi), opt)
            lp3 += diag["lp3_changed"]
            if ns:                                       # the static lines (the origin is inside them all) stay hard in the tracked solve
                assert max(R.violation(l, s2[0], s2[1]) for l in as_tuples(lines[:ns])) <= 1e-5
    assert lp3 >= 5


def walled_world():
    """test_orca_host's walled 2 x 5-robot world after four random ticks, 64 beams; robot 6 stands at its goal, robot 7 faces away
    from its goal, robot 8 faces it"""
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
    goal = env.goal.copy()
    goal[6] = env.pose[6, :2] + f32(0.1)
    for n, away in ((7, np.pi), (8, 0.0)):
        th = float(env.pose[n, 2]) + away
        goal[n] = env.pose[n, :2] + f32(4.0) * np.array([np.cos(th), np.sin(th)], f32)
    return sc, env, goal


def test_whole_robot_equals_the_reference_in_a_walled_world(nhshim):
    sc, env, goal = walled_world()
    for p in (NR.params(), NR.params(jitter=0.0), NR.params(jitter=0.3, max_neighbors=2, obst_dist=6.0, track_error=0.2, track_time=1.0)):
        act, vel, mode, s1, _l, _c = host_env_actions(nhshim, p, 5, sc.seed, env.pose, env.speed_gt, goal, env.scan, env.hit_robot)
        wact, wvel, wmode, wd = NR.env_actions(p, 5, sc.seed, env.pose, env.speed_gt, goal, env.scan, env.hit_robot.astype(bool))
        assert same_bits(wact, act) and same_bits(wvel, vel) and np.array_equal(wmode, mode)
        assert same_bits([d["s1"] for d in wd.values()], s1)
        assert any(d["n_static"] > 0 for d in wd.values())
        MODES_SEEN.update(mode.tolist())
        s, c = U.O.sincos(env.pose[:, 2], f32)
        for n in range(10):
            check_s2(p, s[n], c[n], vel[n], n)
        if p["jitter"] == 0.0:
            assert mode[6] == NR.STILL and not act[6].any()              # at its goal, nobody near: o = 0
            assert mode[7] == NR.TURN and act[7, 0] == 0.0 and abs(act[7, 1]) == 1.0
            assert mode[8] == NR.TRACK and act[8, 0] > 0.5


def test_equal_distances_and_a_full_list(nhshim):
    """Seven robots in an open world, four of them at ONE distance from robot 0 and two on one spot; max_neighbors 2 cuts the
    list among equals (by index), 46 is the most the lanes hold."""
    sc = S.circle_n(7, 3.0, grid=S.empty_grid())
    sc.beams, sc.frames = 64, 1
    env = U.COracleEnv(sc)
    poses = K.equal_distance_poses(sc.init_table)
    env.reset(None, poses, np.asarray(sc.goal_table, f32))
    assert R.neighbours(env.pose[:, :2], 0, 6.0, 2) == [2, 4]
    for p in (NR.params(max_neighbors=2), NR.params(max_neighbors=1, jitter=0.0), NR.params(max_neighbors=NR.MAX_NEIGHBORS)):
        act, vel, mode, _s1, _l, counts = host_env_actions(nhshim, p, 7, sc.seed, env.pose, env.speed_gt, env.goal, env.scan, env.hit_robot,
                                                           want_lines=True)
        wact, wvel, wmode, wd = NR.env_actions(p, 7, sc.seed, env.pose, env.speed_gt, env.goal, env.scan, env.hit_robot.astype(bool))
        assert same_bits(wact, act) and same_bits(wvel, vel) and np.array_equal(wmode, mode)
        assert counts[0, 0] == 2 + min(p["max_neighbors"], 6) and counts[0, 1] == 0
        MODES_SEEN.update(mode.tolist())


@pytest.mark.parametrize("robots,beams", [(34, 64), (64, 192)])
def test_the_device_world_takes_the_modes_it_is_made_for(nhshim, robots, beams):
    """``orca_cases.device_world`` (which tests/test_gpu_nhorca.py puts into an env) through the whole rule: host build ==
    restatement, the situations of ``crafted_solves`` it rebuilds take their modes, and all four modes occur"""
    pose, speed_gt, goal, rows, hit = K.world_arrays(robots, beams)
    seen = set()
    for p in K.nh_device_params():
        act, vel, mode, s1, _l, _c = host_env_actions(nhshim, p, robots, 5, pose, speed_gt, goal, rows, hit)
        wact, wvel, wmode, wd = NR.env_actions(p, robots, 5, pose, speed_gt, goal, rows, hit)
        assert same_bits(wact, act) and same_bits(wvel, vel) and np.array_equal(wmode, mode)
        K.device_expectations(dict(p, radius=NR.derive(p)[3]), 0, beams, pose, speed_gt, goal, rows, hit, {n: d["free"] for n, d in wd.items()})
        if p["jitter"] == 0.0:
            K.nh_device_expectations(p, 0, wmode, wd)
        seen |= set(wmode[:K.N_CASES].tolist())
    assert seen == {NR.TRACK, NR.TURN, NR.STILL, NR.EVADE}, seen


def test_every_mode_occurred():
    assert MODES_SEEN == {NR.TRACK, NR.TURN, NR.STILL, NR.EVADE}, MODES_SEEN


# ------------------------------------------------------------------------------------------------ what the rule promises
@pytest.mark.parametrize("eps,T", SWEEP)
def test_the_unicycle_stays_within_track_error_of_the_tracked_velocity(nhshim, eps, T):
    """The fp32 command (v, omega) of a velocity S2 in the cone and the disc, followed exactly (float64) over [0, T], against the
    point that moves at S2: their greatest distance is at most eps + 1e-3 m (atan2_approx's 1.2e-4 rad over at most 1.5 m of arc
    is 2e-4 m; the rest is rounding)."""
    p = NR.params(track_error=eps, track_time=T)
    _sm, _cm, u_cap, _rr = (float(v) for v in NR.derive(p))
    th_max = min(T, np.pi / 2)
    t = np.linspace(0.0, T, 201)
    worst = 0.0
    for h in (0.0, 2.0):
        s, c = NR.sincos(h)
        hs, hc = float(s), float(c)
        for a in np.linspace(-th_max, th_max, 25):
            for frac in (0.05, 0.5, 1.0):
                u = frac * u_cap
                x, y = f32(u * (hc * np.cos(a) - hs * np.sin(a))), f32(u * (hs * np.cos(a) + hc * np.sin(a)))
                out = np.zeros(2, f32)
                mode = nhshim.shim_command(x, y, s, c, 1, 0.0, p["max_speed"], p["track_time"], _fp(out))
                with np.errstate(all="ignore"):
                    want, wmode = NR.command(x, y, s, c, True, 0.0, p["max_speed"], p["track_time"])
                assert mode == wmode == NR.TRACK and same_bits(want, out)
                v, w = float(out[0]), float(out[1])
                assert 0.0 <= v <= 1.0 and abs(w) <= 1.0
                # the arc in the robot's frame (heading along +x), then turned by the heading
                if abs(w) < 1e-9:
                    ax, ay = v * t, 0.0 * t
                else:
                    ax, ay = v / w * np.sin(w * t), v / w * (1.0 - np.cos(w * t))
                wx, wy = hc * ax - hs * ay, hs * ax + hc * ay
                worst = max(worst, float(np.hypot(wx - float(x) * t, wy - float(y) * t).max()))
    assert worst <= eps + 1e-3, (eps, T, worst)
    assert abs(worst - T * u_cap * np.sin(th_max / 2)) <= 1e-3       # the derivation's T u |sin(th/2)|, reached at the cone's edge


# ------------------------------------------------------------------------------------------------ the library's own defaults
@pytest.fixture(scope="module")
def defaults(built_lib):
    """the library's defaults as nhorca_ref's params"""
    from mrca import _lib
    st = _lib.NhOrcaParamsStruct()
    assert built_lib.mrca_nhorca_default_params(C.byref(st)) == 0
    return NR.params(**{k: getattr(st, k) for k in NR.FIELDS})


def test_default_params_and_their_validation(built_lib):
    from mrca import _lib
    from mrca.nhorca import NhOrcaParams
    assert built_lib.mrca_nhorca_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.NhOrcaParamsStruct()
    assert built_lib.mrca_nhorca_default_params(C.byref(st)) == 0
    got = {k: getattr(st, k) for k in NR.FIELDS}
    assert got == {k: (v if k == "max_neighbors" else float(f32(v))) for k, v in NR.DEFAULTS.items()}
    assert [n for n, _t in _lib.NhOrcaParamsStruct._fields_] == NR.FIELDS and C.sizeof(st) == 52
    assert [n for n, _t in _lib.NhOrcaParamsStruct._fields_][:11] == [n for n, _t in _lib.OrcaParamsStruct._fields_]
    orca = _lib.OrcaParamsStruct()
    built_lib.mrca_orca_default_params(C.byref(orca))
    assert all(getattr(orca, k) == getattr(st, k) for k in R.FIELDS if k != "jitter")     # ORCA's fields at ORCA's defaults
    p = NhOrcaParams(track_error=0.1)
    assert abs(p.track_error - 0.1) < 1e-7 and p.max_neighbors == 10 and p.struct().track_time == st.track_time
    assert NhOrcaParams.from_assignments(["track_time=0.5", "max_neighbors=12"]).max_neighbors == 12
    with pytest.raises(ValueError):
        NhOrcaParams.from_assignments(["nonsense=1"])
    # what can be judged without an env is judged before the env is looked at
    call = built_lib.mrca_nhorca_actions
    assert call(None, None, None, C.c_void_p(0x1000), None, None, None) == -1 and b"env is NULL" in built_lib.mrca_last_error()
    assert call(None, None, None, None, None, None, None) == -1 and b"actions_dev" in built_lib.mrca_last_error()
    assert call(None, None, None, C.c_void_p(0x1000), None, C.c_void_p(0x1002), None) == -1 and b"mode_dev" in built_lib.mrca_last_error()
    bad = [("radius", float("nan"), "radius is not finite"), ("track_error", float("nan"), "track_error is not finite"),
           ("track_time", float("inf"), "track_time is not finite"), ("radius", 0.0, "radius must be > 0"),
           ("obst_dist", 6.5, "obst_dist outside [0, 6]"), ("track_error", 0.0, "track_error outside (0, 0.5]"),
           ("track_error", 0.51, "track_error outside (0, 0.5]"), ("track_time", 0.05, "track_time outside [0.1, 1.5]"),
           ("track_time", 1.6, "track_time outside [0.1, 1.5]"), ("max_neighbors", 0, "max_neighbors 0 outside 1..46"),
           ("max_neighbors", 47, "max_neighbors 47 outside 1..46")]
    for k, v, msg in bad:
        st = _lib.NhOrcaParamsStruct()
        built_lib.mrca_nhorca_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(None, C.byref(st), None, C.c_void_p(0x1000), None, None, None) == -1
        assert built_lib.mrca_last_error().decode() == "mrca_nhorca_actions: " + msg, (k, v, built_lib.mrca_last_error())
    for k, v in (("track_error", 0.5), ("track_time", 0.1), ("track_time", 1.5), ("max_neighbors", 46), ("max_neighbors", 1)):
        st = _lib.NhOrcaParamsStruct()
        built_lib.mrca_nhorca_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(None, C.byref(st), None, C.c_void_p(0x1000), None, None, None) == -1
        assert b"env is NULL" in built_lib.mrca_last_error(), (k, v)      # the params passed


# ------------------------------------------------------------------------------------------------ closed loop on the C oracle
def closed_loop(nhshim, sc, p, ticks, poses=None, goals=None, check=None):
    env = U.COracleEnv(sc)
    env.reset(None, poses, goals)
    for k in range(ticks):
        act, vel, mode, _s1, lines, counts = host_env_actions(nhshim, p, sc.robots_per_world, sc.seed, env.pose, env.speed_gt, env.goal,
                                                              env.scan, env.hit_robot, want_lines=check is not None)
        if check is not None:
            check(k, env, vel, lines, counts)
        env.step(act)
        if (env.first_result != 0).all():
            break
    env.ticks_run = k + 1
    return env


def test_gate_two_robots_pass_each_other(nhshim, defaults):
    sc = S.circle_n(2, 4.0, grid=S.empty_grid())
    poses = np.asarray(sc.init_table, f32).copy()
    poses[1, 1] += f32(0.2)                              # 0.2 m off the axis
    env = closed_loop(nhshim, sc, defaults, 400, poses, np.asarray(sc.goal_table, f32))
    assert (env.first_result == 1).all() and not env.crashed.any(), (env.first_result, env.pose)


def test_gate_one_robot_never_hits_the_block(nhshim, defaults):
    # test_orca_host's scene: a 1 m wide block across the way, the robot drives along y = 0.4, its goal 3 m behind the block
    grid = U.small_grid(blocks=[(0.0, -0.5, 0.5, 0.5)])
    sc = S.circle_n(1, 4.0, grid=grid)
    active = []

    def check(k, env, vel, lines, counts):
        ns = counts[0, 1]
        if ns:
            L, r = lines[0, 2:2 + ns].astype(np.float64), vel[0].astype(np.float64)
            viol = L[:, 2] * (L[:, 1] - r[1]) - L[:, 3] * (L[:, 0] - r[0])
            assert viol.max() <= 1e-5, (k, viol.max())
            active.append(k)
    env = closed_loop(nhshim, sc, defaults, 400, np.array([[-3.0, 0.4, 0.0]], f32), np.array([[3.5, 0.4]], f32), check)
    assert not env.crashed.any() and env.first_result[0] != 2
    assert len(active) > 10                              # the block was seen


def test_gate_four_robots_cross(nhshim, defaults):
    sc = S.circle_n(4, 3.0, grid=S.empty_grid())
    env = closed_loop(nhshim, sc, defaults, 500)
    assert (env.first_result == 1).all() and not env.crashed.any(), (env.first_result, env.pose)


def test_gate_ten_robots_cross(nhshim, defaults):
    sc = S.circle_n(10, 8.0, grid=S.empty_grid())
    env = closed_loop(nhshim, sc, defaults, 800)
    assert (env.first_result == 1).all() and not env.crashed.any(), (env.first_result, env.pose)
