"""The scenario sampler's rule (csrc/mrca_scatter_device.h) compiled for the host with g++ -ffp-contract=off: the very functions
the gfx950 kernel calls, held EQUAL -- poses and goals bit for bit, tries equal -- to the NumPy float32 restatement of
tests/scatter_ref.py on the cases of tests/scatter_cases.py; the rule's properties in float64; the stream words; the library's
defaults and validation table; the producer's checks (check_boxes) and the scenario constructors' coverage rule.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scatter_cases as SC
import scatter_ref as R
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32, u32 = np.float32, np.uint32

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "mrca_host.h"
#include "mrca_scatter_device.h"
#include "mrca_noise_device.h"
using namespace mrca;
extern "C" void shim_cellfield(const uint32_t* bits, const GridGeom* g, uint8_t* out) {
    std::vector<uint8_t> cf;
    build_cell_field(bits, g->width, g->height, g->wpr, &cf);
    memcpy(out, cf.data(), cf.size());
}
extern "C" void shim_scatter(const ScatterParams* p, const GridGeom* g, const uint8_t* cf, uint32_t k0, uint32_t k1, int W, int R,
                             const float* boxes, float* poses, float* goals, int32_t* tries) {
    std::vector<ScatterXY> placed(R);
    for (int w = 0; w < W; ++w)
        scatter_world(*p, *g, cf, k0, k1, R, w, boxes, poses + (size_t)w * R * 3, goals + (size_t)w * R * 2,
                      tries ? tries + (size_t)w * R * 2 : nullptr, placed.data());
}
extern "C" int shim_clearance(const GridGeom* g, const uint8_t* cf, float x, float y) { return scatter_clearance(cf, *g, x, y); }
extern "C" uint32_t shim_streams(void) { return kStreamScatterStart | (kStreamScatterGoal << 8); }
extern "C" uint32_t shim_reset_streams(void) { return kStreamPose | (kStreamGoal << 8); }
extern "C" uint32_t shim_noise_word(int32_t t) { return noise_counter_word(t); }
extern "C" int shim_max_robots(void) { return kScatterMaxRobots; }
"""


class Geom(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("x0", "y0", "cell", "inv_cell")] + [(k, C.c_int32) for k in ("width", "height", "wpr")]


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in R.FIELDS[:4]] + [("clear_cells", C.c_int32), ("max_tries", C.c_int32), ("draw", C.c_uint32)]


def geom(grid):
    return Geom(f32(grid.x0), f32(grid.y0), f32(grid.cell), f32(1.0) / f32(grid.cell), grid.width, grid.height, grid.words_per_row)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("scatter_host")
    src, so = d / "shim.cpp", d / "libscatter_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    lib.shim_scatter.argtypes = [C.POINTER(Params), C.POINTER(Geom), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.shim_clearance.argtypes = [C.POINTER(Geom), C.c_void_p, C.c_float, C.c_float]
    lib.shim_streams.restype = lib.shim_reset_streams.restype = lib.shim_noise_word.restype = C.c_uint32
    return lib


def host_cellfield(shim, grid):
    cf = np.zeros((grid.height, grid.width), np.uint8)
    bits, g = np.ascontiguousarray(grid.bits, np.uint32), geom(grid)
    shim.shim_cellfield(ptr(bits), C.byref(g), ptr(cf))
    return cf


def host_scatter(shim, p, grid, seed, W, Rn, boxes, with_tries=True):
    """the host build of the rule, on the cell field the LIBRARY builds -> (poses, goals, tries)"""
    cf, g, q = host_cellfield(shim, grid), geom(grid), Params(**p)
    boxes = np.ascontiguousarray(boxes, f32)
    poses, goals, tries = np.zeros((W * Rn, 3), f32), np.zeros((W * Rn, 2), f32), np.full((W * Rn, 2), -7, np.int32)
    k0, k1 = R.key_of(seed)
    shim.shim_scatter(C.byref(q), C.byref(g), ptr(cf), int(k0), int(k1), W, Rn, ptr(boxes), ptr(poses), ptr(goals),
                      ptr(tries) if with_tries else None)
    return poses, goals, tries


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def assert_same(got, want, what):
    for g, w, name in zip(got[:2], want[:2], ("poses", "goals")):
        assert np.array_equal(bits(g), bits(w)), (what, name, np.argwhere(bits(g) != bits(w))[:5])
    assert np.array_equal(got[2], want[2]), (what, "tries", np.argwhere(got[2] != want[2])[:5])


def check_properties(grid, W, Rn, boxes, p, out, cf):
    """what the rule promises, computed in float64 from the outputs: for every robot that reports tries > 0"""
    poses, goals, tries = (np.asarray(a) for a in out)
    P, G = poses.astype(np.float64).reshape(W, Rn, 3), goals.astype(np.float64).reshape(W, Rn, 2)
    T = tries.reshape(W, Rn, 2)
    assert ((T >= 1) & (T <= p["max_tries"]) | (T == -1)).all()
    assert (np.abs(P[..., 2]) <= np.pi + 1e-6).all()
    b = np.asarray(boxes, np.float64)
    for pts, lo, phase, sep in ((P[..., :2], 0, 0, p["min_sep"]), (G, 4, 1, p["goal_sep"])):
        # inside the robot's box (up to a rounding of x0 + (x1 - x0) * u)
        assert (pts[..., 0] >= b[None, :, lo] - 1e-5).all() and (pts[..., 0] <= b[None, :, lo + 2] + 1e-5).all()
        assert (pts[..., 1] >= b[None, :, lo + 1] - 1e-5).all() and (pts[..., 1] <= b[None, :, lo + 3] + 1e-5).all()
        ok = T[..., phase] > 0
        # a robot that was placed keeps its distance from every robot BEFORE it, placed or not; one float32 rounding of each of
        # the three squares and of the sum: relative 4 * 2^-24 of the squared distance
        d2 = ((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(-1)
        earlier = np.tril(np.ones((Rn, Rn), bool), -1)[None] & ok[:, :, None]
        assert (d2[earlier] >= float(f32(sep)) ** 2 * (1 - 2.0 ** -21)).all(), (phase, np.sqrt(d2[earlier].min()), sep)
        # clear of the map, by the restatement's own cell field
        v = R.clearance(cf, grid, pts[..., 0].astype(f32).ravel(), pts[..., 1].astype(f32).ravel()).reshape(W, Rn)
        assert (v[ok] > p["clear_cells"]).all()
    ok = T[..., 1] > 0
    d = np.sqrt(((G - P[..., :2]) ** 2).sum(-1))[ok]
    assert (d >= p["goal_min"] * (1 - 1e-6)).all() and (d <= p["goal_max"] * (1 + 1e-6)).all()


# ------------------------------------------------------------------------------------------------ equality with scatter_ref
@pytest.mark.parametrize("name", SC.HOST_CASES)
def test_host_build_equals_the_restatement(shim, name):
    grid, W, Rn, boxes, p, want = SC.case(name)
    assert np.array_equal(host_cellfield(shim, grid), R.cellfield(grid.dense()))
    got = host_scatter(shim, p, grid, SC.SEED, W, Rn, boxes)
    assert_same(got, want, name)
    check_properties(grid, W, Rn, boxes, p, got, R.cellfield(grid.dense()))
    # tries not wanted: the same poses and goals
    again = host_scatter(shim, p, grid, SC.SEED, W, Rn, boxes, with_tries=False)
    assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(bits(again[1]), bits(got[1])) and (again[2] == -7).all()


def test_the_cases_exercise_what_they_are_for():
    """asserted on the RESTATEMENT's answers, so that the paths are taken whatever the code under test does"""
    for name in ("narrow_R4", "narrow_R65"):            # more candidates than a 256-lane round holds, and every robot placed
        tries = SC.case(name)[5][2]
        assert (tries[:, 1] > 256).any() and (tries > 0).all(), (name, tries[:, 1].max())
    assert (SC.case("narrow_R65")[5][2][:, 1] > 1024).any()         # ... more than four rounds of them
    tries = SC.case("infeasible")[5][2]                              # a 2 m x 2 m box holds 9 points 1 m apart at most
    assert (tries[:, 0] == -1).sum() >= 7 and (tries[:, 1] == -1).sum() >= 7 and tries[0, 0] == 1
    assert (SC.case("tries1")[5][2] == -1).any() and set(np.unique(SC.case("tries1")[5][2])) <= {-1, 1}
    assert SC.case("tries100")[5][2].max() <= 100 and SC.case("tries300")[5][2].max() <= 300
    # 12 robots in 4 m x 4 m: one of them gives up at 100 candidates and is placed within 300 -- more than one round of 64 lanes
    assert (SC.case("tries100")[5][2] == -1).any() and SC.case("tries100")[5][2].max() > 64
    assert 100 < SC.case("tries300")[5][2].max() and (SC.case("tries300")[5][2] > 0).all()
    # the off-map case: accepted points inside AND outside the map, and every robot placed
    grid, W, Rn, boxes, p, (poses, goals, tries) = SC.case("off_map")
    assert (tries > 0).all()
    x, y = poses[:, 0].astype(np.float64), poses[:, 1].astype(np.float64)
    outside = (x < grid.x0) | (x >= grid.x0 + grid.width * 0.1) | (y < grid.y0) | (y >= grid.y0 + grid.height * 0.1)
    assert outside.any() and (~outside).any()
    assert (tries[:, 0] > 1).any()                                   # some first candidate was refused
    # pinned coordinates come out to the bit
    grid, W, Rn, boxes, p, (poses, goals, tries) = SC.case("pinned")
    for w in range(W):
        assert np.array_equal(poses[w * Rn + 0, :2], boxes[0, :2]) and np.array_equal(goals[w * Rn + 1], boxes[1, 4:6])
        assert poses[w * Rn + 2, 0] == f32(-0.5) and goals[w * Rn + 3, 1] == f32(0.75)
        assert tries[w * Rn, 0] == 1 and tries[w * Rn, 1] == 1


def test_the_clamped_clearance(shim):
    """on, beside and beyond every edge of a map whose edge cells have bytes of their own: the host build equals the
    restatement, the value off the map is the clamped cell's byte or the distance to it, and never more than the TRUE
    Chebyshev distance to an occupied cell"""
    grid = SC.holes_grid()
    cf, g = R.cellfield(grid.dense()), geom(grid)
    assert np.array_equal(host_cellfield(shim, grid), cf)
    occ = np.argwhere(grid.dense())                                  # (row, column)
    xs = [grid.x0 + 0.1 * c for c in (-7.5, -2.5, -1.5, -1.0, -0.5, 0.0, 0.5, 1.5, 20.5, 38.5, 39.5, 40.0, 40.5, 41.5, 46.5)]
    ys = [grid.y0 + 0.1 * c for c in (-6.5, -1.5, -1.0, -0.5, 0.0, 0.5, 14.5, 28.5, 29.5, 30.0, 30.5, 31.5, 35.5)]
    seen_off = 0
    for x in xs:
        for y in ys:
            got = shim.shim_clearance(C.byref(g), ptr(cf), x, y)
            want = int(R.clearance(cf, grid, np.array([x], f32), np.array([y], f32))[0])
            assert got == want, (x, y, got, want)
            cx = int(np.floor((f32(x) - f32(grid.x0)) * (f32(1.0) / f32(grid.cell))))
            cy = int(np.floor((f32(y) - f32(grid.y0)) * (f32(1.0) / f32(grid.cell))))
            true = np.maximum(np.abs(occ[:, 1] - cx), np.abs(occ[:, 0] - cy)).min()
            assert got <= true, (x, y, got, true)
            if 0 <= cx < grid.width and 0 <= cy < grid.height:
                assert got == cf[cy, cx] == true
            else:
                seen_off += 1
                qx, qy = min(max(cx, 0), grid.width - 1), min(max(cy, 0), grid.height - 1)
                assert got == max(int(cf[qy, qx]), abs(cx - qx), abs(cy - qy))
    assert seen_off > 50
    # a point that is no number, or beyond any cell index, is never clear
    for x, y in ((float("nan"), 0.0), (0.0, float("inf")), (3.0e9, 0.0), (0.0, -3.0e9)):
        assert shim.shim_clearance(C.byref(g), ptr(cf), x, y) == 0
        with np.errstate(all="ignore"):
            assert R.clearance(cf, grid, np.array([x], f32), np.array([y], f32))[0] == 0
    # the open world: everything is clear for every clear_cells the library takes
    og = S.empty_grid()
    ocf, ogg = R.cellfield(og.dense()), geom(og)
    assert (ocf == 255).all()
    for x, y in ((0.0, 0.0), (-3.99, 3.99), (-4.0, 4.0), (1.0e4, -1.0e4), (12.0, 0.5)):
        assert shim.shim_clearance(C.byref(ogg), ptr(ocf), x, y) >= 255


# ------------------------------------------------------------------------------------------------ properties
def test_a_world_does_not_depend_on_the_other_worlds(shim):
    grid, W, Rn, boxes, p, want = SC.case("open_R65_W3")
    for fewer in (1, 2):
        got = host_scatter(shim, p, grid, SC.SEED, fewer, Rn, boxes)
        assert_same(got, tuple(a[:fewer * Rn] for a in want), fewer)
        ref = R.scatter(p, grid, SC.SEED, fewer, Rn, boxes)
        assert_same(ref, tuple(a[:fewer * Rn] for a in want), fewer)
    # ... and the worlds of one call differ from each other
    assert not np.array_equal(want[0][:Rn], want[0][Rn:2 * Rn])


def test_another_draw_or_seed_is_another_set_of_scenarios(shim):
    grid, W, Rn, boxes, p, want = SC.case("open_R3_W3")
    for change in (dict(draw=1), dict(draw=0xFFFFFFFF)):
        q = dict(p, **change)
        got = host_scatter(shim, q, grid, SC.SEED, W, Rn, boxes)
        assert_same(got, R.scatter(q, grid, SC.SEED, W, Rn, boxes), change)
        assert (bits(got[0][:, :2]) != bits(want[0][:, :2])).all() and (bits(got[1]) != bits(want[1])).all()
    got = host_scatter(shim, p, grid, SC.SEED + 1, W, Rn, boxes)
    assert_same(got, R.scatter(p, grid, SC.SEED + 1, W, Rn, boxes), "seed")
    assert (bits(got[0][:, :2]) != bits(want[0][:, :2])).all()
    # the same call twice: the same bits
    assert_same(host_scatter(shim, p, grid, SC.SEED, W, Rn, boxes), want, "again")


def test_the_words_meet_neither_the_reset_sampler_nor_the_noise_model(shim):
    streams = shim.shim_streams()
    start, goal = streams & 0xFF, streams >> 8
    assert (start, goal) == (R.STREAM_START, R.STREAM_GOAL) == (3, 7) and start & 3 == 3 and goal & 3 == 3
    reset = shim.shim_reset_streams()
    pose, rgoal = reset & 0xFF, reset >> 8
    assert (pose, rgoal) == (R.O.STREAM_POSE, R.O.STREAM_GOAL) == (0, 1)
    assert len({start, goal, pose, rgoal}) == 4
    ts = np.concatenate([np.arange(0, 4096), [2 ** 29, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, -1]]).astype(np.int64)
    words = np.array([shim.shim_noise_word(int(np.int32(t))) for t in ts.astype(np.int32)], np.int64)
    assert ((words & 3) == 2).all() and not np.isin(words, [start, goal]).any()
    # the same robot, second word and candidate on the four whole-word streams: four different draws
    key = R.key_of(SC.SEED)
    seen = {tuple(int(w) for w in R.O.philox4x32(u32(5), u32(0), u32(9), u32(word), *key)) for word in (pose, rgoal, start, goal)}
    assert len(seen) == 4


# ------------------------------------------------------------------------------------------------ the library's own table
def test_default_params_and_the_validation_table(built_lib, shim):
    from mrca import _lib
    from mrca.scatter import ScatterParams
    lib = built_lib
    assert "mrca_scatter" in _lib.EXPORTS and "mrca_scatter_default_params" in _lib.EXPORTS
    assert lib.mrca_scatter_default_params(None) == -1 and lib.mrca_last_error() == b"mrca_scatter_default_params: out is NULL"
    st = _lib.ScatterParamsStruct()
    assert lib.mrca_scatter_default_params(C.byref(st)) == 0
    assert {k: getattr(st, k) for k in R.FIELDS} == {k: (float(f32(v)) if isinstance(v, float) else v) for k, v in R.DEFAULTS.items()}
    assert [n for n, _t in _lib.ScatterParamsStruct._fields_] == list(R.FIELDS) and C.sizeof(st) == C.sizeof(Params) == 28
    assert shim.shim_max_robots() == R.MAX_ROBOTS == 4096
    p = ScatterParams(min_sep=0.8, draw=3)
    assert p.min_sep == 0.8 and p.draw == 3 and p.max_tries == 1024 and isinstance(p.max_tries, int) and p.struct().goal_min == 5.0
    q = ScatterParams.from_assignments("min_sep=0.7,max_tries=4096,draw=9")
    assert (q.min_sep, q.max_tries, q.draw, q.goal_sep) == (0.7, 4096, 9, 1.0)
    assert ScatterParams.from_assignments(["clear_cells=0"], start=dict(goal_min=6.0)).as_dict() == dict(R.DEFAULTS, clear_cells=0, goal_min=6.0)
    for bad in ("nonsense=1", "min_sep"):
        with pytest.raises(ValueError):
            ScatterParams.from_assignments(bad)

    buf = np.zeros(64, f32)
    good = buf.ctypes.data + (-buf.ctypes.data) % 16

    def call(over=None, boxes=good, poses=good, goals=good, tries=good):
        st = _lib.ScatterParamsStruct()
        lib.mrca_scatter_default_params(C.byref(st))
        for k, v in (over or {}).items():
            setattr(st, k, v)
        rc = lib.mrca_scatter(None, C.byref(st), *[None if a is None else C.c_void_p(a) for a in (boxes, poses, goals, tries)], None)
        return rc, lib.mrca_last_error().decode()

    # what can be judged without an env is judged before the env is looked at -- each message in full
    assert call() == (-1, "env is NULL")
    assert lib.mrca_scatter(None, None, C.c_void_p(good), C.c_void_p(good), C.c_void_p(good), None, None) == -1 and \
        lib.mrca_last_error() == b"env is NULL"
    for k in R.FIELDS[:4]:
        for v in (float("nan"), float("inf"), float("-inf")):
            assert call({k: v}) == (-1, f"mrca_scatter: {k} is not finite")
    below = float(np.nextafter(f32(0.6), f32(0)))
    assert call({"min_sep": below}) == (-1, "mrca_scatter: min_sep must be >= 0.6")
    assert call({"min_sep": 0.1}) == (-1, "mrca_scatter: min_sep must be >= 0.6")
    assert call({"min_sep": float(f32(0.6))}) == (-1, "env is NULL")
    assert call({"goal_sep": -0.01}) == (-1, "mrca_scatter: goal_sep must be >= 0")
    assert call({"goal_sep": 0.0}) == (-1, "env is NULL")
    assert call({"goal_min": -1.0}) == (-1, "mrca_scatter: goal_min must be >= 0")
    assert call({"goal_min": 7.0, "goal_max": 6.0}) == (-1, "mrca_scatter: goal_max must be >= goal_min")
    assert call({"goal_min": 6.0, "goal_max": 6.0}) == (-1, "env is NULL")
    assert call({"clear_cells": -1}) == (-1, "mrca_scatter: clear_cells -1 outside 0..254")
    assert call({"clear_cells": 255}) == (-1, "mrca_scatter: clear_cells 255 outside 0..254")
    assert call({"clear_cells": 254}) == (-1, "env is NULL")
    assert call({"max_tries": 0}) == (-1, "mrca_scatter: max_tries 0 outside 1..65536")
    assert call({"max_tries": 65537}) == (-1, "mrca_scatter: max_tries 65537 outside 1..65536")
    assert call({"max_tries": 65536, "draw": 0xFFFFFFFF}) == (-1, "env is NULL")
    assert call(boxes=None) == (-1, "mrca_scatter: boxes_dev is NULL")
    assert call(poses=None) == (-1, "mrca_scatter: poses_dev is NULL")
    assert call(goals=None) == (-1, "mrca_scatter: goals_dev is NULL")
    assert call(tries=None) == (-1, "env is NULL")
    assert call(boxes=good + 2) == (-1, "mrca_scatter: boxes_dev must be 4-byte aligned")
    assert call(poses=good + 1) == (-1, "mrca_scatter: poses_dev must be 4-byte aligned")
    assert call(poses=good + 4) == (-1, "env is NULL")
    assert call(goals=good + 4) == (-1, "mrca_scatter: goals_dev must be 8-byte aligned")
    assert call(tries=good + 2) == (-1, "mrca_scatter: tries_dev must be 4-byte aligned")
    # the params are judged before the pointers
    assert call({"min_sep": 0.1}, poses=None) == (-1, "mrca_scatter: min_sep must be >= 0.6")
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the producer and the constructors
def test_check_boxes():
    from mrca.scatter import check_boxes
    good = SC.pinned_boxes()
    out = check_boxes(good.astype(np.float64).tolist(), 6)
    assert out.dtype == f32 and out.flags.c_contiguous and np.array_equal(out, good)
    bad = {
        "shape": (good[:5], "expected shape (6, 8)"),
        "nan": (np.where(np.arange(48).reshape(6, 8) == 13, np.nan, good), "row 1 holds a value that is not finite"),
        "inf": (np.where(np.arange(48).reshape(6, 8) == 47, np.inf, good), "row 5 holds a value that is not finite"),
        "far": (np.where(np.arange(48).reshape(6, 8) == 16, -10000.5, good), "row 2 holds a coordinate beyond +-10000"),
    }
    for lo, hi, what in ((0, 2, "sx0 > sx1"), (1, 3, "sy0 > sy1"), (4, 6, "gx0 > gx1"), (5, 7, "gy0 > gy1")):
        b = good.copy()
        b[3, [lo, hi]] = b[3, [hi, lo]] + np.array([1.0, 0.0], f32)
        bad[what] = (b, f"row 3 has {what}")
    for key, (b, text) in bad.items():
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")):
            check_boxes(b, 6)
    assert check_boxes(np.full((2, 8), 1.0e4), 2).shape == (2, 8)      # the bound itself, and a box that is a point


CONSTRUCTORS = [("random_box", 74, {}), ("group_swap", 30, {}), ("group_crossing", 12, {}), ("corridor", 30, {})]


@pytest.mark.parametrize("name,most,kw", CONSTRUCTORS)
def test_a_constructor_refuses_more_than_its_boxes_take(name, most, kw):
    """discs of diameter min_sep may cover 30 % of the smallest box they are dealt into: the count at the bound is taken, one
    more robot in a box is refused"""
    make = getattr(S, name)
    sc = make(robots=most, num_worlds=3, seed=5, **kw)
    assert (sc.robots_per_world, sc.num_worlds, sc.seed, sc.auto_reset, sc.w_thresh, sc.pre_dist_zero) == (most, 3, 5, S.AUTO_NONE, 0.7, True)
    assert sc.boxes.shape == (most, 8) and sc.scatter["min_sep"] == 1.0 and (sc.reset_mode == S.RESET_TABLE).all()
    assert sc.grid.cell == 0.1 and sc.timeout == 900 and make(robots=2, timeout=300).timeout == 300
    # the count per box, from the boxes themselves
    disc = np.pi * 0.25
    for half in (sc.boxes[:, :4], sc.boxes[:, 4:]):
        for box in np.unique(half, axis=0):
            n = (half == box).all(1).sum()
            area = (box[2] - box[0]) * (box[3] - box[1])
            assert n * disc <= 0.3 * area < (n + 1) * disc
    with pytest.raises(ValueError, match="more than 30 %"):
        make(robots=most + (1 if name == "random_box" else 2), **kw)
    with pytest.raises(ValueError, match="more than 30 %"):
        make(robots=most + 1, **kw)                      # (the even indices' box takes the one more)
    # a smaller min_sep makes room
    assert make(robots=most + 2, min_sep=0.8, **kw).scatter["min_sep"] == 0.8
    # a walled room with a 2-cell border, and every box at least a metre inside the wall
    occ = sc.grid.dense()
    assert occ[:2].all() and occ[-2:].all() and occ[:, :2].all() and occ[:, -2:].all() and not occ[2, 2]
    assert (sc.boxes[:, [0, 4]] >= sc.grid.x0 + 1.0 - 1e-9).all() and (sc.boxes[:, [2, 6]] <= -sc.grid.x0 - 1.0 + 1e-9).all()
    assert (sc.boxes[:, [1, 5]] >= sc.grid.y0 + 1.0 - 1e-9).all() and (sc.boxes[:, [3, 7]] <= -sc.grid.y0 - 1.0 + 1e-9).all()


def test_the_constructors_rooms_and_boxes():
    sc = S.random_box(robots=4, side=12.0)
    assert (sc.grid.width, sc.grid.height) == (120, 120) and (sc.boxes == [-5, -5, 5, 5, -5, -5, 5, 5]).all()
    assert sc.scatter == dict(min_sep=1.0, goal_min=6.0, goal_max=1.0e4)
    sc = S.group_swap(robots=5)
    assert (sc.grid.width, sc.grid.height, sc.grid.x0, sc.grid.y0) == (200, 120, -10.0, -6.0)
    assert (sc.boxes[0] == [-9, -5, -5, 5, 5, -5, 9, 5]).all() and (sc.boxes[1] == [5, -5, 9, 5, -9, -5, -5, 5]).all()
    assert (sc.boxes[::2] == sc.boxes[0]).all() and (sc.boxes[1::2] == sc.boxes[1]).all()
    sc = S.group_crossing(robots=4)
    assert (sc.grid.width, sc.grid.height) == (200, 200)
    assert (sc.boxes[0] == [-9, -3, -6, 3, 6, -3, 9, 3]).all() and (sc.boxes[1] == [-3, -9, 3, -6, -3, 6, 3, 9]).all()
    sc = S.corridor(robots=4, width=3.0)
    assert (sc.grid.width, sc.grid.height) == (240, 100)
    assert (sc.boxes[0] == [-11, -4, -6, 4, 6, -4, 11, 4]).all() and (sc.boxes[1] == [6, -4, 11, 4, -11, -4, -6, 4]).all()
    occ = sc.grid.dense()
    xc, yc = -12.0 + (np.arange(240) + 0.5) * 0.1, -5.0 + (np.arange(100) + 0.5) * 0.1
    inner = occ[2:-2, 2:-2]
    want = (np.abs(yc[2:-2, None]) > 1.5) & (np.abs(xc[None, 2:-2]) < 4.0)
    assert np.array_equal(inner, want) and want.any()
    free_rows = np.flatnonzero(~occ[:, 120])
    assert len(free_rows) == 30 and abs(yc[free_rows].mean()) < 1e-9       # a corridor of 3 m around y = 0
    with pytest.raises(ValueError):
        S.corridor(width=0.5)
    # a Scenario without boxes is what it was
    assert S.circle().boxes is None and S.circle().scatter is None and S.doorway().boxes is None
