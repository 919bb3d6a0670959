"""The renderer's rules (csrc/mrca_render_device.h) compiled for the host with g++ -ffp-contract=off and driven in their
SCATTER form -- per robot: pixel box, inside tests, maximum into the ID image; the very functions the gfx950 kernel calls --
held EQUAL, pixel for pixel, to the NumPy float32 GATHER restatement of tests/render_ref.py (per pixel: the maximum over the
map, all goals, all robots).  What can go wrong in between is the conservative pixel box (a robot clipped by its own box),
the clipping at the image's edges, and the priority rule; the cases are chosen for those.  Also the palette against the
documented table and mrca_render's argument checks, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_ref as RR
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")

SHIM = r"""
#include <stdint.h>
#include "mrca_render_device.h"
using namespace mrca;
struct MaxPut {
    uint32_t* img;
    void operator()(int pixel, uint32_t id) { if (id > img[pixel]) img[pixel] = id; }
};
extern "C" void shim_map(int W, int H, float cx, float cy, float m, float gx0, float gy0, float cell, int gw, int gh, int wpr,
                         const uint32_t* bits, uint32_t* ids) {
    const RenderFrame f = render_frame(RenderView{0, cx, cy, m}, W, H);
    const GridGeom g{gx0, gy0, cell, 1.0f / cell, gw, gh, wpr};
    for (int row = 0; row < H; ++row)
        for (int col = 0; col < W; ++col)
            ids[row * W + col] = render_map_at(g, bits, pixel_x(f, col), pixel_y(f, row)) ? render_id(kLayerMap, 0u) : 0u;
}
// the scatter: robot after robot (in the order given), `lanes` lanes sharing each one as a wavefront's do
extern "C" void shim_splat(int W, int H, float cx, float cy, float m, uint32_t layers, int n, const int32_t* order, const float* pose_xy,
                           const float* sincos, const float* goal, int lanes, uint32_t* ids) {
    const RenderFrame f = render_frame(RenderView{0, cx, cy, m}, W, H);
    MaxPut put{ids};
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        for (int lane = 0; lane < lanes; ++lane)
            render_splat_robot(f, layers, pose_xy[2 * i], pose_xy[2 * i + 1], sincos[2 * i], sincos[2 * i + 1], goal[2 * i],
                               goal[2 * i + 1], (uint32_t)i, lane, lanes, put);
    }
}
extern "C" uint32_t shim_rgb(uint32_t id, uint32_t trail, uint32_t crashed, uint32_t first, uint32_t live) {
    return render_rgb(id, trail, crashed, first, live);
}
extern "C" int shim_pixel_of(int W, int H, float cx, float cy, float m, float x, float y, int* col, int* row) {
    return pixel_of(render_frame(RenderView{0, cx, cy, m}, W, H), x, y, col, row);
}
"""

SIZES = [(70, 45), (64, 64)]
SCALES = [1.0 / 16.0, 0.05, 0.3, 2.0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_host")
    src, so = d / "shim.cpp", d / "librender_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    lib.shim_map.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                             C.c_int, up, up]
    lib.shim_splat.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, ip, fp, fp, fp, C.c_int, up]
    lib.shim_rgb.argtypes = [C.c_uint32] * 5
    lib.shim_rgb.restype = C.c_uint32
    lib.shim_pixel_of.argtypes = [C.c_int, C.c_int] + [C.c_float] * 5 + [ip, ip]
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def scatter(lib, view, W, H, layers, pose_xy, sincos, goals, lanes=1, order=None):
    n = len(pose_xy)
    order = np.arange(n, dtype=np.int32) if order is None else np.ascontiguousarray(order, np.int32)
    pose_xy, sincos, goals = (np.ascontiguousarray(a, np.float32) for a in (pose_xy, sincos, goals))
    ids = np.zeros((H, W), np.uint32)
    lib.shim_splat(W, H, view[0], view[1], view[2], layers, n, _ptr(order, C.c_int32), _ptr(pose_xy, C.c_float),
                   _ptr(sincos, C.c_float), _ptr(goals, C.c_float), lanes, _ptr(ids, C.c_uint32))
    return ids


def edge_cases(view, W, H, rng):
    """Robots straddling each image edge and corner, wholly outside, at negative coordinates, on top of each other and of each
    other's goals, with pixel centres exactly on footprint edges; headings at multiples of pi/2 and random."""
    x0, y1, m, wx, wy = RR.frame(view, W, H)
    xl, xr, yt, yb = float(x0), float(x0 + np.float32(W) * m), float(y1), float(y1 - np.float32(H) * m)
    xm, ym = 0.5 * (xl + xr), 0.5 * (yt + yb)
    pts = [(xl, ym), (xr, ym), (xm, yt), (xm, yb),                       # the four edges
           (xl, yt), (xr, yt), (xl, yb), (xr, yb),                       # the four corners
           (xl - 0.5, ym), (xr + 7.0, yb - 7.0), (xm, yt + 0.31),        # outside: near, far, just beyond the body's reach
           (xm, ym), (xm + 0.1, ym + 0.05), (xm + 0.1, ym + 0.05),       # overlapping, two of them identical
           (float(wx[W // 3]) - 0.22, float(wy[H // 3])),                # a pixel centre exactly on the front edge ...
           (float(wx[W // 4]), float(wy[H // 4]) + 0.19),                # ... and on a side edge
           (float(wx[W // 5]) - 0.11, float(wy[H // 5]))]                # ... and on the nose line
    # a footprint corner reaching 0.2905 of its 0.2907 m along +x, +y, -x, -y, onto a pixel centre: the box's reach is needed
    diag = float(np.arctan2(0.19, 0.22))
    pts += [(float(wx[W // 2]) - 0.2905, float(wy[H // 2])), (float(wx[W // 2 + 9]), float(wy[H // 2]) - 0.2905),
            (float(wx[W // 2]) + 0.2905, float(wy[H // 2 + 9])), (float(wx[W // 2 - 9]), float(wy[H // 2]) + 0.2905)]
    pts += [(rng.uniform(xl - 1, xr + 1), rng.uniform(yb - 1, yt + 1)) for _ in range(8)]
    pose = np.array(pts, np.float32)
    n = len(pose)
    th = np.concatenate([np.arange(n - 12) * (np.pi / 2), np.arange(4) * (np.pi / 2) - diag, rng.uniform(-np.pi, np.pi, 8)])
    sincos = np.stack([np.sin(th), np.cos(th)], 1).astype(np.float32)
    quarter = np.arange(n - 12) % 4                                       # exact sines and cosines at multiples of pi / 2
    sincos[:n - 12] = np.array([(0, 1), (1, 0), (0, -1), (-1, 0)], np.float32)[quarter]
    goals = np.roll(pose, 5, axis=0).copy()                               # every goal under another robot
    goals[::3] += rng.uniform(-0.4, 0.4, goals[::3].shape).astype(np.float32)
    return pose, sincos, goals


def views_for(W, H, m):
    """Centred on the origin, at negative coordinates, and far off anything."""
    return [(0.0, 0.0, m), (-13.37, -7.25, m), (0.4 * W * m, -0.45 * H * m, m)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("m", SCALES)
def test_scatter_equals_gather(shim, size, m):
    W, H = size
    rng = np.random.default_rng(int(m * 1000) + W)
    for view in views_for(W, H, m):
        pose, sincos, goals = edge_cases(view, W, H, rng)
        seen = set()
        for layers in (RR.BODIES, RR.GOALS, RR.GOALS | RR.BODIES):
            want = RR.gather_ids(view, W, H, layers, None, pose, sincos, goals)
            got = scatter(shim, view, W, H, layers, pose, sincos, goals)
            assert np.array_equal(got, want), (view, layers, np.argwhere(got != want)[:5])
            seen |= set(np.unique(want >> 24).tolist())
        # (the cases show every layer; the nose only where a pixel is smaller than it)
        assert seen >= {0, RR.L_GOAL, RR.L_BODY} | ({RR.L_NOSE} if m < 0.11 else set()), seen
        # the order of the robots and the number of lanes sharing one do not show
        again = scatter(shim, view, W, H, layers, pose, sincos, goals, lanes=64, order=rng.permutation(len(pose)))
        assert np.array_equal(again, want)


def test_sub_pixel_robots_are_never_lost(shim):
    """2 m per pixel: a robot is a fraction of a pixel and no pixel centre may fall inside it -- the pixel containing its
    centre is marked all the same, by the higher index where two share one."""
    W, H, view = 70, 45, (0.0, 0.0, 2.0)
    rng = np.random.default_rng(5)
    pose = rng.uniform(-40, 40, (30, 2)).astype(np.float32)
    pose[7] = pose[3]
    sincos = np.tile(np.array([[0.0, 1.0]], np.float32), (30, 1))
    ids = scatter(shim, view, W, H, RR.BODIES, pose, sincos, pose)
    for i, (x, y) in enumerate(pose):
        col, row = RR.pixel_of(view, W, H, x, y)
        assert ids[row, col] >> 24 >= RR.L_BODY and (ids[row, col] & 0xFFFFFF) >= i
    col, row = RR.pixel_of(view, W, H, *pose[3])
    assert ids[row, col] & 0xFFFFFF == 7
    assert np.array_equal(ids, RR.gather_ids(view, W, H, RR.BODIES, None, pose, sincos, pose))


def test_pixel_of_agrees(shim):
    rng = np.random.default_rng(11)
    W, H = 70, 45
    for m in SCALES:
        view = (1.5, -2.25, m)
        for x, y in rng.uniform(-0.6 * W * m, 0.6 * W * m, (200, 2)) + (1.5, -2.25):
            col, row = C.c_int32(-1), C.c_int32(-1)
            ok = shim.shim_pixel_of(W, H, *view, x, y, C.byref(col), C.byref(row))
            want = RR.pixel_of(view, W, H, x, y)
            assert (None if not ok else (col.value, row.value)) == want


@pytest.mark.parametrize("size", SIZES)
def test_map_layer_windows_on_and_off_the_map(shim, size):
    W, H = size
    rng = np.random.default_rng(W)
    grid = S.GridData.from_dense(rng.random((40, 40)) < 0.3, 0.25, -5.0, -5.0)
    bits = np.ascontiguousarray(grid.bits, np.uint32)
    seen = set()
    # inside the map, straddling its edges and corner, wholly off it; cells of several and of a fraction of a pixel
    for view in [(0.0, 0.0, 1.0 / 16.0), (0.0, 0.0, 0.3), (-5.0, 5.0, 0.05), (4.0, -6.0, 0.3), (0.0, 0.0, 2.0), (80.0, 3.0, 0.3),
                 (-3.0, -40.0, 0.05)]:
        got = np.zeros((H, W), np.uint32)
        shim.shim_map(W, H, *view, grid.x0, grid.y0, grid.cell, grid.width, grid.height, grid.words_per_row,
                      _ptr(bits, C.c_uint32), _ptr(got, C.c_uint32))
        want = RR.map_layer(view, W, H, grid)
        assert np.array_equal(got, want.astype(np.uint32) << 24), view
        seen.add((bool(want.any()), bool(want.all())))
    assert (False, False) in seen and (True, False) in seen      # a window off the map shows nothing, others show walls


def test_palette_is_the_documented_table(shim):
    def rgb(*a):
        v = shim.shim_rgb(*a)
        return v & 255, (v >> 8) & 255, (v >> 16) & 255

    assert rgb(0, 0, 0, 0, 1) == RR.BACKGROUND == (255, 255, 255)
    assert rgb(0, 3, 0, 0, 1) == RR.TRAIL_RGB
    assert rgb(1 << 24, 3, 0, 0, 1) == RR.MAP_RGB                   # the trail shows only where nothing else is
    assert rgb(3 << 24 | 5, 0, 0, 0, 1) == RR.BEAM_WALL_RGB and rgb(4 << 24 | 5, 0, 0, 0, 1) == RR.BEAM_ROBOT_RGB
    assert len(set(RR.HUES)) == 16
    for i in list(range(40)) + [50_000, (1 << 24) - 1]:
        h = RR.HUES[i % 16]
        assert rgb(2 << 24 | i, 0, 0, 0, 1) == tuple((c + 255) // 2 for c in h)
        assert rgb(5 << 24 | i, 0, 0, 0, 1) == h
        assert rgb(6 << 24 | i, 0, 0, 0, 1) == tuple(c // 2 for c in h)
        assert rgb(5 << 24 | i, 0, 1, 1, 0) == RR.CRASHED_RGB        # crashed beats reached beats not live
        assert rgb(5 << 24 | i, 0, 0, 1, 0) == RR.REACHED_RGB
        assert rgb(5 << 24 | i, 0, 0, 2, 1) == h                     # only REACH turns a body green
        assert rgb(5 << 24 | i, 0, 0, 0, 0) == tuple(c // 4 + 144 for c in h)
        assert rgb(6 << 24 | i, 9, 1, 0, 1) == tuple(c // 2 for c in RR.CRASHED_RGB)
        for layer in range(7):
            for st in [(0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 0), (0, 3, 0)]:
                assert rgb(layer << 24 | i, 0, *st) == RR.colour(layer, i, 0, *st)


def test_bad_arguments_are_refused_without_a_device(built_lib):
    """Every check that does not need the env runs before the env is looked at, and all of them before the first HIP call."""
    from mrca import _lib
    lib = _lib.load()
    one = (_lib.RenderView * 1)(_lib.RenderView(0, 0.0, 0.0, 0.1))
    ids = C.c_void_p(0x1000)        # never dereferenced: the call fails first

    def call(views=one, n=1, w=8, h=8, layers=7, ids=ids, trail=None, rgb=None):
        rc = lib.mrca_render(None, views, n, w, h, layers, ids, trail, rgb, None)
        return rc, lib.mrca_last_error().decode()

    assert call() == (-1, "env is NULL")
    for kw, text in [(dict(n=0), "num_views"), (dict(n=257), "num_views"), (dict(w=0), "image size"), (dict(h=4097), "image size"),
                     (dict(w=-3), "image size"), (dict(layers=16), "layer bits"), (dict(layers=0x80000001), "layer bits"),
                     (dict(ids=None), "ids_dev is NULL")]:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        rc, msg = call(views=(_lib.RenderView * 1)(_lib.RenderView(0, 0.0, 0.0, bad)))
        assert rc == -1 and "m_per_px" in msg, (bad, msg)
