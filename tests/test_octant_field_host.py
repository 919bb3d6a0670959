"""The octant free-rectangle field (csrc/mrca_host.h: build_octant_rect_field) and the march over it (csrc/mrca_device.h:
grid_march_skip / grid_march_skip_n with FreeRectField's shift 4, major 8), compiled for the host:

* soundness -- every one of the eight rectangles of every empty cell holds no occupied cell, extents <= 254, occupied cells
  flagged in all eight entries, the border zero;
* exactness -- the march whose first jump takes the origin cell's QUADRANT entry and whose later lookups read the octant array
  returns the bits of the cell-by-cell grid_march, one ray at a time and two in lock step;
* the point of it -- on the seeded Stage-1 sample (3000 poses in the free cells of the +-9 m square, 512 beams, waves of 64
  consecutive beams, trips counted as the kernel's loop takes them) the trips per wave are at least 4 % below the quadrant
  array's.  (Measured: 2.882 -> 2.659, 7.7 %, profiles/octant_field/field_probe.txt; the bar guards against a builder that
  quietly degenerates, it is not the performance claim.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util as U
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")

SHIM = r"""
#include <cmath>
#include <random>
#include <vector>
#include "mrca_host.h"
using namespace mrca;

struct Ctx {
    std::vector<uint32_t> bits;
    GridGeom g;
    std::vector<uint16_t> quad, oct;
    int pitch;
    FreeRectField qf() const { return FreeRectField{quad.data(), g.width, g.height, pitch}; }
    FreeRectField of() const { return FreeRectField{oct.data(), g.width, g.height, pitch, 4u, 8u}; }
};
// a field that counts its lookups and remembers the last entry it returned
struct Counting {
    FreeRectField f;
    mutable int lookups = 0;
    mutable uint32_t last = 0;
    uint32_t entry_bytes(float dx, float dy) const { return f.entry_bytes(dx, dy); }
    uint32_t operator()(int ix, int iy, uint32_t qb) const { ++lookups; return last = f(ix, iy, qb); }
};

extern "C" {
void octant_pads(int* px, int* py, int* max_extent) { *px = kFieldPadX; *py = kFieldPadY; *max_extent = kFieldMaxExtent; }
Ctx* octant_new(const uint32_t* bits, int w, int h, int wpr, float cell, float x0, float y0) {
    Ctx* c = new Ctx;
    c->bits.assign(bits, bits + (size_t)h * wpr);
    c->g.x0 = x0; c->g.y0 = y0; c->g.cell = cell; c->g.inv_cell = 1.0f / cell;
    c->g.width = w; c->g.height = h; c->g.wpr = wpr;
    int p2 = 0;
    build_free_rect_field(c->bits.data(), w, h, wpr, &c->quad, &c->pitch);
    build_octant_rect_field(c->bits.data(), w, h, wpr, &c->oct, &p2);
    if (p2 != c->pitch) { delete c; return nullptr; }
    return c;
}
void octant_free(Ctx* c) { delete c; }
// the padded octant array [(h + 2 py)][pitch][8]
long long octant_copy(const Ctx* c, uint16_t* out, long long cap) {
    if ((long long)c->oct.size() > cap) return -1;
    std::copy(c->oct.begin(), c->oct.end(), out);
    return (long long)c->oct.size();
}
// plain: grid_march over the bitmap; one: grid_march_skip; two: grid_march_skip_n<2> with ray i + 1's direction as the partner;
// quad: grid_march_skip over the quadrant array (what MRCA_FIELD_OCTANTS=0 runs)
void octant_march(const Ctx* c, int n, const float* ox, const float* oy, const float* dx, const float* dy, const float* tmax,
                  float* plain, float* one, float* two, float* quad) {
    const GlobalGrid occ{c->bits.data(), c->g.width, c->g.height, c->g.wpr};
    const FreeRectField qf = c->qf(), of = c->of();
    for (int i = 0; i < n; ++i) {
        plain[i] = grid_march(occ, c->g, ox[i], oy[i], dx[i], dy[i], tmax[i]);
        const MarchOrigin org = march_origin(qf, c->g, ox[i], oy[i]);     // the head record's quadrant entries
        one[i] = grid_march_skip(of, c->g, org, dx[i], dy[i], tmax[i]);
        quad[i] = grid_march_skip(qf, c->g, org, dx[i], dy[i], tmax[i]);
        const float ddx[2] = {dx[i], dx[(i + 1) % n]}, ddy[2] = {dy[i], dy[(i + 1) % n]};
        float o[2];
        grid_march_skip_n<2>(of, c->g, org, ddx, ddy, tmax[i], o);
        two[i] = o[0];
    }
}
// seeded lidar sample: `robots` poses uniform in the free cells of the +-half square, 512 beams over the front half circle.
// out: lookups per beam and trips per wave (64 consecutive beams) and beam -- quadrant array, then octant array
void octant_trips(const Ctx* c, int robots, unsigned seed, float half, double* out) {
    const GlobalGrid occ{c->bits.data(), c->g.width, c->g.height, c->g.wpr};
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> Un(-1.0f, 1.0f);
    long long looks[2] = {0, 0}, trips[2] = {0, 0}, waves = 0, beams = 0;
    for (int r = 0; r < robots; ++r) {
        float x, y;
        do {
            x = Un(rng) * half;
            y = Un(rng) * half;
        } while (occ((int)std::floor((x - c->g.x0) * c->g.inv_cell), (int)std::floor((y - c->g.y0) * c->g.inv_cell)));
        const float th = Un(rng) * 3.14159265f;
        const MarchOrigin org = march_origin(c->qf(), c->g, x, y);
        int wmax[2] = {0, 0};
        for (int b = 0; b < 512; ++b) {
            const double a = th - M_PI / 2 + b * M_PI / 511;
            const float dx = (float)std::cos(a), dy = (float)std::sin(a);
            for (int f = 0; f < 2; ++f) {
                Counting cf{f ? c->of() : c->qf()};
                const uint32_t vq = dy > 0.0f ? org.v_hi : org.v_lo;
                cf.last = dx > 0.0f ? vq >> 16 : vq & 0xFFFFu;
                (void)grid_march_skip(cf, c->g, org, dx, dy, 6.0f);
                // a trip looks up once unless it is the one that finds the beam's end (t >= tmax); a hit ends in a lookup
                const int t = cf.lookups + (cf.last == kCellOccupied ? 0 : 1);
                looks[f] += cf.lookups;
                wmax[f] = std::max(wmax[f], t);
            }
            ++beams;
            if ((b & 63) == 63) {
                trips[0] += wmax[0]; trips[1] += wmax[1]; ++waves;
                wmax[0] = wmax[1] = 0;
            }
        }
    }
    out[0] = (double)looks[0] / beams; out[1] = (double)trips[0] / waves;
    out[2] = (double)looks[1] / beams; out[3] = (double)trips[1] / waves;
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("octant_field")
    src, so = d / "shim.cpp", d / "liboctant.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", "-shared",
                    "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    so = C.CDLL(str(so))
    so.octant_new.restype = C.c_void_p
    so.octant_new.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    so.octant_free.argtypes = [C.c_void_p]
    so.octant_copy.restype = C.c_longlong
    so.octant_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    so.octant_march.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
    so.octant_trips.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_void_p]
    return so


def random_map(seed):
    """96 x 80 cells of 0.1 m: boxes, walls with a one-cell gap, one-cell corridors between two walls, diagonal staircases of both
    slopes (one cell wide: corner-touching cells a diagonal ray passes between)"""
    rng = np.random.default_rng(seed)
    h, w = 80, 96
    occ = np.zeros((h, w), bool)
    for _ in range(6):
        x, y = rng.integers(0, w - 8), rng.integers(0, h - 8)
        occ[y:y + rng.integers(1, 8), x:x + rng.integers(1, 8)] = True
    for _ in range(3):                      # a corridor one cell wide, horizontal or vertical, with a gap in one wall
        x, y, n = rng.integers(2, w - 40), rng.integers(2, h - 40), rng.integers(10, 36)
        if rng.integers(0, 2):
            occ[y, x:x + n] = occ[y + 2, x:x + n] = True
            occ[y, x + n // 2] = False
        else:
            occ[y:y + n, x] = occ[y:y + n, x + 2] = True
            occ[y + n // 2, x + 2] = False
    for _ in range(4):                      # staircases: slope +-1 and +-2, one cell thick
        x, y, n = rng.integers(5, w - 45), rng.integers(5, h - 45), rng.integers(10, 36)
        sy, step = (1 if rng.integers(0, 2) else -1), int(rng.integers(1, 3))
        for i in range(n):
            yy = y + (sy * i if sy > 0 else 35 - i)
            occ[yy, x + i // step if step > 1 else x + i] = True
    return S.GridData.from_dense(occ, 0.1, -4.8, -4.0)


def maps():
    yield "stage1", S.stage1(1, 2).grid
    yield "stage2", S.stage2(1).grid
    yield "circle", S.circle(1).grid
    for seed in (1, 2, 3):
        yield f"random{seed}", random_map(seed)
    yield "one_cell", S.GridData.from_dense(np.zeros((1, 1), bool), 0.5, -0.25, -0.25)
    yield "one_cell_occupied", S.GridData.from_dense(np.ones((1, 1), bool), 0.5, -0.25, -0.25)
    yield "all_empty", S.GridData.from_dense(np.zeros((37, 70), bool), 0.1, -3.5, -1.85)
    yield "all_occupied", S.GridData.from_dense(np.ones((37, 70), bool), 0.1, -3.5, -1.85)


MAPS = dict(maps())


@pytest.fixture(scope="module")
def ctxs(lib):
    made = {}

    def get(name):
        if name not in made:
            g = MAPS[name]
            bits = np.ascontiguousarray(g.bits, np.uint32)
            made[name] = (lib.octant_new(bits.ctypes.data, g.width, g.height, g.words_per_row, g.cell, g.x0, g.y0), bits)
            assert made[name][0]
        return made[name][0]
    yield get
    for c, _bits in made.values():
        lib.octant_free(c)


@pytest.mark.parametrize("name", list(MAPS))
def test_octant_field_is_sound(lib, ctxs, name):
    g = MAPS[name]
    px, py, emax = C.c_int(), C.c_int(), C.c_int()
    lib.octant_pads(C.byref(px), C.byref(py), C.byref(emax))
    px, py = px.value, py.value
    assert emax.value == 254
    buf = np.full((g.height + 2 * py) * (g.width + 2 * px) * 8, 0xABCD, np.uint16)
    assert lib.octant_copy(ctxs(name), buf.ctypes.data, buf.size) == buf.size
    padded = buf.reshape(g.height + 2 * py, g.width + 2 * px, 8)
    border = np.ones(padded.shape[:2], bool)
    border[py:py + g.height, px:px + g.width] = False
    assert (padded[border] == 0).all()
    f = padded[py:py + g.height, px:px + g.width]
    occ = g.dense()
    assert ((f == 0xFFFF).all(axis=2) == occ).all() and ((f == 0xFFFF).any(axis=2) == occ).all()
    sat = np.pad(occ.astype(np.int64).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    ys, xs = np.nonzero(~occ)
    if len(ys) == 0:
        return
    for k in range(8):
        q = k & 3
        sx, sy = (1 if q & 1 else -1), (1 if q & 2 else -1)
        v = f[ys, xs, k].astype(np.int64)
        ex, ey = v & 255, v >> 8
        assert ex.max() <= 254 and ey.max() <= 254
        xa, xb = xs, xs + sx * ex
        ya, yb = ys, ys + sy * ey
        x0 = np.clip(np.minimum(xa, xb), 0, g.width - 1)
        x1 = np.clip(np.maximum(xa, xb), 0, g.width - 1)
        y0 = np.clip(np.minimum(ya, yb), 0, g.height - 1)
        y1 = np.clip(np.maximum(ya, yb), 0, g.height - 1)
        cnt = sat[y1 + 1, x1 + 1] - sat[y0, x1 + 1] - sat[y1 + 1, x0] + sat[y0, x0]
        assert (cnt == 0).all(), k
    if name in ("stage1", "stage2", "circle"):
        # the bias is there: the x-major entries are longer in x than the y-major ones, and the other way round
        ex = (f[ys, xs] & 255).astype(np.int64)
        ey = (f[ys, xs] >> 8).astype(np.int64)
        assert ex[:, 4:].mean() > ex[:, :4].mean() and ey[:, :4].mean() > ey[:, 4:].mean()


def rays(g, n, rng):
    """n >= 200 000 seeded rays: random ones, the eight compass directions, +-0 components, |dx| == |dy| exactly, origins on cell
    faces, on corners and outside the map, tmax 0 / denormal / the outline walks' 0.38 and 0.44 m, and rays that graze a wall:
    from a face of an empty cell next to an occupied one, along the wall and a hair toward or away from it"""
    cell = np.float32(g.cell)
    ox = rng.uniform(g.x0 - 2, g.x0 + g.width * g.cell + 2, n).astype(np.float32)
    oy = rng.uniform(g.y0 - 2, g.y0 + g.height * g.cell + 2, n).astype(np.float32)
    th = rng.uniform(-np.pi, np.pi, n)
    th[:4000] = rng.integers(0, 8, 4000) * np.pi / 4
    dx = np.cos(th).astype(np.float32)
    dy = np.sin(th).astype(np.float32)
    dx[:1000] = np.where(np.abs(dx[:1000]) < 1e-6, 0, dx[:1000])
    dy[:1000] = np.where(np.abs(dy[:1000]) < 1e-6, 0, dy[:1000])
    dx[1000:1500] = np.where(np.abs(dx[1000:1500]) < 1e-6, np.float32(-0.0), dx[1000:1500])      # -0 components
    dy[1500:2000] = np.where(np.abs(dy[1500:2000]) < 1e-6, np.float32(-0.0), dy[1500:2000])
    # exactly diagonal: |dx| == |dy| bit for bit, every sign combination, unit and non-unit lengths
    k = slice(20000, 30000)
    dy[k] = np.abs(dx[k]) * rng.choice(np.array([-1, 1], np.float32), 10000)
    assert (np.abs(dx[k]) == np.abs(dy[k])).all()
    ox[4000:12000] = (g.x0 + rng.integers(-1, g.width + 2, 8000) * cell).astype(np.float32)       # faces; 8000:12000 corners
    oy[8000:16000] = (g.y0 + rng.integers(-1, g.height + 2, 8000) * cell).astype(np.float32)
    ox[24000:28000] = (g.x0 + rng.integers(0, g.width + 1, 4000) * cell).astype(np.float32)       # diagonal rays from corners
    oy[24000:28000] = (g.y0 + rng.integers(0, g.height + 1, 4000) * cell).astype(np.float32)
    # grazing rays
    occ = g.dense()
    pad = np.pad(occ, 1)
    near = ~occ & (pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:] | pad[:-2, :-2] | pad[2:, 2:] | pad[:-2, 2:] | pad[2:, :-2])
    ys, xs = np.nonzero(near)
    if len(ys):
        m = 40000
        k = slice(40000, 40000 + m)
        pick = rng.integers(0, len(ys), m)
        fx = rng.choice(np.array([0.0, 0.0, 0.5, 1.0]), m)          # on a face, mid cell, on the far face
        fy = rng.choice(np.array([0.0, 0.0, 0.5, 1.0]), m)
        ox[k] = (g.x0 + (xs[pick] + fx) * g.cell).astype(np.float32)
        oy[k] = (g.y0 + (ys[pick] + fy) * g.cell).astype(np.float32)
        base = rng.integers(0, 8, m) * np.pi / 4                     # along a wall or along a staircase ...
        tilt = rng.choice(np.array([0.0, 1e-7, -1e-7, 1e-4, -1e-4, 3e-3, -3e-3, 0.02, -0.02]), m)   # ... and a hair off it
        dx[k] = np.cos(base + tilt).astype(np.float32)
        dy[k] = np.sin(base + tilt).astype(np.float32)
    tmax = np.full(n, 6.0, np.float32)
    tmax[::7] = rng.uniform(0, 6, len(tmax[::7])).astype(np.float32)
    tmax[::11] = 0.44
    tmax[::13] = 0.38
    tmax[::101] = 0.0
    tmax[::103] = np.float32(1e-40)       # denormal
    tmax[::107] = np.float32(1.4e-45)     # the smallest one
    return ox, oy, dx, dy, tmax


@pytest.mark.parametrize("name", list(MAPS))
def test_march_over_the_octant_field_equals_the_plain_walk(lib, ctxs, name):
    g = MAPS[name]
    n = 200000
    rng = np.random.default_rng(sorted(MAPS).index(name) + 17)
    ox, oy, dx, dy, tmax = rays(g, n, rng)
    plain, one, two, quad = (np.empty(n, np.float32) for _ in range(4))
    P = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    lib.octant_march(ctxs(name), n, P(ox), P(oy), P(dx), P(dy), P(tmax), P(plain), P(one), P(two), P(quad))
    for what, got in (("grid_march_skip", one), ("grid_march_skip_n<2>", two), ("grid_march_skip over the quadrant array", quad)):
        same = got.view(np.uint32) == plain.view(np.uint32)
        assert same.all(), f"{what}: {(~same).sum()} rays differ, first at {np.argwhere(~same)[0]}"
    if name in ("stage1", "stage2", "circle") or name.startswith("random"):
        assert 0.05 < (plain < tmax).mean() < 0.95          # the sample has both hits and misses


def test_octants_take_fewer_trips_on_the_stage1_sample(lib, ctxs):
    out = np.zeros(4, np.float64)
    lib.octant_trips(ctxs("stage1"), 3000, 1, 9.0, out.ctypes.data)
    q_looks, q_trips, o_looks, o_trips = out
    print(f"stage1, 3000 poses x 512 beams: quadrant {q_looks:.3f} lookups / beam, {q_trips:.3f} trips / wave; "
          f"octant {o_looks:.3f}, {o_trips:.3f} ({100 * (1 - o_trips / q_trips):.1f} % fewer trips)")
    assert 2.0 < q_trips < 4.0                  # the sample is a lidar's: a few trips per wave
    assert o_trips <= 0.96 * q_trips
    assert o_looks < q_looks
