"""The cull's beam interval as the device forms it (csrc/mrca_device.h: beam_interval_approx -- ratio = radius * rsq(d2), the near
test on the squares, a = mn * rcp(mx)), compiled for the host with rcp / rsq = the exact value scaled by (1 + k 2^-23) for every
pair of k in {-2, 0, 2}: the hardware's documented error is 1 ulp, this is twice that.  Held against the rectangle itself and against
the exact form (beam_interval, the host's):

  * every beam whose ray_box is finite lies inside [lo, hi];
  * lo and hi are within one beam of the exact form's -- a condition: it bounds how far the number of tested pairs can grow;

with 512, 64 and 1024 beams and both parameter sets -- (radius, near) = (0.2917, 0.30) and fidelity mode's at a 0.2 m raster --
over the neighbour positions of test_geometry_properties.test_beam_interval_never_culls_a_hit and: distances either side of
`near` and of the reach, bearings on the axes (mn = 0) and the diagonals (mn = mx) bit for bit, bearings at +-pi (ly = +-0).

"Either side of near": the exact form tests sqrtf(d2) <= near, the device form d2 <= near * near.  Their roundings (d2: 1.5 ulp,
near * near: 0.5 ulp, the square root halves a relative error) cannot part them where the distance is two fp32 steps or more from
`near`; nearer than that they may take different branches, one the whole row and one +-1.5 rad, and either is safe.  So the
positions from 2 to 64 steps either side are held to both conditions, and the positions at `near` itself and one step either side
to the first one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f = np.float32

SHIM = r"""
#include <math.h>
#include "mrca_device.h"

struct ScaledOps {       // the exact value, scaled and rounded once
    double rcp_scale, rsq_scale;
    float rcp(float v) const { return (float)((1.0 / (double)v) * rcp_scale); }
    float rsq(float v) const { return (float)((1.0 / sqrt((double)v)) * rsq_scale); }
};

extern "C" void interval_exact(int n, const float* lx, const float* ly, int beams, float step, float inv_step, float radius,
                               float near, int* lo, int* hi) {
    for (int i = 0; i < n; ++i) mrca::beam_interval(lx[i], ly[i], beams, step, inv_step, radius, near, &lo[i], &hi[i]);
}
extern "C" void interval_device_form(int n, const float* lx, const float* ly, int beams, float step, float inv_step, float radius,
                                     float near, int k_rcp, int k_rsq, int* lo, int* hi) {
    const ScaledOps ops{1.0 + k_rcp * ldexp(1.0, -23), 1.0 + k_rsq * ldexp(1.0, -23)};
    for (int i = 0; i < n; ++i)
        mrca::beam_interval_approx(lx[i], ly[i], beams, step, inv_step, radius, near, ops, &lo[i], &hi[i]);
}
// the first and last beam of a sensor at the origin, heading 0, whose ray_box against the neighbour is finite (beams, -1: none)
extern "C" void hit_range(int n, const float* lx, const float* ly, const float* sj, const float* cj, int beams, const float* bc,
                          const float* bs, int* first, int* last) {
    for (int i = 0; i < n; ++i) {
        first[i] = beams;
        last[i] = -1;
        for (int b = 0; b < beams; ++b)
            if (isfinite(mrca::ray_box(0.0f, 0.0f, bc[b], bs[b], lx[i], ly[i], sj[i], cj[i]))) {
                if (first[i] == beams) first[i] = b;
                last[i] = b;
            }
    }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_interval")
    src, so = d / "shim.cpp", d / "libprep_interval.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I", CSRC, "-shared",
                    "-fPIC", str(src), "-o", str(so)], check=True, capture_output=True)
    return C.CDLL(str(so))


def P(a):
    return C.c_void_p(a.ctypes.data)


def steps_from(x, ks):
    """the fp32 numbers k steps above x > 0"""
    return (np.array([x], f).view(np.int32) + np.asarray(ks, np.int32)).view(f)


# (radius, near, reach) as mrca_create forms them: the circumscribed circle + 1 mm; fidelity mode: + one raster-cell diagonal
def parameters(raster):
    radius = f(0.2917) if raster is None else f(f(0.2917) + f(f(1.4143) * f(raster)))
    near = f(0.30) if raster is None else f(radius + f(0.01))
    reach = f(f(6.0) + f(0.2907)) if raster is None else f(f(f(6.0) + radius) + f(0.01))
    return radius, near, reach


def positions(near, reach):
    """(lx, ly, both): the neighbour centres in the sensor's frame; both = held to the exact form as well"""
    rng = np.random.default_rng(0)
    n = 4000
    # test_beam_interval_never_culls_a_hit's: anywhere within reach, very close, behind, clustered on the axes
    r = np.concatenate([rng.uniform(0.45, 6.6, n - 600), rng.uniform(0.4, 0.7, 600)])
    phi = rng.uniform(-np.pi, np.pi, n)
    phi[:400] = rng.choice([-np.pi / 2, np.pi / 2, 0.0, np.pi], 400) + rng.normal(0, 0.02, 400)
    lx, ly = [(r * np.cos(phi)).astype(f)], [(r * np.sin(phi)).astype(f)]
    both = [np.ones(n, bool)]
    # bearings on the axes (mn = 0), the diagonals (mn = mx) and at +-pi (ly = +-0), bit for bit, at distances across the range
    for d in np.concatenate([np.geomspace(float(near) * 1.02, float(reach), 40), rng.uniform(0.4, 6.6, 60)]).astype(f):
        h = f(d * f(np.sqrt(0.5)))
        for x, y in ((d, 0), (-d, 0), (0, d), (0, -d), (h, h), (h, -h), (-h, h), (-h, -h), (-d, f(-0.0)), (-d, f(0.0)), (d, f(-0.0))):
            lx.append(np.array([x], f))
            ly.append(np.array([y], f))
            both.append(np.ones(1, bool))
    # either side of `near` and of the reach: along the axes the distance is the coordinate itself, elsewhere the positions are
    # sorted by their true distance (float64 of the fp32 coordinates)
    near_steps = np.concatenate([np.arange(-64, -1), np.arange(2, 65)])
    for ks, held in ((near_steps, True), (np.array([-1, 0, 1]), False)):
        d = steps_from(near, ks)
        for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            lx.append((d * f(sx)).astype(f))
            ly.append((d * f(sy)).astype(f))
            both.append(np.full(len(d), held))
    ang = rng.uniform(-np.pi, np.pi, 3000)
    dd = float(near) * (1.0 + rng.uniform(-8e-6, 8e-6, 3000))
    ax, ay = (dd * np.cos(ang)).astype(f), (dd * np.sin(ang)).astype(f)
    true = np.hypot(ax.astype(np.float64), ay.astype(np.float64))
    off = np.abs(true - float(near)) / float(np.spacing(near))
    lx.append(ax)
    ly.append(ay)
    both.append(off >= 2.0)
    dr = float(reach) * (1.0 + rng.uniform(-4e-6, 4e-6, 1000))
    ang = rng.uniform(-np.pi, np.pi, 1000)
    lx.append((dr * np.cos(ang)).astype(f))
    ly.append((dr * np.sin(ang)).astype(f))
    both.append(np.ones(1000, bool))
    return np.concatenate(lx), np.concatenate(ly), np.concatenate(both)


@pytest.mark.parametrize("raster", [None, 0.2], ids=["exact_rectangles", "fidelity_0.2m"])
@pytest.mark.parametrize("beams", [512, 64, 1024])
def test_the_device_form_keeps_every_hit_and_stays_within_a_beam_of_the_exact_form(lib, beams, raster):
    radius, near, reach = parameters(raster)
    assert near > radius                # (what lets the device form go without the ratio's clamp)
    lx, ly, both = positions(near, reach)
    n = len(lx)
    assert both.sum() > 0.95 * n and (~both).sum() >= 12
    rng = np.random.default_rng(1)
    sj, cj = O.sincos(rng.uniform(-np.pi, np.pi, n).astype(f), f)
    bc, bs = O.beam_table(f, beams)
    step, inv_step = f(f(np.pi) / f(beams - 1)), f(f(beams - 1) / f(np.pi))
    first, last = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.hit_range(n, P(lx), P(ly), P(sj), P(cj), beams, P(bc), P(bs), P(first), P(last))
    hit = last >= 0
    assert hit.sum() > n // 4
    lo0, hi0 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.interval_exact(n, P(lx), P(ly), beams, C.c_float(step), C.c_float(inv_step), C.c_float(radius), C.c_float(near), P(lo0), P(hi0))
    assert (lo0[hit] <= first[hit]).all() and (last[hit] <= hi0[hit]).all()        # (the exact form itself)
    worst = 0
    for k_rcp in (-2, 0, 2):
        for k_rsq in (-2, 0, 2):
            lo, hi = np.zeros(n, np.int32), np.zeros(n, np.int32)
            lib.interval_device_form(n, P(lx), P(ly), beams, C.c_float(step), C.c_float(inv_step), C.c_float(radius), C.c_float(near),
                                     k_rcp, k_rsq, P(lo), P(hi))
            what = (beams, raster, k_rcp, k_rsq)
            assert (0 <= lo).all() and (hi <= beams - 1).all(), what
            bad = hit & ((lo > first) | (last > hi))
            assert not bad.any(), (what, [(lx[i], ly[i], lo[i], hi[i], first[i], last[i]) for i in np.nonzero(bad)[0][:5]])
            # an empty interval (the neighbour behind the sensor) may be empty in another way: what is compared is the kept beams
            kept0, kept = lo0 <= hi0, lo <= hi
            off = np.where(kept0 & kept, np.maximum(np.abs(lo - lo0), np.abs(hi - hi0)),
                           np.where(kept0 | kept, np.maximum(hi - lo + 1, hi0 - lo0 + 1), 0))
            worst = max(worst, int(off[both].max()))
            far = both & (off > 1)
            assert not far.any(), (what, [(lx[i], ly[i], lo[i], hi[i], lo0[i], hi0[i]) for i in np.nonzero(far)[0][:5]])
    print(f"beams {beams} raster {raster}: lo / hi at most {worst} beam(s) from the exact form's over {int(both.sum())} positions")
