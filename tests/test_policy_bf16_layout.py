"""CPU: the data movement of the bf16 front end (csrc/mrca_policy_bf16.hip) re-enacted with the formulas of
csrc/mrca_policy_bf16_layout.h before any GPU time is spent.  A shim around the header is compiled with the host C++
compiler; NumPy then plays one wave: the scan staged into the LDS image, conv1's B operands gathered with the bf16 lane
maps (lane l holds A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31]), h1 stored and conv2's operands gathered from
the SAME image (the scan lives inside it: a layout that let a tile overwrite rows a later tile reads would show here),
the output transposed through it.  Every MFMA is summed in float64 over the same bf16 products as the float64 reference
of tests/bf16_ref.py, so the two must agree bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bf16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")

FUNCS = {  # name: arity
    "rowmap": 2, "x_stage_off": 1, "conv1_b_off": 3, "conv1_ci": 3, "conv1_tap": 3, "h1_store_off": 3, "conv2_a_off": 3,
    "conv2_ci": 3, "conv2_tap": 1, "out_store_off": 4, "out_load_off": 2, "out_feat_elem": 2,
}
CONSTS = ["kWaveBytes", "kXOff", "kOOff", "kOPitch", "kHRowBytes", "kHRows"]


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("bf16_layout")
    src = ['#include "mrca_policy_bf16_layout.h"', "using namespace mrca_pbf16;", 'extern "C" {']
    for name, k in FUNCS.items():
        args = ", ".join(f"int a{i}" for i in range(k))
        call = ", ".join(f"a{i}" for i in range(k))
        src.append(f"int L_{name}({args}) {{ return {name}({call}); }}")
    for c in CONSTS:
        src.append(f"int C_{c}() {{ return {c}; }}")
    src.append("}")
    (d / "shim.cpp").write_text("\n".join(src) + "\n")
    so = d / "libshim.so"
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "shim.cpp"), "-o", str(so)], check=True,
                   capture_output=True)
    lib = C.CDLL(str(so))

    class L:
        pass
    lay = L()
    for name, k in FUNCS.items():
        f = getattr(lib, f"L_{name}")
        f.argtypes, f.restype = [C.c_int] * k, C.c_int
        setattr(lay, name, f)
    for c in CONSTS:
        setattr(lay, c, getattr(lib, f"C_{c}")())
    return lay


class Image:
    """One wave's LDS image as bytes, read and written as bf16 values (float32 holding a bf16 value)"""

    def __init__(self, nbytes, rng):
        self.b = np.frombuffer(rng.bytes(nbytes), dtype=np.uint8).copy()       # LDS is not cleared: start with garbage

    def write(self, off, vals):
        assert off % 2 == 0 and 0 <= off and off + 2 * len(vals) <= self.b.size, off
        v = np.asarray(vals, dtype=np.float32)
        assert np.array_equal(R.rne_bf16(v), v) or np.isnan(v).any()
        self.b[off:off + 2 * len(v)] = (v.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)

    def read(self, off, n):
        assert off % 2 == 0 and 0 <= off and off + 2 * n <= self.b.size, off
        u = self.b[off:off + 2 * n].view(np.uint16).astype(np.uint32) << 16
        return u.view(np.float32)


def _mfma(A, B, acc):
    """v_mfma_f32_32x32x16_bf16 re-enacted: A[i][k] / B[k][j] assembled from the lanes' fragments, products summed in
    float64.  A_frag[l][j] = A[l & 31][8 (l >> 5) + j], B_frag[l][j] = B[8 (l >> 5) + j][l & 31]."""
    Am = np.zeros((32, 16))
    Bm = np.zeros((16, 32))
    for l in range(64):
        for j in range(8):
            Am[l & 31, 8 * (l >> 5) + j] = A[l][j]
            Bm[8 * (l >> 5) + j, l & 31] = B[l][j]
    return acc + Am @ Bm


def _reenact(lay, x, w1, b1, w2, b2, rng, robots):
    """One wave walking `robots` (one tower) through ONE image, as the kernel does -> f32[len(robots), 4096]"""
    img = Image(lay.kWaveBytes, rng)
    wa1 = [[[float(R.rne_bf16(w1[l & 31, lay.conv1_ci(mf, l >> 5, j), lay.conv1_tap(mf, l >> 5, j)])[0])
             if lay.conv1_ci(mf, l >> 5, j) >= 0 else 0.0 for j in range(8)] for l in range(64)] for mf in range(2)]
    wb2 = [[[float(R.rne_bf16(w2[l & 31, lay.conv2_ci(s, l >> 5, j), lay.conv2_tap(s)])[0]) for j in range(8)]
            for l in range(64)] for s in range(6)]
    zero_row = np.zeros(32, np.float32)
    img.write(0, zero_row)                                        # H[0], H[256]: once, before the first robot
    img.write((lay.kHRows - 1) * lay.kHRowBytes, zero_row)
    out = []
    for n in robots:
        xb = R.rne_bf16(x[n])                                     # [3, 512]
        for i in range(-1, 512):
            img.write(lay.x_stage_off(i), [0.0, 0.0, 0.0, 0.0] if i < 0 else [xb[0, i], xb[1, i], xb[2, i], 0.0])
        for t in range(8):
            B0, B1 = [], []
            for l in range(64):
                p, hl = 32 * t + (l & 31), l >> 5
                B0.append(img.read(lay.conv1_b_off(0, p, hl), 8))
                v = img.read(lay.conv1_b_off(1, p, 0), 4)
                B1.append(np.concatenate([v if hl == 0 else np.zeros(4, np.float32), np.zeros(4, np.float32)]))
            acc = np.repeat(b1.astype(np.float64)[:, None], 32, axis=1)              # C[channel][position]
            acc = _mfma(wa1[0], B0, acc)
            acc = _mfma(wa1[1], B1, acc)
            for l in range(64):
                p, hl = 32 * t + (l & 31), l >> 5
                if p >= 255:
                    continue
                for g in range(4):
                    chans = [lay.rowmap(4 * g + e, hl) for e in range(4)]
                    vals = R.rne_bf16(np.maximum(acc[chans, l & 31], 0.0).astype(np.float32))
                    img.write(lay.h1_store_off(p, g, hl), vals)
        accs = []
        for t in range(4):
            acc = np.repeat(b2.astype(np.float64)[None, :], 32, axis=0)             # C[position][channel]
            for s in range(6):
                A = [img.read(lay.conv2_a_off(s, 32 * t + (l & 31), l >> 5), 8) for l in range(64)]
                acc = _mfma(A, wb2[s], acc)
            accs.append(acc)
        for t in range(4):
            for l in range(64):
                c, hl = l & 31, l >> 5
                for g in range(4):
                    pos = [lay.rowmap(4 * g + e, hl) for e in range(4)]
                    img.write(lay.out_store_off(c, t, g, hl), R.rne_bf16(np.maximum(accs[t][pos, c], 0.0).astype(np.float32)))
        row = np.full(4096, np.nan, np.float32)
        for q in range(8):
            for l in range(64):
                e = lay.out_feat_elem(q, l)
                row[e:e + 8] = img.read(lay.out_load_off(q, l), 8)
        out.append(row)
    return np.stack(out)


def test_one_wave_reenacted_equals_the_rounding_point_reference(lay):
    rng = np.random.default_rng(7)
    n = 3
    x = (rng.random((n, 3, 512), dtype=np.float32) - 0.5).astype(np.float32)
    x[1, :, :5] = 0.0
    x[2, 2, -3:] = 1.25                                           # the right edge of the scan matters
    w1 = (0.3 * rng.standard_normal((32, 3, 5))).astype(np.float32)
    b1 = (0.05 * rng.standard_normal(32)).astype(np.float32)
    w2 = (0.15 * rng.standard_normal((32, 32, 3))).astype(np.float32)
    b2 = (0.05 * rng.standard_normal(32)).astype(np.float32)
    got = _reenact(lay, x, w1, b1, w2, b2, rng, robots=[0, 1, 2, 0])     # robot 0 again: nothing stale in the image
    want, exact, _S = R.front_end_ref(x, w1, b1, w2, b2)
    assert not np.isnan(got).any()
    assert float(np.abs(exact).max()) > 0.1 and (exact == 0).mean() < 0.9       # not a comparison between zeros
    np.testing.assert_array_equal(got[:3], want)
    np.testing.assert_array_equal(got[3], want[0])


def test_asymmetric_probe(lay):
    """One non-zero scan sample and one non-zero weight per layer land in exactly the outputs the convolution says
    (catches a transposed or shifted lane map that random data could average out)."""
    rng = np.random.default_rng(1)
    x = np.zeros((1, 3, 512), np.float32)
    x[0, 1, 100] = 1.0
    w1 = np.zeros((32, 3, 5), np.float32)
    w2 = np.zeros((32, 32, 3), np.float32)
    w1[5, 1, 3] = 2.0
    w2[9, 5, 0] = 3.0
    z = np.zeros(32, np.float32)
    got = _reenact(lay, x, w1, z, w2, z, rng, robots=[0])
    want, _e, _S = R.front_end_ref(x, w1, z, w2, z)
    assert int((want != 0).sum()) == 1
    np.testing.assert_array_equal(got, want)


def test_the_image_regions(lay):
    """The three uses of the one image stay apart where the kernel needs them apart."""
    assert lay.kWaveBytes * 9 <= 160 * 1024                      # 2 waves per SIMD leave room by LDS
    o_end = lay.out_load_off(7, 63) + 16
    assert lay.kOOff >= lay.kHRowBytes and o_end <= lay.kXOff     # O between H[0] and X
    assert lay.conv1_b_off(1, 255, 0) + 8 <= (lay.kHRows - 1) * lay.kHRowBytes     # X below H[256]
    assert lay.conv2_a_off(5, 127, 1) + 16 <= lay.kWaveBytes
    for off in [lay.conv1_b_off(0, p, h) for p in range(256) for h in range(2)] + \
               [lay.conv2_a_off(s, l, h) for s in range(6) for l in range(128) for h in range(2)] + \
               [lay.out_load_off(q, l) for q in range(8) for l in range(64)]:
        assert off % 16 == 0, off                                 # every 16-byte access aligned
