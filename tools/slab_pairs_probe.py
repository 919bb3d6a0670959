#!/usr/bin/env python3
"""What the ray cast's slab tests have to do in the worlds bench.py runs: neighbours, (neighbour, beam) pairs and wave-trips per
robot, beam-major against pair-major (host only, no GPU).

    python tools/slab_pairs_probe.py > profiles/slab_pairs/premise.txt

Seeded worlds are stepped by the C oracle under bench.py's random actions (v ~ U(0, 1), w ~ U(-1, 1)) and sampled at a few
ticks.  For every robot of a sample the preparing wave's work is redone with the header's OWN cull and beam_interval
(csrc/mrca_device.h compiled for the host with -ffp-contract=off): the kept neighbours, their intervals, then

  flagged       the kept neighbours (the list's length cnt)
  pairs P       the sum of the interval lengths
  trips now     what the beam-major loop runs: per group of 64 consecutive beams (a wave's) as many trips as its busiest beam has
                neighbours, summed over the beams / 64 groups
  trips dense   ceil(P / 64): the pairs dealt densely to lanes
  passes        ceil(P / 256): what one of a 512-beam workgroup's four waves runs of the pair loop at the most
  search trips  ceil(cnt / 8) (at least one): the trips of slab_pair_locate per pair

Printed: the mean per robot of every sample and the range of those means over the samples; the share of robots without a
neighbour (no second barrier), and the distribution of cnt.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("rl-collision-avoidance_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import util as U  # noqa: E402
from mrca import scenario as S  # noqa: E402

BUILD = os.path.join(ROOT, "tools", "_build")
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
TICKS = (0, 10, 25, 50, 100, 150, 200)

SHIM = r"""
#include <stdint.h>
#include "mrca_device.h"
// one world of R robots (pose [R][3]) -> per robot: cnt, P, the beam-major loop's wave-trips
extern "C" void slab_premise(int R, int B, const float* pose, int* cnt, int* P, int* trips_now) {
    static int per_beam[4096];
    for (int i = 0; i < R; ++i) {
        const float x = pose[3 * i], y = pose[3 * i + 1];
        float s, c;
        mrca::sincos_det(pose[3 * i + 2], &s, &c);
        for (int b = 0; b < B; ++b) per_beam[b] = 0;
        cnt[i] = P[i] = trips_now[i] = 0;
        for (int j = 0; j < R; ++j) {
            if (j == i) continue;
            const float ddx = pose[3 * j] - x, ddy = pose[3 * j + 1] - y;
            if (!(ddx * ddx + ddy * ddy <= mrca::kLidarReach2)) continue;
            int lo = 0, hi = -1;
            mrca::beam_interval(ddx * c + ddy * s, ddy * c - ddx * s, B, &lo, &hi);
            if (lo > hi) continue;
            ++cnt[i];
            P[i] += hi - lo + 1;
            for (int b = lo; b <= hi; ++b) ++per_beam[b];
        }
        for (int g = 0; g < B / 64; ++g) {
            int busiest = 0;
            for (int b = 64 * g; b < 64 * g + 64; ++b) busiest = per_beam[b] > busiest ? per_beam[b] : busiest;
            trips_now[i] += busiest;
        }
    }
}
"""


def build():
    os.makedirs(BUILD, exist_ok=True)
    src, so = os.path.join(BUILD, "slab_pairs_probe.cpp"), os.path.join(BUILD, "libslab_pairs_probe.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, src, "-o", so], check=True)
    return C.CDLL(so)


def sample(lib, sc, pose):
    R, B = sc.robots_per_world, sc.beams
    out = []
    for w in range(sc.num_worlds):
        p = np.ascontiguousarray(pose[w * R:(w + 1) * R], np.float32)
        cnt, P, now = (np.zeros(R, np.int32) for _ in range(3))
        lib.slab_premise(R, B, p.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                         now.ctypes.data_as(C.c_void_p))
        out.append(np.stack([cnt, P, now], 1))
    return np.concatenate(out)


def run(lib, title, sc, seed):
    ora = U.COracleEnv(sc)
    ora.reset()
    rng = np.random.default_rng(seed)
    rows, every = [], []
    print(f"## {title}: {sc.num_worlds} worlds x {sc.robots_per_world} robots, {sc.beams} beams, scenario seed {sc.seed}, action seed {seed}")
    print("tick   flagged  pairs P  trips now (per 64 beams)  trips dense  passes  search trips  alone")
    for k in range(max(TICKS) + 1):
        if k in TICKS:
            m = sample(lib, sc, np.asarray(ora.pose)).astype(np.float64)
            cnt, P, now = m[:, 0], m[:, 1], m[:, 2]
            dense, passes, search = np.ceil(P / 64), np.ceil(P / 256), np.maximum(np.ceil(cnt / 8), 1)
            row = (cnt.mean(), P.mean(), now.mean(), now.mean() / (sc.beams / 64), dense.mean(), passes.mean(), search.mean(),
                   (cnt == 0).mean())
            print("%4d   %7.2f  %7.1f  %9.2f (%4.2f)          %11.2f  %6.2f  %12.3f  %5.3f" % ((k,) + row))
            rows.append(row)
            every.append(m)
        ora.step(U.random_actions(rng, sc.num_robots))
    rows, every = np.array(rows), np.concatenate(every)
    print("range  %s" % "  ".join("%.2f - %.2f" % (lo, hi) for lo, hi in zip(rows.min(0), rows.max(0))))
    cnt = every[:, 0].astype(int)
    hist = np.bincount(cnt)
    print("cnt over all samples: max %d, over 8: %.4f of the robots; histogram %s" % (cnt.max(), (cnt > 8).mean(),
          " ".join("%d:%d" % (k, n) for k, n in enumerate(hist) if n)))
    print("P over all samples: max %d, over 256 (a second pass): %.4f of the robots" % (every[:, 1].max(), (every[:, 1] > 256).mean()))
    print()
    return rows


def main():
    lib = build()
    run(lib, "Stage-1", S.stage1(num_worlds=16, robots_per_world=32, seed=7), 1)
    run(lib, "Stage-2", S.stage2(num_worlds=4, seed=7), 1)


if __name__ == "__main__":
    main()
