#!/usr/bin/env python3
"""Sweep behind mrca_nhorca_default_params (profiles/nhorca/defaults.txt): the host build of csrc/mrca_nhorca_device.h drives the
C oracle's env through the four closed-loop gates of tests/test_nhorca_host.py for every point of
track_error {0.05, 0.1, 0.2} x track_time {0.3, 0.5, 1.0} x jitter {0, 0.1, 0.3} (other fields at ORCA's defaults; --horizons
adds time_horizon values).  A point is a candidate when it passes all four gates; the candidate with the fewest ticks summed
over the four-robot and the ten-robot gate wins.  CPU only.

    python tools/nhorca_defaults.py [--horizons 2 1] > profiles/nhorca/defaults.txt"""
import argparse
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rl-collision-avoidance_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import nhorca_ref as NR  # noqa: E402
import test_nhorca_host as H  # noqa: E402
import util as U  # noqa: E402
from util import S  # noqa: E402

f32 = np.float32


def gates(shim, p):
    """-> [(reached, crashed, ticks, passed)] of the four gates, and the static-line check of the block gate"""
    out = []
    sc = S.circle_n(2, 4.0, grid=S.empty_grid())
    poses = np.asarray(sc.init_table, f32).copy()
    poses[1, 1] += f32(0.2)
    env = H.closed_loop(shim, sc, p, 400, poses, np.asarray(sc.goal_table, f32))
    out.append((env, (env.first_result == 1).all() and not env.crashed.any()))
    sc = S.circle_n(1, 4.0, grid=U.small_grid(blocks=[(0.0, -0.5, 0.5, 0.5)]))
    worst = [0.0]

    def check(k, env, vel, lines, counts):
        ns = counts[0, 1]
        if ns:
            L, r = lines[0, 2:2 + ns].astype(np.float64), vel[0].astype(np.float64)
            worst[0] = max(worst[0], (L[:, 2] * (L[:, 1] - r[1]) - L[:, 3] * (L[:, 0] - r[0])).max())
    env = H.closed_loop(shim, sc, p, 400, np.array([[-3.0, 0.4, 0.0]], f32), np.array([[3.5, 0.4]], f32), check)
    out.append((env, not env.crashed.any() and env.first_result[0] != 2 and worst[0] <= 1e-5))
    for n, r, ticks in ((4, 3.0, 500), (10, 8.0, 800)):
        env = H.closed_loop(shim, S.circle_n(n, r, grid=S.empty_grid()), p, ticks)
        out.append((env, (env.first_result == 1).all() and not env.crashed.any()))
    return [(int((e.first_result == 1).sum()), int(e.crashed.sum()), e.ticks_run, bool(ok)) for e, ok in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizons", type=float, nargs="*", default=[2.0])
    args = ap.parse_args()
    shim = H.build_shim(pathlib.Path(tempfile.mkdtemp()))
    print("Defaults of mrca_nhorca_params: the sweep of tools/nhorca_defaults.py (host build of csrc/mrca_nhorca_device.h driving the C")
    print("oracle's env, fp32).  Per gate: (robots that reached, robots that crashed, ticks run); * = the gate FAILS.")
    print("  a: circle_n(2, 4.0), robot 1 started 0.2 m off the axis, 400 ticks: both reach, no crash")
    print("  b: one robot past a 1 m wide block, 400 ticks: no crash, the static lines hold at S2 (reaching is not asked)")
    print("  c: circle_n(4, 3.0), 500 ticks: all reach, no crash")
    print("  d: circle_n(10, 8.0), 800 ticks: all reach, no crash")
    print("Other fields at ORCA's defaults.  score = ticks of c + ticks of d, for points that pass all four.\n")
    print(f"{'horizon':>7} {'eps':>5} {'T':>4} {'jitter':>6}  {'a':<14}{'b':<14}{'c':<14}{'d':<14} score")
    best = None
    for th in args.horizons:
        for eps in (0.05, 0.1, 0.2):
            for T in (0.3, 0.5, 1.0):
                for jit in (0.0, 0.1, 0.3):
                    p = NR.params(time_horizon=th, track_error=eps, track_time=T, jitter=jit)
                    g = gates(shim, p)
                    ok = all(x[3] for x in g)
                    score = g[2][2] + g[3][2] if ok else None
                    cells = "".join(f"{'(%d,%d,%d)%s' % (x[0], x[1], x[2], '' if x[3] else '*'):<14}" for x in g)
                    print(f"{th:>7g} {eps:>5g} {T:>4g} {jit:>6g}  {cells} {score if ok else '-'}", flush=True)
                    if ok and (best is None or score < best[0]):
                        best = (score, th, eps, T, jit)
    if best is None:
        print("\nNo point passes all four gates.")
    else:
        print(f"\nChosen: time_horizon {best[1]:g}, track_error {best[2]:g}, track_time {best[3]:g}, jitter {best[4]:g} (score {best[0]}).")


if __name__ == "__main__":
    main()
