#!/usr/bin/env python3
"""The renderer's two measurement cases, meant to run under ``rocprofv3 --kernel-trace --stats`` in a run of its
own (no counters in the same run); prints one JSON line per case with the bytes each launch moves by construction, so that the
trace's times turn into rates:

  views128   128 views of 256 x 256 over the 128-world x 32-robot Stage-1 env (map, goals, bodies, trail)
  bigworld   one 1024 x 1024 view of a 50 000-robot ``circle_big`` (fitted: every robot a fraction of a pixel)

    python tools/render_probe.py views128|bigworld [calls]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))

import torch  # noqa: E402

from mrca import scenario  # noqa: E402
from mrca.vec_env import VecStageWorld  # noqa: E402


def main(case, calls):
    if case == "views128":
        env = VecStageWorld(scenario.stage1(num_worlds=128, robots_per_world=32, seed=0)).reset()
        size = (256, 256)
    else:
        env = VecStageWorld(scenario.circle_big(50000)).reset()
        size = (1024, 1024)
    V = env.W
    trail = torch.zeros(V, size[1], size[0], dtype=torch.int32, device=env.device)
    out = env.render(None, size, trail=trail)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        env.render(None, size, trail=trail, out=out)
    torch.cuda.synchronize()
    wall_us = (time.perf_counter() - t0) / calls * 1e6
    px = V * size[0] * size[1]
    g = env.scenario.grid
    print(json.dumps({
        "case": case, "views": V, "size": list(size), "robots_per_view": env.R, "calls": calls, "wall_us_per_call": wall_us,
        # by construction: (a) stores every id once and reads the bit map; (b) reads 36 B of state per robot, its atomics land
        # on what its boxes cover; (c) loads ids + trail, stores 3 B per pixel
        "bytes_clear_map": {"written": 4 * px, "map_bits_read_at_most": V * g.height * g.words_per_row * 4},
        "bytes_splat": {"state_read": 36 * V * env.R, "body_pixels": int(((env.render_ids >> 24) >= 5).sum())},
        "bytes_resolve": {"read": 8 * px, "written": 3 * px},
    }))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20)
