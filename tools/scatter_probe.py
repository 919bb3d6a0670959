#!/usr/bin/env python3
"""Time of the scenario sampler's kernel (mrca_scatter) with mrca_reset's time -- the call that takes its
outputs -- in the SAME process beside it: 1000 worlds x 50 robots and 128 worlds x 32 robots (scenario.random_box), ONE world of
4096 robots in the open world (the most the call takes: a box of 120 m x 120 m, 22 % covered), and the densest shipped
constructor (scenario.group_swap with 30 robots, 29.5 % of a box covered) in 128 worlds.  Per sample the one launch between its
own pair of events, minus what an empty event pair reads; mrca_reset(None, poses, goals) the same way.  Every case runs in a
child process of its own under a time limit, and every launch under an alarm: a launch that does not come back ends its
process, and nothing is started after it.

    python tools/scatter_probe.py [out.json]          (default: profiles/scatter/scatter_probe.json)
"""
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from orca_probe import CASE_LIMIT_S, timed  # noqa: E402

# name -> (warm-ups, samples)
CASES = {"random_box_1000x50": (5, 50), "random_box_128x32": (20, 200), "open_world_1x4096": (2, 10), "group_swap_128x30": (20, 200)}


def scenario_of(name):
    import numpy as np
    from mrca import scenario
    if name == "random_box_1000x50":
        return scenario.random_box(robots=50, num_worlds=1000)
    if name == "random_box_128x32":
        return scenario.random_box(robots=32, num_worlds=128)
    if name == "group_swap_128x30":
        return scenario.group_swap(robots=30, num_worlds=128)
    sc = scenario.circle_big(4096)
    sc.boxes = np.tile(np.asarray([-60.0, -60.0, 60.0, 60.0] * 2), (4096, 1))
    sc.scatter = dict(goal_min=5.0)
    return sc


def child(name):
    import torch
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    warmup, samples = CASES[name]
    env = VecStageWorld(scenario_of(name))
    out = env.scatter()
    for _ in range(warmup):
        env.scatter(out=out)
    torch.cuda.synchronize()
    tries = out[2].cpu()
    overhead = env.event_pair_overhead(200)
    kernel = timed(lambda: env.scatter(out=out), samples, overhead)
    env.reset(None, out[0], out[1])
    reset = timed(lambda: env.reset(None, out[0], out[1]), samples, overhead)
    env.step(torch.zeros((env.N, 2), device=env.device))
    torch.cuda.synchronize()
    env.check()
    print(json.dumps({
        "worlds": env.W, "robots_per_world": env.R, "robots": env.N, "block": 64 if env.R <= 64 else 256, "samples": samples,
        "event_pair_overhead_us": overhead, "scatter_kernel_us": kernel, "reset_us": reset,
        "tries_max": int(tries.max()), "tries_mean": float(tries.float().mean()), "robots_without_a_place": int((tries < 0).any(dim=1).sum()),
        "crashed_after_one_idle_tick": int(env.crashed.sum())}))


def main(path):
    results = []
    for name in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"scatter_probe: case {name} ended with status {r.returncode}; nothing more is started")
        results.append({"case": name, **json.loads(r.stdout.strip().splitlines()[-1])})
        print(results[-1])
    doc = {"cases": results,
           "method": ("per case a process of its own; after the warm-ups, each sample is the one mrca_scatter launch between one HIP "
                      "event pair minus an empty pair; mrca_reset(None, poses, goals) timed the same way in the same process")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 1 and args[0] == "--child":
        child(args[1])
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "scatter", "scatter_probe.json"))
