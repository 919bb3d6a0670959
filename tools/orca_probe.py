#!/usr/bin/env python3
"""Time of the ORCA baseline controller's kernel (mrca_orca_actions): 82 circles x 50 robots = 4100 robots,
at the default params and at max_neighbors = 48.  The env is taken mid-run -- tick 200 of an ORCA closed loop from perturbed
starts -- so that the constraints are real.  Per case 20 warm-up launches, then 200 launches each between its own pair of
events, minus what an empty event pair reads (mrca_event_pair_overhead).  Every case runs in a child process of its own under
a time limit, and every launch under an alarm: a launch that does not come back ends its process, and nothing is started
after it.

    python tools/orca_probe.py [out.json]          (default: profiles/orca/orca_probe.json)

The big-world case (mrca_orca_actions_any: ONE world of more than 64 robots, the neighbours found through the lidar hash):

    python tools/orca_probe.py --big [out.json]    (default: profiles/orca/orca_big_probe.json)

One world of 5 000 and of 50 000 robots in two states: "reset" -- scenario.circle_big right after reset(), 3.14 m between
neighbours, one chunk of candidates per robot -- and "jam" -- the robots teleported onto a square lattice 0.7 m apart with goals
across its centre, then 400 go-to-goal ticks: a crowd in which a robot's 3 x 3 cells hold hundreds of candidates.  Beside the
kernel's time: the env tick of the same world in the same process, timed the same way, and the candidates per robot (robots in
the 3 x 3 cells of 6.5 m, counted on the host from the poses) with the 64-entry chunks that makes.
"""
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))

CASES = {"defaults": {}, "max_neighbors_48": {"max_neighbors": 48}}
WARMUP, LAUNCHES, TICK = 20, 200, 200
LAUNCH_LIMIT_S, CASE_LIMIT_S = 20, 240
# for context (README / DESIGN.md 5.1, 5.10: the same 4096-robot scale)
CONTEXT = {"env_tick_us": 16.0, "fp32_rollout_tick_us": 248.0}


def child(case):
    import torch
    from mrca import evaluate, scenario
    from mrca.orca import OrcaParams
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(scenario.circle(num_worlds=82, seed=0))
    poses, goals = evaluate.perturbed_start(env, 0.2, 0.1, 0)
    env.reset(None, poses, goals)
    params = OrcaParams(**CASES[case])
    out = torch.zeros(env.N, 2, device=env.device)
    signal.alarm(CASE_LIMIT_S)
    for _ in range(TICK):
        env.step(env.orca_actions(params, out=out))
    torch.cuda.synchronize()
    for _ in range(WARMUP):
        env.orca_actions(params, out=out)
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    us = []
    for _ in range(LAUNCHES):
        signal.alarm(LAUNCH_LIMIT_S)                 # (SIGALRM's default action ends the process)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.orca_actions(params, out=out)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 - overhead)
    signal.alarm(0)
    env.check()
    us.sort()
    print(json.dumps({
        "case": case, "robots": env.N, "circles": env.W, "tick": TICK, "params": CASES[case], "launches": LAUNCHES,
        "event_pair_overhead_us": overhead, "kernel_us_median": statistics.median(us), "kernel_us_min": us[0],
        "kernel_us_p90": us[int(0.9 * len(us))], "kernel_us_max": us[-1],
        "live_robots_at_tick": int(env.live.sum()), "crashed_at_tick": int(env.crashed.sum()),
        "reached_at_tick": int((env.first_result == 1).sum())}))


BIG_SIZES, BIG_STATES, JAM_TICKS, JAM_PITCH = (5000, 50000), ("reset", "jam"), 400, 0.7


def timed(fn, launches, overhead):
    import torch
    us = []
    for _ in range(launches):
        signal.alarm(LAUNCH_LIMIT_S)                 # (SIGALRM's default action ends the process)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 - overhead)
    signal.alarm(0)
    us.sort()
    return {"median": statistics.median(us), "min": us[0], "p90": us[int(0.9 * len(us))], "max": us[-1]}


def child_big(robots, state):
    import numpy as np
    import torch
    from mrca import scenario
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    env = VecStageWorld(scenario.circle_big(robots))
    if state == "reset":
        env.reset()
    else:
        side = int(np.ceil(np.sqrt(robots)))
        k = np.arange(robots)
        xy = np.stack([(k % side - (side - 1) / 2.0) * JAM_PITCH, (k // side - (side - 1) / 2.0) * JAM_PITCH], 1)
        th = np.arctan2(-xy[:, 1], -xy[:, 0])
        poses = torch.from_numpy(np.concatenate([xy, th[:, None]], 1).astype(np.float32)).to(env.device)
        env.reset(None, poses, torch.from_numpy((-xy).astype(np.float32)).to(env.device))
        for _ in range(JAM_TICKS):
            lg = env.local_goal
            b = torch.atan2(lg[:, 1], lg[:, 0])
            env.step(torch.stack([(b.abs() < 1.0).float(), torch.clamp(2.0 * b, -1.0, 1.0)], 1).contiguous())
    torch.cuda.synchronize()
    out = torch.zeros(env.N, 2, device=env.device)
    for _ in range(WARMUP):
        env.orca_actions(out=out)
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    kernel = timed(lambda: env.orca_actions(out=out), LAUNCHES, overhead)
    # candidates per robot: the robots in the 3 x 3 cells around its own (neighbor_dist 6: one ring)
    xy = env.pose[:, :2].cpu().numpy()
    cell = np.floor(xy * np.float32(1.0 / 6.5)).astype(np.int64)
    cell -= cell.min(0)
    w = int(cell[:, 0].max()) + 3
    grid = np.zeros((int(cell[:, 1].max()) + 3, w), np.int64)
    np.add.at(grid, (cell[:, 1] + 1, cell[:, 0] + 1), 1)
    around = sum(np.roll(np.roll(grid, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    cand = around[cell[:, 1] + 1, cell[:, 0] + 1]
    chunks = (cand + 63) // 64
    status = {"live": int(env.live.sum()), "crashed": int(env.crashed.sum()), "reached": int((env.first_result == 1).sum())}
    zeros = torch.zeros(env.N, 2, device=env.device)    # the tick last: it moves nobody, but it is timed on the same state
    for _ in range(WARMUP):
        env.step(zeros)
    torch.cuda.synchronize()
    tick = timed(lambda: env.step(zeros), LAUNCHES, overhead)
    env.check()
    print(json.dumps({
        "robots": env.N, "state": state, "launches": LAUNCHES, "event_pair_overhead_us": overhead,
        "orca_kernel_us": kernel, "env_tick_us": tick, **status,
        "candidates_per_robot": {"mean": float(cand.mean()), "median": float(np.median(cand)), "max": int(cand.max())},
        "chunks_per_robot": {"mean": float(chunks.mean()), "max": int(chunks.max())}}))


def main_big(path):
    results = []
    for robots in BIG_SIZES:
        for state in BIG_STATES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-big", str(robots), state], capture_output=True,
                               text=True, timeout=CASE_LIMIT_S + 120)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(f"orca_probe: big case {robots} / {state} ended with status {r.returncode}; nothing more is started")
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(results[-1])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"cases": results, "params": "defaults (neighbor_dist 6, max_neighbors 10)",
                   "method": f"{LAUNCHES} launches after {WARMUP} warm-ups, one HIP event pair per launch (the tick: per step call, "
                             "its launches together) minus an empty pair; jam = a 0.7 m lattice after "
                             f"{JAM_TICKS} go-to-goal ticks"}, fh, indent=1)
        fh.write("\n")


def main(path):
    results = []
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"orca_probe: case {case} ended with status {r.returncode}; nothing more is started")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(results[-1])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"cases": results, "context_us": CONTEXT,
                   "method": f"{LAUNCHES} launches after {WARMUP} warm-ups, one HIP event pair per launch minus an empty pair"}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--child-big":
        child_big(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) > 1 and sys.argv[1] == "--big":
        main_big(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "orca", "orca_big_probe.json"))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "orca", "orca_probe.json"))
