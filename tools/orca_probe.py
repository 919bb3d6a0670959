#!/usr/bin/env python3
"""Time of the ORCA baseline controller's kernel (mrca_orca_actions): 82 circles x 50 robots = 4100 robots,
at the default params and at max_neighbors = 48.  The env is taken mid-run -- tick 200 of an ORCA closed loop from perturbed
starts -- so that the constraints are real.  Per case 20 warm-up launches, then 200 launches each between its own pair of
events, minus what an empty event pair reads (mrca_event_pair_overhead).  Every case runs in a child process of its own under
a time limit, and every launch under an alarm: a launch that does not come back ends its process, and nothing is started
after it.

    python tools/orca_probe.py [out.json]          (default: profiles/orca/orca_probe.json)
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
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "orca", "orca_probe.json"))
