#!/usr/bin/env python3
"""Time of the lidar noise model's kernel (mrca_scan_noise) with the env tick's time (mrca_step) in the SAME
process beside it: 82 circles x 50 robots = 4100 robots from perturbed starts with both lazy_obs values, and ONE world of
50 000 robots (scenario.circle_big).  The kernel is timed where it runs in use -- right behind a tick, on the row that tick's
ray cast has just stored (a second call on the same row would see what the first one left: dropped beams pile up): per
sample one mrca_step driven by the DWA controller OUTSIDE the event pair, then the noise launch between its own pair of
events, minus what an empty event pair reads.  20 warm-ups, 200 samples.  The tick is timed the same way, its actions made
outside the pair.  Every case runs in a child process of its own under a time limit, and every launch under an alarm: a launch
that does not come back ends its process, and nothing is started after it.

    python tools/scan_noise_probe.py [out.json]          (default: profiles/scan_noise/scan_noise_probe.json)
"""
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from orca_probe import CASE_LIMIT_S, CONTEXT, LAUNCH_LIMIT_S, LAUNCHES, WARMUP  # noqa: E402

CASES = [("circles_4100", 0, 1), ("circles_4100", 0, 0), ("one_world_50000", 50000, 1)]      # (name, robots of ONE world or 0, lazy_obs)
PARAM_SETS = {"defaults": None, "strong": dict(sigma_const=0.05, sigma_prop=0.03, dropout=0.02, quantum=0.0),
              "quantised": dict(sigma_const=0.02, sigma_prop=0.01, dropout=0.005, quantum=0.01)}


def timed_behind(prep, fn, samples, overhead):
    """fn between its own pair of events, `prep` enqueued in front of the pair"""
    import torch
    us = []
    for _ in range(samples):
        signal.alarm(LAUNCH_LIMIT_S)                 # (SIGALRM's default action ends the process)
        prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 - overhead)
    signal.alarm(0)
    us.sort()
    return {"median": statistics.median(us), "min": us[0], "p90": us[int(0.9 * len(us))], "max": us[-1]}


def child(robots, lazy):
    import torch
    from mrca import evaluate, scenario
    from mrca.noise import ScanNoiseParams
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    if robots:
        env = VecStageWorld(scenario.circle_big(robots), lazy_obs=bool(lazy))
        env.reset()
    else:
        env = VecStageWorld(scenario.circle(num_worlds=82, seed=0), lazy_obs=bool(lazy))
        poses, goals = evaluate.perturbed_start(env, 0.2, 0.1, 0)
        env.reset(None, poses, goals)
    out = torch.zeros(env.N, 2, device=env.device)

    def tick():
        env.step(env.dwa_actions(out=out))

    sets = {k: ScanNoiseParams() if v is None else ScanNoiseParams(**v) for k, v in PARAM_SETS.items()}
    for _ in range(WARMUP):
        tick()
        env.scan_noise(sets["defaults"])
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    res = {name: timed_behind(tick, lambda p=p: env.scan_noise(p), LAUNCHES, overhead) for name, p in sets.items()}
    step = timed_behind(lambda: env.dwa_actions(out=out), lambda: env.step(out), LAUNCHES, overhead)
    returning = float((env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()] < 6.0).float().mean())
    env.check()
    print(json.dumps({
        "robots": env.N, "robots_per_world": env.R, "beams": env.B, "frames": env.F, "lazy_obs": int(lazy), "samples": LAUNCHES,
        "event_pair_overhead_us": overhead, "scan_noise_kernel_us": res, "env_tick_us": step,
        "ring_row_bytes_per_robot": 2 * 4 * env.B + 2 * 8 * (env.B // 64) + (0 if lazy else 2 * 4 * env.B),
        "beams_returning_at_the_end": returning, "live": int(env.live.sum())}))


def main(path):
    results = []
    for name, robots, lazy in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(robots), str(lazy)], capture_output=True,
                           text=True, timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"scan_noise_probe: case {name} / lazy_obs {lazy} ended with status {r.returncode}; nothing more is started")
        results.append({"case": name, **json.loads(r.stdout.strip().splitlines()[-1])})
        print(results[-1])
    doc = {"cases": results, "context": CONTEXT,
           "params": {k: (v or "mrca_scan_noise_default_params") for k, v in PARAM_SETS.items()},
           "method": (f"{LAUNCHES} samples after {WARMUP} warm-ups: one DWA-driven mrca_step outside the event pair, then the noise "
                      "launch between one HIP event pair minus an empty pair; mrca_step timed the same way in the same process")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 2 and args[0] == "--child":
        child(int(args[1]), int(args[2]))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "scan_noise", "scan_noise_probe.json"))
