#!/usr/bin/env python3
"""Time of the hybrid control kernel (mrca_hybrid_actions) with the lidar noise kernel's (mrca_scan_noise) and
the env tick's (mrca_step) in the SAME process on the same states: 82 circles x 50 robots = 4100 robots from perturbed starts,
200 DWA-driven ticks into the run, and ONE world of 50 000 robots (scenario.circle_big).  Both kernels are timed where they run
in use -- right behind a tick, on the row that tick's ray cast has just stored: per sample one mrca_step driven by the DWA
controller OUTSIDE the event pairs, then the hybrid launch and the noise launch, each between its own pair of events, minus
what an empty event pair reads.  The two take turns at going first (the second finds the row where the first left it in the
caches; the hybrid call writes nothing of the env, so the order changes no state the other sees but the noise itself), and the
medians are given per position as well.  20 warm-ups, 200 samples.  The tick is timed the same way, its actions made outside
the pair.  Every case runs in a child process of its own under a time limit, and every sample under an alarm: a launch that
does not come back ends its process, and nothing is started after it.

    python tools/hybrid_probe.py [out.json]          (default: profiles/hybrid/hybrid_probe.json)
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
from scan_noise_probe import timed_behind  # noqa: E402

CASES = [("circles_4100", 0), ("one_world_50000", 50000)]      # (name, robots of ONE world or 0)
MID_RUN_TICKS = 200


def summary(us):
    us = sorted(us)
    return {"median": statistics.median(us), "min": us[0], "p90": us[int(0.9 * len(us))], "max": us[-1]}


def child(robots):
    import torch
    from mrca import evaluate, scenario
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    if robots:
        env = VecStageWorld(scenario.circle_big(robots))
        env.reset()
        ticks_before = 0
    else:
        env = VecStageWorld(scenario.circle(num_worlds=82, seed=0))
        poses, goals = evaluate.perturbed_start(env, 0.2, 0.1, 0)
        env.reset(None, poses, goals)
        ticks_before = MID_RUN_TICKS
    out = torch.zeros(env.N, 2, device=env.device)
    cmd = torch.rand(env.N, 2, device=env.device)
    wrapped = torch.zeros(env.N, 2, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    clear = torch.zeros(env.N, 3, device=env.device)

    def tick():
        env.step(env.dwa_actions(out=out))

    launches = {"hybrid_all_outputs": lambda: env.hybrid_actions(cmd, out=wrapped, mode=mode, clear=clear),
                "hybrid_command_only": lambda: env.hybrid_actions(cmd, out=wrapped),
                "scan_noise": lambda: env.scan_noise()}
    for _ in range(ticks_before):
        tick()
    for _ in range(WARMUP):
        tick()
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b
    us = {k: [] for k in launches}
    by_position = {k: ([], []) for k in launches}
    for i in range(LAUNCHES):
        signal.alarm(LAUNCH_LIMIT_S)                 # (SIGALRM's default action ends the process)
        tick()
        order = ["hybrid_all_outputs", "scan_noise"] if i % 2 == 0 else ["scan_noise", "hybrid_all_outputs"]
        pairs = [(k, timed(launches[k])) for k in order]
        pairs[-1][1][1].synchronize()
        for pos, (k, (a, b)) in enumerate(pairs):
            t = a.elapsed_time(b) * 1e3 - overhead
            us[k].append(t)
            by_position[k][pos].append(t)
    signal.alarm(0)
    mode_share = {str(m): float((mode == m).float().mean()) for m in (0, 1, 2, -2)}
    res = {k: summary(us[k]) for k in ("hybrid_all_outputs", "scan_noise")}
    for k in res:
        res[k]["median_when_first"] = statistics.median(by_position[k][0])
        res[k]["median_when_second"] = statistics.median(by_position[k][1])
    res["hybrid_command_only"] = timed_behind(tick, launches["hybrid_command_only"], LAUNCHES, overhead)
    step = timed_behind(lambda: env.dwa_actions(out=out), lambda: env.step(out), LAUNCHES, overhead)
    returning = float((env.scan_ring[torch.arange(env.N, device=env.device), env.ring_head.long()] < 6.0).float().mean())
    env.check()
    print(json.dumps({
        "robots": env.N, "robots_per_world": env.R, "beams": env.B, "frames": env.F, "samples": LAUNCHES,
        "ticks_before_the_samples": ticks_before + WARMUP, "event_pair_overhead_us": overhead, "kernel_us": res, "env_tick_us": step,
        "hybrid_bytes_per_robot": {"read": 4 * env.B + 8 + 8 + 1, "written_at_most": 24},
        "scan_noise_bytes_per_robot": 2 * 4 * env.B + 2 * 8 * (env.B // 64),
        "mode_share_at_the_end": mode_share, "beams_returning_at_the_end": returning, "live": int(env.live.sum())}))


def main(path):
    results = []
    for name, robots in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(robots)], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"hybrid_probe: case {name} ended with status {r.returncode}; nothing more is started")
        results.append({"case": name, **json.loads(r.stdout.strip().splitlines()[-1])})
        print(results[-1], flush=True)
    doc = {"cases": results, "context": CONTEXT,
           "method": (f"{LAUNCHES} samples after {WARMUP} warm-ups: one DWA-driven mrca_step outside the event pairs, then the hybrid "
                      "launch and the noise launch (library defaults both), each between one HIP event pair minus an empty pair, "
                      "taking turns at going first; hybrid_command_only and mrca_step timed behind a tick of their own in the same "
                      "process")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 1 and args[0] == "--child":
        child(int(args[1]))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "hybrid", "hybrid_probe.json"))
