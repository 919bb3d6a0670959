#!/usr/bin/env python3
"""Time of the DWA baseline controller's kernel (mrca_dwa_actions) with the ORCA kernel's time on the SAME
state beside it: 82 circles x 50 robots = 4100 robots from perturbed starts, right after reset ("reset": the robots see
nobody within obst_dist) and at tick 200 of a DWA closed loop ("mid_run": they have met).  Per case 20 warm-up launches, then
200 launches each between its own pair of events, minus what an empty event pair reads (tools/orca_probe.py's `timed`).  Every
case runs in a child process of its own under a time limit, and every launch under an alarm: a launch that does not come back
ends its process, and nothing is started after it.

    python tools/dwa_probe.py [out.json]          (default: profiles/dwa/dwa_probe.json)
    python tools/dwa_probe.py --big [out.json]    (the same file: the cases are added to it)

--big: ONE world of 5 000 and of 50 000 robots (scenario.circle_big), after reset and at tick 100 of a DWA closed loop; ORCA
there is mrca_orca_actions_any.  DWA needs no neighbour search: its time per robot should not depend on the world's size.
"""
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from orca_probe import CASE_LIMIT_S, LAUNCHES, WARMUP, timed  # noqa: E402

STATES = {"reset": 0, "mid_run": 200}
BIG_SIZES, BIG_STATES = (5000, 50000), {"reset": 0, "mid_run": 100}


def child(robots, state):
    import torch
    from mrca import evaluate, scenario
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    if robots:
        env = VecStageWorld(scenario.circle_big(robots))
        env.reset()
        ticks = BIG_STATES[state]
    else:
        env = VecStageWorld(scenario.circle(num_worlds=82, seed=0))
        poses, goals = evaluate.perturbed_start(env, 0.2, 0.1, 0)
        env.reset(None, poses, goals)
        ticks = STATES[state]
    out = torch.zeros(env.N, 2, device=env.device)
    choice = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    for _ in range(ticks):
        env.step(env.dwa_actions(out=out))
    torch.cuda.synchronize()
    for _ in range(WARMUP):
        env.dwa_actions(out=out, choice=choice)
        env.orca_actions(out=out)
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    dwa = timed(lambda: env.dwa_actions(out=out), LAUNCHES, overhead)
    orca = timed(lambda: env.orca_actions(out=out), LAUNCHES, overhead)
    env.dwa_actions(out=out, choice=choice)
    env.check()
    print(json.dumps({
        "robots": env.N, "robots_per_world": env.R, "state": state, "tick": ticks, "launches": LAUNCHES, "event_pair_overhead_us": overhead,
        "dwa_kernel_us": dwa, "orca_kernel_us": orca, "orca_call": "mrca_orca_actions_any" if env.R > 64 else "mrca_orca_actions",
        "dwa_blocked": int((choice == -1).sum()), "dwa_at_goal": int((choice == -2).sum()),
        "live": int(env.live.sum()), "crashed": int(env.crashed.sum()), "reached": int((env.first_result == 1).sum())}))


def main(path, big):
    cases = [(n, s) for n in BIG_SIZES for s in BIG_STATES] if big else [(0, s) for s in STATES]
    results = []
    for robots, state in cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(robots), state], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"dwa_probe: case {robots} / {state} ended with status {r.returncode}; nothing more is started")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(results[-1])
    doc = {}
    if os.path.exists(path):
        with open(path) as fh:
            doc = json.load(fh)
    doc["big_cases" if big else "cases"] = results
    doc["params"] = "both controllers at their defaults (DWA: 5 x 21 candidates, 10 sub-steps, 64 obstacle points)"
    doc["method"] = (f"{LAUNCHES} launches after {WARMUP} warm-ups, one HIP event pair per launch minus an empty pair; both kernels "
                     "on the same env state in the same process")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 2 and args[0] == "--child":
        child(int(args[1]), args[2])
    else:
        big = "--big" in args
        rest = [a for a in args if a != "--big"]
        main(rest[0] if rest else os.path.join(ROOT, "profiles", "dwa", "dwa_probe.json"), big)
