#!/usr/bin/env python3
"""Time of the NH-ORCA baseline controller's kernel (mrca_nhorca_actions) beside plain ORCA's
(mrca_orca_actions) on the same states in the same process.  The states are tools/orca_probe.py's: 82 circles x 50 robots = 4100
robots at tick 200 of an ORCA closed loop from perturbed starts.  Per call 20 warm-up launches, then 200 launches each between
its own pair of events, minus what an empty event pair reads.  The case runs in a child process under a time limit, and every
launch under an alarm: a launch that does not come back ends its process, and nothing is started after it.

    python tools/nhorca_probe.py [out.json]          (default: profiles/nhorca/nhorca_probe.json)
    python tools/nhorca_probe.py --big [out.json]    (default: profiles/nhorca/nhorca_big_probe.json)

--big: ONE world of 5 000 and of 50 000 robots (the neighbours come from the lidar hash), in orca_probe.py's two states, "reset"
and "jam"."""
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import orca_probe as P  # noqa: E402  (the states, the timing loop and the limits)


def both(env):
    """the two calls timed on the env as it stands -> {"orca_kernel_us", "nhorca_kernel_us", "ratio_of_medians", "nhorca_modes"}"""
    import torch
    from mrca.nhorca import MODES
    out = torch.zeros(env.N, 2, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    calls = {"orca": lambda: env.orca_actions(out=out), "nhorca": lambda: env.nhorca_actions(out=out, mode=mode)}
    overhead = env.event_pair_overhead(200)
    res = {"event_pair_overhead_us": overhead}
    for name, fn in calls.items():
        for _ in range(P.WARMUP):
            fn()
        torch.cuda.synchronize()
        res[name + "_kernel_us"] = P.timed(fn, P.LAUNCHES, overhead)
    res["ratio_of_medians"] = res["nhorca_kernel_us"]["median"] / res["orca_kernel_us"]["median"]
    counts = torch.bincount(mode[env.first_result == 0], minlength=len(MODES)).tolist()
    res["nhorca_modes_of_live_robots"] = dict(zip(MODES, counts))
    env.check()
    return res


def child():
    import torch
    from mrca import evaluate, scenario
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(scenario.circle(num_worlds=82, seed=0))
    poses, goals = evaluate.perturbed_start(env, 0.2, 0.1, 0)
    env.reset(None, poses, goals)
    out = torch.zeros(env.N, 2, device=env.device)
    signal.alarm(P.CASE_LIMIT_S)
    for _ in range(P.TICK):
        env.step(env.orca_actions(out=out))
    torch.cuda.synchronize()
    print(json.dumps({"robots": env.N, "circles": env.W, "tick": P.TICK, "launches": P.LAUNCHES, **both(env),
                      "live_robots_at_tick": int(env.live.sum())}))


def child_big(robots, state):
    import numpy as np
    import torch
    from mrca import scenario
    from mrca.vec_env import VecStageWorld
    signal.alarm(P.CASE_LIMIT_S)
    env = VecStageWorld(scenario.circle_big(robots))
    if state == "reset":
        env.reset()
    else:
        side = int(np.ceil(np.sqrt(robots)))
        k = np.arange(robots)
        xy = np.stack([(k % side - (side - 1) / 2.0) * P.JAM_PITCH, (k // side - (side - 1) / 2.0) * P.JAM_PITCH], 1)
        th = np.arctan2(-xy[:, 1], -xy[:, 0])
        poses = torch.from_numpy(np.concatenate([xy, th[:, None]], 1).astype(np.float32)).to(env.device)
        env.reset(None, poses, torch.from_numpy((-xy).astype(np.float32)).to(env.device))
        for _ in range(P.JAM_TICKS):
            lg = env.local_goal
            b = torch.atan2(lg[:, 1], lg[:, 0])
            env.step(torch.stack([(b.abs() < 1.0).float(), torch.clamp(2.0 * b, -1.0, 1.0)], 1).contiguous())
    torch.cuda.synchronize()
    print(json.dumps({"robots": env.N, "state": state, "launches": P.LAUNCHES, **both(env), "live": int(env.live.sum())}))


def run(children, path, note):
    results = []
    for args in children:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=P.CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"nhorca_probe: {args} ended with status {r.returncode}; nothing more is started")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(results[-1])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"cases": results, "params": "each controller's defaults",
                   "method": f"{P.LAUNCHES} launches after {P.WARMUP} warm-ups, one HIP event pair per launch minus an empty pair; "
                             "ORCA first, then NH-ORCA, on the same state in the same process; " + note}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    elif len(sys.argv) > 3 and sys.argv[1] == "--child-big":
        child_big(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) > 1 and sys.argv[1] == "--big":
        run([["--child-big", str(n), s] for n in P.BIG_SIZES for s in P.BIG_STATES],
            sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "nhorca", "nhorca_big_probe.json"),
            f"jam = a {P.JAM_PITCH} m lattice after {P.JAM_TICKS} go-to-goal ticks")
    else:
        run([["--child"]], sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nhorca", "nhorca_probe.json"),
            f"4100 robots at tick {P.TICK} of an ORCA closed loop from perturbed starts")
