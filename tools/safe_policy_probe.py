#!/usr/bin/env python3
"""Times of hybrid control in the paper's form in ONE process per case, on the same states: mrca_hybrid_plan
and mrca_hybrid_commit against mrca_hybrid_actions, and the scaled against the unscaled front end, fp32 and bf16
(mrca_lidar_features[_bf16] and mrca_lidar_features[_bf16]_scaled on the env's ring of raw scans, the shipped checkpoint's
weights, the scale the plan has just written).  82 circles x 50 robots = 4100 robots from perturbed starts, 200 DWA-driven ticks
into the run, and ONE world of 50 000 robots (scenario.circle_big).  As tools/hybrid_probe.py: per sample one DWA-driven
mrca_step OUTSIDE the event pairs, then the launches of a group, each between its own pair of events, minus what an empty
event pair reads; the members of a group take turns at going first and the medians are given per position as well.  20
warm-ups, 200 samples.  Every case runs in a child process of its own under a time limit, and every sample under an alarm: a
launch that does not come back ends its process, and nothing is started after it.

    python tools/safe_policy_probe.py [out.json]          (default: profiles/safe_policy/safe_policy_probe.json)
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

CASES = [("circles_4100", 0), ("one_world_50000", 50000)]      # (name, robots of ONE world or 0)
MID_RUN_TICKS = 200
CKPT = os.path.join(ROOT, "rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")


def summary(us):
    us = sorted(us)
    return {"median": statistics.median(us), "min": us[0], "p90": us[int(0.9 * len(us))], "max": us[-1]}


def child(robots):
    import torch
    from mrca import evaluate, policy_ops, scenario
    from mrca.net import CNNPolicy
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
    pol = CNNPolicy(3, 2).to(env.device)
    pol.load_state_dict(torch.load(CKPT, map_location=env.device))
    rc = pol._rollout_cache()
    w = (rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    out = torch.zeros(env.N, 2, device=env.device)
    cmd = torch.rand(env.N, 2, device=env.device)
    wrapped, committed = torch.zeros(env.N, 2, device=env.device), torch.zeros(env.N, 2, device=env.device)
    mode, hmode = (torch.zeros(env.N, dtype=torch.int32, device=env.device) for _ in range(2))
    scale, pid = torch.ones(env.N, device=env.device), torch.zeros(env.N, 2, device=env.device)
    clear = torch.zeros(env.N, 3, device=env.device)
    feat = {False: torch.empty(2, env.N, 4096, device=env.device),
            True: torch.empty(2, env.N, 4096, dtype=torch.bfloat16, device=env.device)}
    ring, head = env.policy_obs()

    def tick():
        env.step(env.dwa_actions(out=out))

    def front(bf16, scaled):
        fn = policy_ops.lidar_features_bf16 if bf16 else policy_ops.lidar_features
        return lambda: fn(ring, *w, out=feat[bf16], head=head, scale=scale if scaled else None)

    # groups whose members take turns at going first; the plan runs outside the pairs of the front ends' groups, so that the
    # scaled front end reads the scale of THIS state
    groups = {"control": {"hybrid_plan": lambda: env.hybrid_plan(mode=mode, scale=scale, pid=pid, clear=clear),
                          "hybrid_actions": lambda: env.hybrid_actions(cmd, out=wrapped, mode=hmode, clear=clear)},
              "front_end_fp32": {"unscaled": front(False, False), "scaled": front(False, True)},
              "front_end_bf16": {"unscaled": front(True, False), "scaled": front(True, True)}}
    commit = lambda: env.hybrid_commit(cmd, mode, pid, out=committed)  # noqa: E731
    for _ in range(ticks_before):
        tick()
    for _ in range(WARMUP):
        tick()
        for g in groups.values():
            for fn in g.values():
                fn()
        commit()
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b
    res = {}
    for gname, g in groups.items():
        names = list(g)
        us = {k: [] for k in names}
        by_position = {k: ([], []) for k in names}
        for i in range(LAUNCHES):
            signal.alarm(LAUNCH_LIMIT_S)             # (SIGALRM's default action ends the process)
            tick()
            if gname != "control":
                env.hybrid_plan(mode=mode, scale=scale, pid=pid)
            order = names if i % 2 == 0 else names[::-1]
            pairs = [(k, timed(g[k])) for k in order]
            pairs[-1][1][1].synchronize()
            for pos, (k, (a, b)) in enumerate(pairs):
                t = a.elapsed_time(b) * 1e3 - overhead
                us[k].append(t)
                by_position[k][pos].append(t)
        res[gname] = {}
        for k in names:
            res[gname][k] = summary(us[k])
            res[gname][k]["median_when_first"] = statistics.median(by_position[k][0])
            res[gname][k]["median_when_second"] = statistics.median(by_position[k][1])
    # the commit, behind a tick and a plan of its own
    us = []
    for _ in range(LAUNCHES):
        signal.alarm(LAUNCH_LIMIT_S)
        tick()
        env.hybrid_plan(mode=mode, scale=scale, pid=pid)
        a, b = timed(commit)
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 - overhead)
    signal.alarm(0)
    res["control"]["hybrid_commit"] = summary(us)
    mode_share = {str(m): float((mode == m).float().mean()) for m in (0, 1, 2, -2)}
    groups["control"]["hybrid_actions"]()
    assert torch.equal(mode, hmode)                      # the plan's mode is the wrapper's on the same state (the last tick's)
    env.check()
    print(json.dumps({
        "robots": env.N, "robots_per_world": env.R, "beams": env.B, "frames": env.F, "samples": LAUNCHES,
        "ticks_before_the_samples": ticks_before + WARMUP, "event_pair_overhead_us": overhead, "kernel_us": res,
        "plan_bytes_per_robot": {"read": 4 * env.B + 8 + 1, "written_at_most": 4 + 4 + 8 + 12},
        "commit_bytes_per_robot": {"read": 4 + 8 + 8, "written": 8},
        "mode_share_at_the_end": mode_share, "robots_scaled_at_the_end": float((scale < 1).float().mean()),
        "live": int(env.live.sum())}))


def main(path):
    results = []
    for name, robots in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(robots)], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S + 120)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"safe_policy_probe: case {name} ended with status {r.returncode}; nothing more is started")
        results.append({"case": name, **json.loads(r.stdout.strip().splitlines()[-1])})
        print(results[-1], flush=True)
    doc = {"cases": results, "context": CONTEXT,
           "method": (f"{LAUNCHES} samples after {WARMUP} warm-ups: one DWA-driven mrca_step outside the event pairs, then the launches "
                      "of a group (plan | hybrid_actions; unscaled | scaled front end, fp32 and bf16, the plan run in front of the "
                      "pairs), each between one HIP event pair minus an empty pair, taking turns at going first; the commit timed "
                      "behind a tick and a plan of its own; library defaults; the shipped checkpoint's weights")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 1 and args[0] == "--child":
        child(int(args[1]))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "safe_policy", "safe_policy_probe.json"))
