#!/usr/bin/env python3
"""Times of the global planner (mrca_goal_fields, mrca_subgoals) on one MI355X.

Per tick: mrca_subgoals next to mrca_hybrid_actions and the env tick (mrca_step) in the SAME process on the same states, each
between its own pair of events behind a tick, minus what an empty event pair reads; 20 warm-ups, 200 samples.  Two cases on the
shipped Stage-2 map with the fields of its 44 table goals (library defaults: stride 2, inflate 7, lookahead 15):
  stage2_4092     93 Stage-2 worlds of 44 robots, 200 DWA-driven ticks into the run;
  stage2_49984    1136 such worlds.  (NOT one world of 50 000 robots, as the other probes have it: that world is a circle of 25 km
                  in open space, where no robot stands on a map; the subgoal call needs nothing of a robot's world, only N.)
Each case runs twice, with the library's eight lanes per robot and with MRCA_SUBGOAL_LANES=1 (one thread per robot: the same
outputs, compared here word for word), which is what decides between the two shapes.
Planning: mrca_goal_fields for the 44 table goals at strides 1 and 2, five calls each after one warm-up: wall time of the call
(it returns synchronised) and the launches that lowered something.
Line of sight (--los): mrca_subgoals_los at reach 15 / 60 / 256 beside mrca_subgoals, and the three controllers
steered at the subgoals (mrca_dwa_actions_goal, mrca_hybrid_actions_goal, mrca_hybrid_plan_goal) beside their siblings, in the SAME
process on the same two states; each case twice, with eight lanes per robot and with MRCA_SUBGOAL_LOS_LANES=64 (a wavefront per
robot: the same outputs, compared here word for word), which is what decides between the two shapes.
Every case runs in a child process of its own under a time limit, and every sample under an alarm: a launch that does not come
back ends its process, and nothing is started after it.

    python tools/planner_probe.py [out.json]          (default: profiles/planner/planner_probe.json)
    python tools/planner_probe.py --los [out.json]    (default: profiles/planner_los/planner_los_probe.json)
    python tools/planner_probe.py --goal [out.json]   (default: profiles/planner_los/goal_probe.json; the controllers and their _goal
                                                       forms alone, on a copy of the local goal and on subgoals, interleaved)
"""
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from orca_probe import CASE_LIMIT_S, LAUNCHES, WARMUP  # noqa: E402
from scan_noise_probe import timed_behind  # noqa: E402

MID_RUN_TICKS = 200
TICK_CASES = [("stage2_4092", 93), ("stage2_49984", 1136)]      # (name, Stage-2 worlds of 44 robots)


def table_goals(torch, sc, device):
    return torch.as_tensor(sc.goal_table, dtype=torch.float32, device=device).contiguous()


def child_tick(worlds):
    import torch
    from mrca import scenario
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    sc = scenario.stage2(num_worlds=worlds, seed=0)
    env = VecStageWorld(sc)
    env.reset()
    fields = env.plan_goals(table_goals(torch, sc, env.device))
    ticks_before = MID_RUN_TICKS
    act = torch.zeros(env.N, 2, device=env.device)
    cmd = torch.rand(env.N, 2, device=env.device)
    wrapped = torch.zeros(env.N, 2, device=env.device)
    out = env.subgoals(fields)

    def tick():
        env.step(env.dwa_actions(out=act))
    for _ in range(ticks_before + WARMUP):
        tick()
        env.subgoals(fields, out=out)
        env.hybrid_actions(cmd, out=wrapped)
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    res = {"subgoals_all_outputs": timed_behind(tick, lambda: env.subgoals(fields, out=out), LAUNCHES, overhead),
           "hybrid_actions": timed_behind(tick, lambda: env.hybrid_actions(cmd, out=wrapped), LAUNCHES, overhead),
           "env_tick": timed_behind(lambda: env.dwa_actions(out=act), lambda: env.step(act), LAUNCHES, overhead)}
    env.subgoals(fields, out=out)
    torch.cuda.synchronize()
    status = {str(c): int((out[3] == c).sum()) for c in (1, 0, -1, -2)}
    digest = [int(out[3].long().sum()), int(out[0].view(torch.int32).long().sum()), int(out[2].view(torch.int32).long().sum())]
    env.check()
    print(json.dumps({"robots": env.N, "robots_per_world": env.R, "lanes_per_robot": 1 if os.environ.get("MRCA_SUBGOAL_LANES") == "1" else 8,
                      "goals": fields.num_goals, "planner_params": fields.params.as_dict(), "plan_rounds": fields.rounds,
                      "samples": LAUNCHES, "ticks_before_the_samples": ticks_before + WARMUP, "event_pair_overhead_us": overhead,
                      "us": res, "status_at_the_end": status, "output_digest": digest}))


LOS_REACHES = (15, 60, 256)


def child_los(worlds):
    import torch
    from mrca import scenario
    from mrca.planner import LosParams
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    sc = scenario.stage2(num_worlds=worlds, seed=0)
    env = VecStageWorld(sc)
    env.reset()
    fields = env.plan_goals(table_goals(torch, sc, env.device))
    act = torch.zeros(env.N, 2, device=env.device)
    cmd = torch.rand(env.N, 2, device=env.device)
    wrapped = torch.zeros(env.N, 2, device=env.device)
    out = env.subgoals(fields)
    los = {r: LosParams(reach=r) for r in LOS_REACHES}
    outs = {r: env.subgoals_los(fields, los[r]) for r in LOS_REACHES}
    plan = env.hybrid_plan()

    def tick():
        env.step(env.dwa_actions(out=act))
    for _ in range(MID_RUN_TICKS + WARMUP):
        tick()
        env.subgoals(fields, out=out)
        for r in LOS_REACHES:
            env.subgoals_los(fields, los[r], out=outs[r])
    torch.cuda.synchronize()
    local = outs[60][0]
    overhead = env.event_pair_overhead(200)
    res = {"subgoals": timed_behind(tick, lambda: env.subgoals(fields, out=out), LAUNCHES, overhead)}
    for r in LOS_REACHES:
        res[f"subgoals_los_reach_{r}"] = timed_behind(tick, lambda: env.subgoals_los(fields, los[r], out=outs[r]), LAUNCHES, overhead)
    # the controllers on one frozen state (nothing moves between the samples): the sibling, then the same kernel with the goal given
    idle = lambda: None
    for name, fn in (("dwa_actions", lambda **kw: env.dwa_actions(out=act, **kw)),
                     ("hybrid_actions", lambda **kw: env.hybrid_actions(cmd, out=wrapped, **kw)),
                     ("hybrid_plan", lambda **kw: env.hybrid_plan(mode=plan[0], scale=plan[1], pid=plan[2], **kw))):
        for _ in range(WARMUP):
            fn()
            fn(goal=local)
        res[name] = timed_behind(idle, fn, LAUNCHES, overhead)
        res[name + "_goal"] = timed_behind(idle, lambda: fn(goal=local), LAUNCHES, overhead)
    for r in LOS_REACHES:
        env.subgoals_los(fields, los[r], out=outs[r])
    torch.cuda.synchronize()
    digest = {str(r): [int(t.view(torch.int32).long().sum()) for t in outs[r]] for r in LOS_REACHES}
    ahead = {str(r): [float(v) for v in outs[r][4].float().mean(dim=0)] for r in LOS_REACHES}
    env.check()
    print(json.dumps({"robots": env.N, "robots_per_world": env.R,
                      "lanes_per_robot": 64 if os.environ.get("MRCA_SUBGOAL_LOS_LANES") == "64" else 8,
                      "goals": fields.num_goals, "planner_params": fields.params.as_dict(), "samples": LAUNCHES,
                      "ticks_before_the_samples": MID_RUN_TICKS + WARMUP, "event_pair_overhead_us": overhead, "us": res,
                      "mean_ahead_m_and_m_vis": ahead, "output_digest": digest}))


def child_goal(worlds):
    """the three controllers and their _goal forms on one frozen state: the sibling, the _goal form on a COPY of
    MRCA_F_LOCAL_GOAL (the same kernel on the same values: expected equal) and on the line-of-sight subgoals (other values: a
    robot that stands at its own goal leaves the kernel early, one that is handed a subgoal elsewhere does not)"""
    import torch
    from mrca import scenario
    from mrca.planner import LosParams
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    sc = scenario.stage2(num_worlds=worlds, seed=0)
    env = VecStageWorld(sc)
    env.reset()
    fields = env.plan_goals(table_goals(torch, sc, env.device))
    act = torch.zeros(env.N, 2, device=env.device)
    cmd = torch.rand(env.N, 2, device=env.device)
    wrapped = torch.zeros(env.N, 2, device=env.device)
    plan = env.hybrid_plan()
    for _ in range(MID_RUN_TICKS + WARMUP):
        env.step(env.dwa_actions(out=act))
    local = env.subgoals_los(fields, LosParams(reach=60))[0]
    same = env.local_goal.clone()
    torch.cuda.synchronize()
    overhead = env.event_pair_overhead(200)
    res = {}
    idle = lambda: None
    for name, fn in (("dwa_actions", lambda **kw: env.dwa_actions(out=act, **kw)),
                     ("hybrid_actions", lambda **kw: env.hybrid_actions(cmd, out=wrapped, **kw)),
                     ("hybrid_plan", lambda **kw: env.hybrid_plan(mode=plan[0], scale=plan[1], pid=plan[2], **kw))):
        for _ in range(WARMUP):
            fn()
            fn(goal=same)
            fn(goal=local)
        # (interleaved rounds, so that a drift over the samples falls on all three alike)
        parts = {"": [], "_goal_on_a_copy_of_the_local_goal": [], "_goal_on_subgoals": []}
        for _round in range(4):
            for key, kw in (("", {}), ("_goal_on_a_copy_of_the_local_goal", {"goal": same}), ("_goal_on_subgoals", {"goal": local})):
                parts[key].append(timed_behind(idle, lambda: fn(**kw), LAUNCHES // 4, overhead)["median"])
        for key, meds in parts.items():
            res[name + key] = {"median_of_4_round_medians": statistics.median(meds), "round_medians": meds}
    env.check()
    print(json.dumps({"robots": env.N, "samples_per_round": LAUNCHES // 4, "ticks_before_the_samples": MID_RUN_TICKS + WARMUP,
                      "event_pair_overhead_us": overhead, "us": res}))


def main_goal(path):
    cases = []
    for name, worlds in TICK_CASES:
        cases.append({"case": name, **run(["--goal-case", str(worlds)])})
        print(cases[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"controllers": cases, "method": "four interleaved rounds of 50 samples per form on one frozen state, each call between "
                   "one HIP event pair, minus an empty pair; sibling and _goal form are one kernel"}, fh, indent=1)
        fh.write("\n")


def main_los(path):
    cases = []
    for name, worlds in TICK_CASES:
        pair = [run(["--los-case", str(worlds)], {"MRCA_SUBGOAL_LOS_LANES": lanes}) for lanes in ("8", "64")]
        same = pair[0]["output_digest"] == pair[1]["output_digest"]
        for r in pair:
            cases.append({"case": name, **r, "same_outputs_as_the_other_shape": same})
            print(cases[-1], flush=True)
    doc = {"per_tick": cases,
           "method": (f"{LAUNCHES} samples after {WARMUP} warm-ups, each call between one HIP event pair, minus an empty pair; the subgoal "
                      "calls behind a DWA-driven mrca_step enqueued in front of the pair, the controllers and their _goal forms on one "
                      "frozen state; lanes_per_robot 64 = MRCA_SUBGOAL_LOS_LANES=64")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def child_plan(stride):
    import torch
    from mrca import scenario
    from mrca.planner import PlannerParams
    from mrca.vec_env import VecStageWorld
    signal.alarm(CASE_LIMIT_S)
    sc = scenario.stage2(num_worlds=1, seed=0)
    env = VecStageWorld(sc)
    env.reset()
    goals = table_goals(torch, sc, env.device)
    p = PlannerParams(stride=stride)
    ms, rounds = [], []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = env.plan_goals(goals, p)
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
            rounds.append(f.rounds)
    print(json.dumps({"stride": stride, "goals": int(goals.shape[0]), "planning_grid": list(f.field.shape[1:]), "planner_params": p.as_dict(),
                      "calls": len(ms), "call_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)},
                      "rounds": sorted(set(rounds)), "field_bytes": f.field.numel() * 4,
                      "reachable_share": float((f.field != -1).float().mean())}))


def run(args, extra_env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=CASE_LIMIT_S + 120,
                       env=dict(os.environ, **(extra_env or {})))
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(f"planner_probe: {args} ended with status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(path):
    ticks, plans = [], []
    for name, worlds in TICK_CASES:
        pair = [run(["--tick", str(worlds)], {"MRCA_SUBGOAL_LANES": lanes}) for lanes in ("8", "1")]
        same = pair[0]["output_digest"] == pair[1]["output_digest"]
        for r in pair:
            ticks.append({"case": name, **r, "same_outputs_as_the_other_shape": same})
            print(ticks[-1], flush=True)
    for stride in (2, 1):
        plans.append(run(["--plan", str(stride)]))
        print(plans[-1], flush=True)
    doc = {"per_tick": ticks, "planning": plans,
           "method": (f"per tick: {LAUNCHES} samples after {WARMUP} warm-ups, each call between one HIP event pair behind a DWA-driven "
                      "mrca_step enqueued in front of the pair, minus an empty pair; lanes_per_robot 1 = MRCA_SUBGOAL_LANES=1; "
                      "planning: wall time of mrca_goal_fields (it returns synchronised), five calls after a warm-up")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 1 and args[0] == "--tick":
        child_tick(int(args[1]))
    elif len(args) > 1 and args[0] == "--plan":
        child_plan(int(args[1]))
    elif len(args) > 1 and args[0] == "--los-case":
        child_los(int(args[1]))
    elif len(args) > 1 and args[0] == "--goal-case":
        child_goal(int(args[1]))
    elif args and args[0] == "--goal":
        main_goal(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "planner_los", "goal_probe.json"))
    elif args and args[0] == "--los":
        main_los(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "planner_los", "planner_los_probe.json"))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "planner", "planner_probe.json"))
