#!/usr/bin/env python3
"""Behaviour with the global planner (mrca_goal_fields, mrca_subgoals), REPORTED, not gated: the doorway scenario
(`mrca.evaluate --scenario doorway --circles 20`: 20 rooms of 12 robots, 1200 ticks at most) driven by the shipped checkpoint
(--fused) and by the go-to-goal stand-in, each without and with --planner -- one run each, every run a child process under a time
limit; a run that fails ends the tool, and nothing is started after it.

    python tools/planner_sr.py [out.json] [NAME=VALUE ...]       (default: profiles/planner/doorway_sr.json)
    python tools/planner_sr.py --los [out.json] [NAME=VALUE ...] (default: profiles/planner_los/doorway_sr.json)

--los: plain subgoals against line-of-sight ones (--planner-los) for the checkpoint, and --planner-los under DWA
and under hybrid control around the checkpoint, which take no plain --planner; beside them DWA and hybrid on their own local goal.

NAME=VALUE: fields of mrca_planner_params for the --planner runs (default: PlannerParams.for_grid of the map)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rl-collision-avoidance_amd")
CKPT = os.path.join("rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")

CONTROLLERS = {"policy": ["--policy", CKPT, "--fused"], "stand_in": []}
SCENARIO = ["--scenario", "doorway", "--circles", "20"]
SHOWN = ("success_rate", "crash_rate", "timeout_rate", "unfinished_rate", "extra_time_s", "extra_distance_m", "planner_status_last_tick",
         "planner_mean_initial_path_m")
LIMIT_S = 300


LOS_RUNS = {"policy_planner": CONTROLLERS["policy"] + ["--planner"], "policy_planner_los": CONTROLLERS["policy"] + ["--planner-los"],
            "dwa_own_local_goal": ["--dwa"], "dwa_planner_los": ["--dwa", "--planner-los"],
            "hybrid_own_local_goal": CONTROLLERS["policy"] + ["--hybrid"],
            "hybrid_planner_los": CONTROLLERS["policy"] + ["--hybrid", "--planner-los"],
            "hybrid_safe_planner_los": CONTROLLERS["policy"] + ["--hybrid-safe", "--planner-los"]}


def main_los(path, assignments):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    runs = {}
    for name, flags in LOS_RUNS.items():
        pflags = [x for a in assignments for x in ("--planner-param", a)] if "planner" in name else []
        r = subprocess.run([sys.executable, "-m", "mrca.evaluate"] + SCENARIO + flags + pflags, env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"planner_sr: run {name} ended with status {r.returncode}; nothing more is started")
        out = runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, {k: out.get(k) for k in SHOWN + ("los_params", "planner_mean_ahead", "mean_ticks_to_goal")}, flush=True)
    doc = {"command": "python -m mrca.evaluate --scenario doorway --circles 20 + the flags of each run (LOS_RUNS, tools/planner_sr.py; the "
                      "checkpoint is policy_r03_fused_update_11min.pth --fused); seed 0, one MI355X, one run each",
           "flags": LOS_RUNS, "planner_param_assignments": assignments, "runs": runs}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main(path, assignments):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    planner_flags = ["--planner"] + [x for a in assignments for x in ("--planner-param", a)]
    runs = {}
    for ctl, cflags in CONTROLLERS.items():
        for wrap, pflags in (("plain", []), ("planner", planner_flags)):
            cmd = [sys.executable, "-m", "mrca.evaluate"] + SCENARIO + cflags + pflags
            r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=LIMIT_S)
            name = f"{ctl}_{wrap}"
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(f"planner_sr: run {name} ended with status {r.returncode}; nothing more is started")
            out = runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, {k: out.get(k) for k in SHOWN}, flush=True)
    doc = {"command": "python -m mrca.evaluate --scenario doorway --circles 20 + the controller (--policy policy_r03_fused_update_11min.pth "
                      "--fused | nothing: go_to_goal_policy) + nothing | --planner [--planner-param ...]; seed 0, one MI355X, one run "
                      "each (tools/planner_sr.py)",
           "planner_param_assignments": assignments, "runs": runs}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    rest = sys.argv[1:]
    if rest and rest[0] == "--los":
        rest.pop(0)
        out = rest.pop(0) if rest and "=" not in rest[0] else os.path.join(ROOT, "profiles", "planner_los", "doorway_sr.json")
        main_los(out, rest)
        sys.exit(0)
    out = rest.pop(0) if rest and "=" not in rest[0] else os.path.join(ROOT, "profiles", "planner", "doorway_sr.json")
    main(out, rest)
