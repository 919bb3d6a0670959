#!/usr/bin/env python3
"""Behaviour under hybrid control (mrca_hybrid_actions; in the paper's form: mrca_hybrid_plan / mrca_hybrid_commit,
DESIGN.md 5.16), REPORTED, not gated: the 20 perturbed circles of 50 and
of 10 robots of DESIGN.md 5.12 (`mrca.evaluate --circles 20 --perturb 0.2,0.1 [--robots 10 --radius 8]`, seed 0, 1200 ticks at
most) and the one circle of 5000 robots at 0.9 m spacing (`--one-circle 5000 --spacing 0.9 --max-ticks 20000`), each driven by
the shipped checkpoint (--fused) and by the stand-in, each with and without --hybrid, the checkpoint also with --hybrid-safe (the
stand-in reads no rescaled scan) -- one run each, every run a child process under a time limit; a run that fails ends the tool,
and nothing is started after it.  The rows without hybrid control are compared with the committed ones
(profiles/orca/circle_sr.json, profiles/orca/one_circle_sr.json).

    python tools/hybrid_sr.py circles [out.json] [--only=policy] [NAME=VALUE ...]       (default: profiles/safe_policy/circle_sr.json)
    python tools/hybrid_sr.py one-circle [out.json] [--only=policy] [NAME=VALUE ...]    (default: profiles/safe_policy/one_circle_sr.json)

NAME=VALUE: fields of mrca_hybrid_params for the --hybrid and --hybrid-safe runs, of mrca_safe_policy_params (scan_scale, v_cap)
for the --hybrid-safe runs (default: the library's).  --only=policy | --only=stand_in: that controller's rows alone.
(profiles/hybrid/ holds the rows as they were before --hybrid-safe existed.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rl-collision-avoidance_amd")
CKPT = os.path.join("rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")

CONTROLLERS = {"policy": ["--policy", CKPT, "--fused"], "stand_in": []}
SETS = {
    "circles": {
        "scenarios": {"50": ["--circles", "20", "--perturb", "0.2,0.1"],
                      "10": ["--circles", "20", "--perturb", "0.2,0.1", "--robots", "10", "--radius", "8"]},
        "committed": ("circle_sr.json", {"policy": "policy_{}", "stand_in": "staggered_{}"}), "out": "circle_sr.json", "limit_s": 300},
    "one-circle": {
        "scenarios": {"5000": ["--one-circle", "5000", "--spacing", "0.9", "--max-ticks", "20000"]},
        "committed": ("one_circle_sr.json", {"policy": "checkpoint", "stand_in": "stand_in"}), "out": "one_circle_sr.json", "limit_s": 1000},
}
KEYS = ("success_rate", "crash_rate", "unfinished_rate", "mean_ticks_to_goal", "extra_distance_m")
SHOWN = ("success_rate", "crash_rate", "unfinished_rate", "extra_time_s", "extra_distance_m", "hybrid_modes")
SAFE_FIELDS = ("scan_scale", "v_cap")


def main(which, path, assignments, only=None):
    cfg = SETS[which]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    with open(os.path.join(ROOT, "profiles", "orca", cfg["committed"][0])) as fh:
        committed = json.load(fh)["runs"]
    rule = [x for a in assignments if a.partition("=")[0] not in SAFE_FIELDS for x in ("--hybrid-param", a)]
    hybrid_flags = ["--hybrid"] + rule
    safe_flags = ["--hybrid-safe"] + rule + [x for a in assignments if a.partition("=")[0] in SAFE_FIELDS for x in ("--hybrid-safe-param", a)]
    runs, same = {}, {}
    for ctl, cflags in CONTROLLERS.items():
        if only not in (None, ctl):
            continue
        wraps = [("plain", []), ("hybrid", hybrid_flags)] + ([("hybrid_safe", safe_flags)] if ctl == "policy" else [])
        for size, sflags in cfg["scenarios"].items():
            for wrap, hflags in wraps:
                cmd = [sys.executable, "-m", "mrca.evaluate"] + sflags + cflags + hflags
                r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=cfg["limit_s"])
                name = f"{ctl}_{size}_{wrap}"
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    sys.exit(f"hybrid_sr: run {name} ended with status {r.returncode}; nothing more is started")
                out = runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
                print(name, {k: out.get(k) for k in SHOWN}, flush=True)
                if wrap == "plain":
                    was = committed[cfg["committed"][1][ctl].format(size)]
                    same[name] = all(out[k] == was[k] for k in KEYS)
                    print(name, "reproduces the committed row:", same[name], flush=True)
    doc = {"command": "python -m mrca.evaluate + the scenario (--circles 20 --perturb 0.2,0.1 [--robots 10 --radius 8], max 1200 ticks | "
                      "--one-circle 5000 --spacing 0.9 --max-ticks 20000) + the controller (--policy policy_r03_fused_update_11min.pth "
                      "--fused | nothing: staggered_roundabout_policy) + nothing | --hybrid [--hybrid-param ...] | --hybrid-safe "
                      "[--hybrid-param ... --hybrid-safe-param ...] (the checkpoint only); seed 0, one MI355X, "
                      "one run each (tools/hybrid_sr.py); the scenarios of profiles/orca/circle_sr.json and one_circle_sr.json",
           "hybrid_param_assignments": assignments, "only": only,
           "plain_rows_reproduce_the_committed_ones": same, "runs": runs}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if not args or args[0] not in SETS:
        sys.exit(__doc__)
    rest = args[1:]
    out = rest.pop(0) if rest and "=" not in rest[0] else os.path.join(ROOT, "profiles", "safe_policy", SETS[args[0]]["out"])
    only = [a.partition("=")[2] for a in rest if a.startswith("--only=")]
    if any(o not in CONTROLLERS for o in only):
        sys.exit(__doc__)
    main(args[0], out, [a for a in rest if not a.startswith("--only=")], only[0] if only else None)
