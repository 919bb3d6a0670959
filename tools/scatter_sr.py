#!/usr/bin/env python3
"""Behaviour on the paper's other scenarios (Long et al. 2018, Sec. V: random, group swap, group crossing, corridor), REPORTED,
not gated: 20 worlds whose starts and goals the scenario sampler draws (mrca_scatter; `mrca.evaluate --scenario S
--circles 20`, seed 0, 1200 ticks at most) of 20 robots -- 12 in the crossing, the most its boxes take -- driven by the shipped
checkpoint (--fused), the same under --hybrid, NH-ORCA, DWA and the stand-in: one run each, every run a child process under a
time limit; a run that fails ends the tool, and nothing is started after it.

    python tools/scatter_sr.py [out.json]          (default: profiles/scatter/scenarios_sr.json)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rl-collision-avoidance_amd")
CKPT = os.path.join("rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")
RUN_LIMIT_S = 300

SCENARIOS = {"random": 20, "swap": 20, "crossing": 12, "corridor": 20}
CONTROLLERS = {"policy": ["--policy", CKPT, "--fused"], "policy_hybrid": ["--policy", CKPT, "--fused", "--hybrid"], "nhorca": ["--nh-orca"],
               "dwa": ["--dwa"], "standin": []}
KEYS = ("success_rate", "crash_rate", "timeout_rate", "unfinished_rate", "extra_time_s", "scatter_max_tries_used")


def main(path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    runs = {}
    for sc, robots in SCENARIOS.items():
        for ctl, cflags in CONTROLLERS.items():
            cmd = [sys.executable, "-m", "mrca.evaluate", "--scenario", sc, "--circles", "20", "--robots", str(robots), "--max-ticks", "1200"] + cflags
            r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=RUN_LIMIT_S)
            name = f"{sc}_{ctl}"
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(f"scatter_sr: run {name} ended with status {r.returncode}; nothing more is started")
            out = runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, {k: out[k] for k in KEYS}, flush=True)
    doc = {"command": "python -m mrca.evaluate --scenario random | swap | crossing | corridor --circles 20 --robots 20 (crossing: 12) "
                      "--max-ticks 1200 + --policy policy_r03_fused_update_11min.pth --fused [--hybrid] | --nh-orca | --dwa | nothing "
                      "(the staggered-roundabout stand-in); seed 0 = draw 0, one MI355X (tools/scatter_sr.py)",
           "label": "one run each, stand-in weights: the checkpoint is the repository's own short training run, not the paper's policy",
           "runs": runs}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scatter", "scenarios_sr.json"))
