#!/usr/bin/env python3
"""Behaviour under lidar noise (mrca_scan_noise), REPORTED, not gated: the 20 perturbed circles of 50 and of 10
robots of DESIGN.md 5.12 / 5.13 (`mrca.evaluate --circles 20 --perturb 0.2,0.1 [--robots 10 --radius 8]`, seed 0, 1200 ticks at
most) driven by the checkpoint (--fused), by DWA and by ORCA, each without noise, at the library's default noise and at
const=0.05,prop=0.03,dropout=0.02 -- one run each, every run a child process under a time limit; a run that fails ends the
tool, and nothing is started after it.  The rows without noise are compared with the committed ones (profiles/orca/circle_sr.json,
profiles/dwa/circle_sr.json).

    python tools/scan_noise_sr.py [out.json]          (default: profiles/scan_noise/circle_sr.json)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rl-collision-avoidance_amd")
CKPT = os.path.join("rl-collision-avoidance_amd", "mrca", "data", "policy_r03_fused_update_11min.pth")
RUN_LIMIT_S = 300

CONTROLLERS = {"policy": ["--policy", CKPT, "--fused"], "dwa": ["--dwa"], "orca": ["--orca"]}
SIZES = {"50": [], "10": ["--robots", "10", "--radius", "8"]}
NOISE = {"none": None, "default": "default", "strong": "const=0.05,prop=0.03,dropout=0.02"}
COMMITTED = {"policy": ("orca", "policy"), "dwa": ("dwa", "dwa"), "orca": ("orca", "orca")}     # (profiles/<dir>/circle_sr.json, run prefix)


def main(path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    runs, same = {}, {}
    for ctl, cflags in CONTROLLERS.items():
        for size, sflags in SIZES.items():
            for level, spec in NOISE.items():
                cmd = [sys.executable, "-m", "mrca.evaluate", "--circles", "20", "--perturb", "0.2,0.1"] + sflags + cflags + \
                    ([] if spec is None else ["--lidar-noise", spec])
                r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=RUN_LIMIT_S)
                name = f"{ctl}_{size}_{level}"
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    sys.exit(f"scan_noise_sr: run {name} ended with status {r.returncode}; nothing more is started")
                out = runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
                print(name, {k: out[k] for k in ("success_rate", "crash_rate", "unfinished_rate", "extra_time_s", "lidar_noise")}, flush=True)
                if spec is None:
                    d, prefix = COMMITTED[ctl]
                    with open(os.path.join(ROOT, "profiles", d, "circle_sr.json")) as fh:
                        was = json.load(fh)["runs"][f"{prefix}_{size}"]
                    keys = ("success_rate", "crash_rate", "unfinished_rate", "mean_ticks_to_goal", "extra_distance_m")
                    same[name] = all(out[k] == was[k] for k in keys)
                    print(name, "reproduces the committed row:", same[name], flush=True)
    doc = {"command": "python -m mrca.evaluate --circles 20 --perturb 0.2,0.1 [--robots 10 --radius 8] + --policy "
                      "policy_r03_fused_update_11min.pth --fused | --dwa | --orca, + nothing | --lidar-noise default | --lidar-noise "
                      "const=0.05,prop=0.03,dropout=0.02; max 1200 ticks, one MI355X, one run each (tools/scan_noise_sr.py); the same "
                      "20 perturbed circles (seed 0) as profiles/orca/circle_sr.json and profiles/dwa/circle_sr.json",
           "no_noise_rows_reproduce_the_committed_ones": same, "runs": runs}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scan_noise", "circle_sr.json"))
