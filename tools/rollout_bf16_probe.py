#!/usr/bin/env python3
"""GPU measurement: the rollout tick (policy + sampling + env tick, the body make_bench_step(env, "rollout", ...,
graph=True) captures) of Stage-1 at 128 x 32 = 4096 robots with the fp32 fused policy path and with the opt-in bf16 fused
path (csrc/mrca_policy_bf16.hip + a bf16 fc1), alternating in one process: warm-up, then rounds of device-synchronised
replays of each.  Prints one JSON object: us per tick and agent-steps/s of each path, the algorithmic bytes and FLOPs of
the bf16 front end and of fc1, and -- given ``--stats`` (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace
--stats`` run of this tool) -- the kernel time of mrca_lidar_features_bf16 and its share of the HBM roof.

    python tools/rollout_bf16_probe.py [--worlds 128 --robots-per-world 32 --ticks 200 --rounds 5] [--stats CSV] [--out JSON]
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rl-collision-avoidance_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak


def kernel_stats(path, needle):
    """-> (calls, average ns) of the kernels whose name contains ``needle`` in a rocprofv3 kernel_stats.csv"""
    calls, total = 0, 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            if needle in row.get("Name", ""):
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return calls, (total / calls if calls else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=128)
    ap.add_argument("--robots-per-world", type=int, default=32)
    ap.add_argument("--ticks", type=int, default=200, help="ticks per timed round and path")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as g
    g.build()
    from mrca import scenario as S
    from mrca.trainer import make_bench_step
    from mrca.vec_env import VecStageWorld

    steps, envs = {}, {}
    for name, bf16 in (("fp32", False), ("bf16", True)):
        sc = S.stage1(num_worlds=a.worlds, robots_per_world=a.robots_per_world, seed=0)
        env = VecStageWorld(sc)
        env.reset()
        envs[name] = env
        steps[name] = make_bench_step(env, "rollout", None, fused=True, graph=True, fused_bf16=bf16)
    N = envs["fp32"].N
    for name in steps:
        steps[name].run_ticks(a.warmup)
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name in steps:                   # alternating: both paths see the same clocks and thermal state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps[name].run_ticks(a.ticks)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.ticks)

    out = {"robots": N, "ticks_per_round": a.ticks, "rounds": a.rounds}
    for name in steps:
        best = min(times[name])
        med = sorted(times[name])[len(times[name]) // 2]
        out[name] = {"us_per_tick_median": med * 1e6, "us_per_tick_best": best * 1e6,
                     "agent_steps_per_s_median": N / med, "us_per_tick_rounds": [t * 1e6 for t in times[name]]}
    out["speedup_median"] = out["fp32"]["us_per_tick_median"] / out["bf16"]["us_per_tick_median"]
    # algorithmic counts (both towers)
    fe_bytes = N * (3 * 512 * 4 + 2 * 4096 * 2)
    fe_flops = 2 * N * 2 * (32 * 255 * 15 + 32 * 128 * 96)
    fc1_bytes = 2 * N * 4096 * 2 + 2 * 4096 * 256 * 2 + 2 * N * 256 * 4
    fc1_flops = 2 * 2 * N * 4096 * 256
    out["front_end_bf16"] = {"bytes": fe_bytes, "flops": fe_flops, "hbm_floor_us": fe_bytes / HBM_BYTES_PER_S * 1e6}
    out["fc1_bf16"] = {"bytes": fc1_bytes, "flops": fc1_flops, "hbm_floor_us": fc1_bytes / HBM_BYTES_PER_S * 1e6}
    if a.stats:
        calls, ns = kernel_stats(a.stats, "lidar_features_bf16_kernel")
        out["front_end_bf16"]["rocprof_calls"] = calls
        if ns:
            out["front_end_bf16"]["rocprof_avg_us"] = ns / 1e3
            out["front_end_bf16"]["hbm_roof_share"] = (fe_bytes / HBM_BYTES_PER_S * 1e9) / ns
        calls32, ns32 = kernel_stats(a.stats, "lidar_features_kernel")
        if ns32:
            out["front_end_fp32_rocprof_avg_us"] = ns32 / 1e3
    for env in envs.values():
        env.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
