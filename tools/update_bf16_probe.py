#!/usr/bin/env python3
"""GPU measurement: one PPO minibatch -- forward + loss + backward + Adam through ``ppo.ppo_update_stage1`` with the trainer's
FlatGrads / FlatAdam -- with the fused fp32 update and with the opt-in fused bf16 update (``CNNPolicy.fused_train_bf16``:
csrc/mrca_policy_bf16_rows.hip, csrc/mrca_policy_bf16_bwd.hip and bf16 fc1 GEMMs), alternating in one process on the same
one-frame-per-tick buffer (synthetic by default; ``--real``: a Stage-1 rollout of 128 x 32 robots).  bf16 is an opt-in
precision, not the reference's.  Prints one JSON object:

  * ms per minibatch of each path (median and best of the rounds) and their ratio;
  * the front-end kernels alone, from HIP events around their own launches: fp32 and bf16 forward (row-table form) and
    backward, with the bytes each moves and its share of the HBM roof;
  * given ``--stats`` (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace --stats`` run of this tool): the
    per-kernel table of that run;
  * with ``--real``: the first minibatch's k3 KL(old || new) of a bf16 update after an fp32 rollout and after a bf16 rollout
    (the distance between the policy that acted and the policy the update re-evaluates, before any step).

    python tools/update_bf16_probe.py [--minibatch 16384 --rounds 7 --steps 6] [--real] [--stats CSV] [--out JSON]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rl-collision-avoidance_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak


def synthetic_memory(torch, ppo, T, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    frames = (torch.rand(T + 2, N, 512, generator=g) - 0.5).cuda()
    fidx = torch.stack([torch.arange(t, t + 3).expand(N, 3) for t in range(T)]).contiguous().cuda()      # [T, N, 3]
    goals, speeds = (torch.randn(T, N, 2, generator=g).cuda() for _ in range(2))
    actions = torch.rand(T, N, 2, generator=g).cuda()
    logprobs = (torch.randn(T, N, 1, generator=g) * 0.1 - 2.0).cuda()
    targets, advs = (torch.randn(T, N, 1, generator=g).cuda() for _ in range(2))
    return (ppo.FrameRows(frames, fidx), goals, speeds, actions, logprobs, targets, None, None, advs)


def real_rollout(torch, worlds, robots, horizon, rollout_bf16, seed=0):
    """-> (env, trainer, memory) after ``horizon`` ticks of a fresh Stage-1 trainer whose own update is held back"""
    from mrca import ppo
    from mrca import scenario as S
    from mrca.trainer import HParams, Stage1Trainer
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(S.stage1(num_worlds=worlds, robots_per_world=robots, seed=seed))
    hp = HParams(horizon=horizon + 1, batch_size=16384, rollout_fused=True, rollout_bf16=rollout_bf16, update_fused=True)
    tr = Stage1Trainer(env, hp=hp, seed=seed)
    tr.start()
    for _ in range(horizon):
        tr.tick()
    buf = tr.buffer
    with torch.no_grad():
        obs, head = ppo.policy_input(env, True)
        _m, last_v = tr.policy.mean_value_fused(obs, env.local_goal, env.speed, head=head, bf16=rollout_bf16)
    sl = slice(0, horizon)
    targets, advs = ppo.generate_train_data(buf.reward[sl], hp.gamma, buf.value[sl], last_v, buf.done[sl], hp.lam)
    rows = buf.obs_rows()
    rows = ppo.FrameRows(rows.frames, rows.fidx[sl].contiguous())
    memory = (rows, buf.goal[sl], buf.speed[sl], buf.action[sl], buf.logprob[sl], targets, buf.value[sl], buf.reward[sl], advs)
    return env, tr, memory


def first_minibatch_kl(torch, policy, memory, n):
    """k3 estimate of KL(old || new) over the first ``n`` rows before any step, formed in float64 (the loss kernel's fp32
    (r - 1) - log r cannot resolve a ratio within 1e-4 of 1)"""
    from mrca.net import gaussian_logprob
    obss, goals, speeds, actions, logprobs = memory[:5]
    idx = torch.arange(n, device="cuda")
    obss.lazy = True
    with torch.no_grad():
        mean, _value = policy.mean_value(obss[idx], goals.reshape(-1, 2)[:n], speeds.reshape(-1, 2)[:n])
        new_lp = gaussian_logprob(actions.reshape(-1, 2)[:n].double(), mean.double(), policy.logstd.double().expand_as(mean))
        log_ratio = new_lp - logprobs.reshape(-1, 1)[:n].double()
        return float(((torch.exp(log_ratio) - 1.0) - log_ratio).mean())


def event_time(torch, fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=6, help="minibatches per timed round and path")
    ap.add_argument("--real", action="store_true", help="a real Stage-1 rollout (128 x 32 robots) instead of the synthetic buffer")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()

    import time

    import torch

    import __graft_entry__ as g
    g.build()
    from mrca import policy_ops, ppo
    from mrca.net import CNNPolicy

    mb = a.minibatch
    out = {"minibatch": mb, "steps_per_round": a.steps, "rounds": a.rounds, "buffer": "real" if a.real else "synthetic",
           "note": "bf16 is an opt-in precision, not the reference's; fp32 is the default"}
    envs = []
    if a.real:
        N, T = 128 * 32, mb // (128 * 32)
        kl = {}
        for rollout_bf16 in (False, True):
            env, tr, memory = real_rollout(torch, 128, 32, T, rollout_bf16)
            envs.append(env)
            tr.policy.fused_train = tr.policy.fused_train_bf16 = True
            kl["bf16_rollout" if rollout_bf16 else "fp32_rollout"] = first_minibatch_kl(torch, tr.policy, memory, mb)
            tr.policy.fused_train_bf16 = False
            if not rollout_bf16:
                kl["fp32_rollout_fp32_update"] = first_minibatch_kl(torch, tr.policy, memory, mb)
        out["first_minibatch_kl_of_a_bf16_update_after"] = kl
    else:
        T, N = 8, mb // 8
        memory = synthetic_memory(torch, ppo, T, N)

    torch.manual_seed(0)
    base = CNNPolicy(3, 2).cuda()
    paths = {}
    for name, bf16 in (("fp32", False), ("bf16", True)):
        p = CNNPolicy(3, 2).cuda()
        p.load_state_dict(base.state_dict())
        p.fused_train, p.fused_train_bf16 = True, bf16
        fg = ppo.FlatGrads(p.parameters())
        opt = ppo.FlatAdam(fg, lr=5e-5)
        paths[name] = (p, fg, opt)
    batches = lambda n: [torch.arange(mb, device="cuda")] * a.steps      # noqa: E731

    def run(name):
        p, fg, opt = paths[name]
        ppo.ppo_update_stage1(p, opt, mb, memory, epoch=1, num_step=T, num_env=N, frames=3, obs_size=512, act_size=2,
                              index_batches=batches, flat_grads=fg)

    for name in paths:
        run(name)
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for name in paths:                   # alternating: both paths see the same clocks and thermal state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps)
    for name in paths:
        ts = sorted(times[name])
        out[name] = {"ms_per_minibatch_median": ts[len(ts) // 2] * 1e3, "ms_per_minibatch_best": ts[0] * 1e3,
                     "ms_per_minibatch_rounds": [t * 1e3 for t in times[name]]}
    out["speedup_median"] = out["fp32"]["ms_per_minibatch_median"] / out["bf16"]["ms_per_minibatch_median"]

    # the front-end kernels alone (HIP events around their own launches), row-table form
    memory[0].lazy = True
    table = memory[0][torch.arange(mb, device="cuda")]
    rc = base.refresh_rollout_cache()
    w = (rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    f32 = policy_ops.lidar_features(table, *w)
    g32 = torch.randn(2, mb, 4096, device="cuda") / mb
    f16 = policy_ops.lidar_features_bf16_rows(table, *w)
    g16 = g32.to(torch.bfloat16)
    scan = mb * 3 * 512 * 4
    kern = {
        "forward_fp32": (event_time(torch, lambda: policy_ops.lidar_features(table, *w, out=f32)), scan + 2 * mb * 4096 * 4),
        "forward_bf16_rows": (event_time(torch, lambda: policy_ops.lidar_features_bf16_rows(table, *w, out=f16)),
                              scan + 2 * mb * 4096 * 2),
        "backward_fp32": (event_time(torch, lambda: policy_ops.lidar_features_backward(table, *w[:3], f32, g32[0], g32[1])),
                          2 * scan + 2 * 2 * mb * 4096 * 4),
        "backward_bf16": (event_time(torch, lambda: policy_ops.lidar_features_bf16_backward(table, *w[:3], f16, g16[0], g16[1])),
                          2 * scan + 2 * 2 * mb * 4096 * 2),
    }
    out["front_end_kernels"] = {k: {"us": us, "bytes": b, "hbm_floor_us": b / HBM_BYTES_PER_S * 1e6,
                                    "hbm_roof_share": b / HBM_BYTES_PER_S * 1e6 / us} for k, (us, b) in kern.items()}
    if a.stats:
        rows = []
        with open(a.stats) as f:
            for row in csv.DictReader(f):
                rows.append({"name": row.get("Name", "")[:100], "calls": int(row["Calls"]),
                             "total_ms": float(row["TotalDurationNs"]) / 1e6,
                             "avg_us": float(row["TotalDurationNs"]) / max(int(row["Calls"]), 1) / 1e3})
        rows.sort(key=lambda r: -r["total_ms"])
        out["rocprof_kernels"] = rows[:24]
    for env in envs:
        env.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
