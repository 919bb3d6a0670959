"""GPU: the PPO update in the form ``Stage1Trainer.update()`` runs it, through the HIP kernels -- the front end read through row
tables out of the one-frame store (mrca_lidar_features_rows / _backward_rows), the row kernels with the detached biases,
``ppo_loss``, ``FlatGrads`` + ``FlatAdam`` (mrca_adam_step) -- against a float64 model of the reference's update that runs on
the host (tests/update_ref.py; tests/test_update_ref_host.py grounds it in the reference's own run and runs the CPU twins of
every leg here).

(a) the production path (``index_batches=None``) against a replay of the permutations it drew, bit for bit; (b) against the
model, with the stock layers' distance to the model measured beside it as the yardstick; (c) the update the trainer itself
assembles on a Stage-2 env.  No captured graph anywhere.

D, L and G are update_ref.distance / loss_distance / gradient_distance: the largest per-tensor ||d_got - d_model|| / ||d_model||
of the parameters' change over the update; the largest |logged loss - model| / max(1, |model|); the largest per-tensor
||g_got - g_model|| / ||g_model|| of the first step's gradient.  Bars: L <= 2e-5 (the project's bar on a logged loss on the
device), D_fused <= 8 x D_stock and G_fused <= 8 x G_stock -- twice the 4.3 the docstring of tests/test_gpu_policy_bwd.py::
test_policy_gradients_with_the_hip_front_end_equal_the_stock_gradients records between the fused backward's and MIOpen's
distance to float64 on its worst tensor.

What D is, and is not, on the trainer's own data (c).  Over the 16 steps of that update D does not measure rounding.  On the
MI355X the SAME stock update of the same snapshot gave D = 7.2e-3 in one run and 8.5e-4 in others (in one process, and from
one process to the next); PyTorch's CPU kernels give 7.2e-3 with 8 threads and 8.5e-4 with 2 or 16; the fused path 7.4e-3 --
while every path's first-step gradient is within 2e-6 of the model's, its parameters after the first step within 1.4e-4 and
every logged loss within 3e-7.  The larger figure appears in ONE step (the 9th of 16 in the fused path and on the CPU, the
12th in a stock run): one output channel of the freshly initialised actor's second conv layer parts from the model (3.4e-5 of
the layer's 1.1e-2 change behind that step, the other 31 channels together 4e-6), and from there the whole actor follows
another trajectory.  No sample changes sides of the clip range anywhere (largest drift of a ratio 3e-5, nearest edge 1e-4
away); the paths' ReLUs differ from the model's in single positions whose input is within 3e-8 of zero; Adam divides a
gradient by its own running size, so a unit whose gradient is that small still moves by the learning rate.  Whether a path
has the event is decided at the level of its summation order, so the end of such a trajectory has no yardstick: the
stock path's own D is either figure.  (c) therefore asserts D where it does measure rounding -- behind the FIRST step, D1,
with the stock leg's D1 as the yardstick -- next to G and to L over all 16 steps, and prints the whole update's D of both
legs.  The bar this leg was first written with, D_fused <= 8 x D_stock over the whole update, was met at 7.4e-3 against
7.2e-3 in one run of this file and missed at 7.4e-3 against 8.5e-4 in the next; profiles/update_path/ has the probes.  On the synthetic memories of (b) the policy hardly moves (6 steps on inputs of size 1): D sits at the rounding of
the fp32 parameters themselves, 5e-5 .. 2e-4, in both paths, and is asserted over the whole update as the issue states it."""
import numpy as np
import pytest
import torch

import rollout_ref as R
import update_ref as M
import util as U  # noqa: F401

pytestmark = pytest.mark.gpu

L_BAR = 2e-5
RATIO = 8.0


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def _learner(fused, seed=11):
    """A fresh policy on the device -> (policy, optimizer, flat_grads): the fused path with FlatGrads + FlatAdam (built last: it
    re-seats the parameters), or the stock layers with torch.optim.Adam."""
    from mrca import net, ppo
    torch.manual_seed(seed)
    policy = net.CNNPolicy(frames=3, action_space=2).cuda()
    if not fused:
        return policy, torch.optim.Adam(policy.parameters(), lr=M.HP["lr"]), None
    policy.fused_train = True
    fg = ppo.FlatGrads(policy.parameters())
    return policy, ppo.FlatAdam(fg, lr=M.HP["lr"]), fg


def _drop_list(T, N, what):
    from mrca import ppo
    d = M.done_flags(T, N, np.random.default_rng(3), single_carry=3 if what == "carry" else None)
    drop = ppo.get_filter_index(torch.from_numpy(d).cuda())
    assert len(drop) > 0 and sorted(drop.tolist()) == sorted(R.filter_index(d))
    return drop


def _frame_rows(frames, fidx):
    from mrca import ppo
    return ppo.FrameRows(torch.from_numpy(frames).cuda(), torch.from_numpy(fidx).cuda())


def _front_end_calls(monkeypatch):
    """Count what the fused front end is handed from here on: ``{"table": calls with a policy_ops.FrameTable (the row-table
    kernels), "tensor": calls with gathered stacks}``.  (The rows a Stage-2 update keeps are a FrameRows of their own, so the
    ``lazy`` flag of the one a caller built does not tell.)"""
    from mrca import policy_ops
    calls, real = {"table": 0, "tensor": 0}, policy_ops.lidar_features_fn

    def fn(x, *a, **kw):
        calls["table" if isinstance(x, policy_ops.FrameTable) else "tensor"] += 1
        return real(x, *a, **kw)
    monkeypatch.setattr(policy_ops, "lidar_features_fn", fn)
    return calls


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("T,N,batch,what,stage2", [
    (6, 64, 128, None, False),          # 384 = 3 x 128
    (5, 13, 32, None, False),           # 65 = 2 x 32 + 1: a last minibatch of ONE row
    (4, 5, 64, None, False),            # 20 < 64: one short minibatch
    (6, 64, 128, "runs", True),         # two whole minibatches, the short one dropped
    (5, 13, 32, "carry", True),         # one row dropped: 64 = 2 x 32 left
    (4, 5, 64, "runs", True),           # fewer rows left than a minibatch: no step, nothing touched, no error
])
def test_fused_production_path_equals_the_replay_of_its_permutations(hip, monkeypatch, T, N, batch, what, stage2):
    """The fused update over a one-frame store with restarted robots, ``index_batches=None``, against the same update handed back
    the permutations it drew: parameters and loss log equal to the bit (the GEMM operands are fresh tensors of equal shape and
    values in both runs, the kernels' summation orders are fixed)."""
    from mrca import ppo
    pol, opt, fg = _learner(True)
    before = M.state_of(pol)
    mem, frames, fidx = M.synthetic_memory(before, T, N, seed=T * N)
    drop = _drop_list(T, N, what) if stage2 else None
    left = T * N - (0 if drop is None else len(drop))
    steps = 2 * (left // batch if stage2 else -(-left // batch))
    rows = _frame_rows(frames, fidx)
    calls = _front_end_calls(monkeypatch)
    log, perms = M.run_update(ppo, pol, opt, fg, M.torch_memory(mem, "cuda", rows), T, N, batch, stage2, drop)
    torch.cuda.synchronize()
    assert calls == {"table": steps, "tensor": 0}, "the fused update did not read the frame store through row tables"
    assert stage2 or rows.lazy
    assert len(perms) == 2 and all(sorted(p.tolist()) == list(range(left)) for p in perms) and len(log) == steps
    if steps == 0:
        assert all(np.array_equal(before[k], v) for k, v in M.state_of(pol).items())
        assert opt.steps == 0 and not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())
        return
    if what == "carry":
        assert left == 2 * batch
    if not stage2 and left % batch:
        assert M.cut(perms[0], batch, False)[-1].size == left % batch
    pol2, opt2, fg2 = _learner(True)
    rows2 = _frame_rows(frames, fidx)
    log2, perms2 = M.run_update(ppo, pol2, opt2, fg2, M.torch_memory(mem, "cuda", rows2), T, N, batch, stage2, drop,
                                index_batches=M.replay_batches(perms, batch, stage2, "cuda"))
    torch.cuda.synchronize()
    assert perms2 == [] and calls == {"table": 2 * steps, "tensor": 0}
    assert len(log2) == steps and all(torch.equal(torch.stack(a), torch.stack(b)) for a, b in zip(log, log2))
    moved = 0
    for (k, a), b in zip(pol.state_dict().items(), pol2.state_dict().values()):
        assert torch.equal(a, b), k
        moved += int((a.double().cpu().numpy() != before[k]).sum())
    assert moved > 0


# ---------------------------------------------------------------------------------------------- (b)
def _report(title, before, want, per_f, per_s, g_f, g_s):
    """Per tensor: the two distances of the parameters' change to the model's, and of the first step's gradient to the model's."""
    print(title)
    print(f"  {'tensor':22s} {'D fused':>9s} {'D stock':>9s}   {'g1 fused':>9s} {'g1 stock':>9s}    (g1: the first step's gradient, relative L2 "
          "distance to the model's)")
    sizes = {k: before[k].size for k in M.ORDER}
    (G_f, gper_f), (G_s, gper_s) = (M.gradient_distance(sizes, g, want.grads[0]) for g in (g_f, g_s))
    for k in M.ORDER:
        print(f"  {k:22s} {per_f[k]:9.1e} {per_s[k]:9.1e}   {gper_f[k]:9.1e} {gper_s[k]:9.1e}")
    return G_f, G_s


@pytest.mark.parametrize("stage2", [False, True], ids=["stage1", "stage2"])
@pytest.mark.parametrize("T,N,batch", [(6, 64, 128), (5, 13, 32)])
def test_fused_production_path_against_the_model_and_the_stock_layers_yardstick(hip, monkeypatch, T, N, batch, stage2):
    """The fused production update (row tables, row kernels, ppo_loss, FlatGrads + FlatAdam, its own permutations) and the stock
    layers (MIOpen, torch.optim.Adam, replaying those permutations over materialised stacks: the path the reference-run goldens
    pin) on the same memory, each against the float64 model.  Measured on the MI355X (profiles/update_path/):

                            D_fused  D_stock   L_fused  L_stock   G_fused  G_stock
        stage1 6x64/128     6.3e-5   7.0e-5    6.0e-8   5.4e-8    5.0e-7   6.5e-7      (D_stock 1.0e-4 in another run)
        stage2 6x64/128     1.8e-4   1.8e-4    3.5e-8   8.7e-8    4.6e-7   2.1e-6
        stage1 5x13/32      7.6e-5   7.7e-5    5.2e-8   8.2e-8    4.2e-7   4.4e-7
        stage2 5x13/32      8.3e-5   8.3e-5    4.7e-8   8.3e-8    5.3e-7   3.9e-7
    """
    from mrca import ppo
    pol, opt, fg = _learner(True)
    before = M.state_of(pol)
    mem, frames, fidx = M.synthetic_memory(before, T, N, seed=T * N)
    inside, below, above = M.ratio_classes(before, mem, M.HP["clip"])
    assert inside > 0 and below > 0 and above > 0, (inside, below, above)
    drop = _drop_list(T, N, "runs") if stage2 else None
    rows = _frame_rows(frames, fidx)
    g_f = M.first_step(opt, pol)
    calls = _front_end_calls(monkeypatch)
    log, perms = M.run_update(ppo, pol, opt, fg, M.torch_memory(mem, "cuda", rows), T, N, batch, stage2, drop)
    assert calls == {"table": len(log), "tensor": 0}
    pol_s, opt_s, _none = _learner(False)
    g_s = M.first_step(opt_s, pol_s)
    log_s, _p = M.run_update(ppo, pol_s, opt_s, None, M.torch_memory(mem, "cuda"), T, N, batch, stage2, drop,
                             index_batches=M.replay_batches(perms, batch, stage2, "cuda"))
    torch.cuda.synchronize()
    want = M.update(before, mem, None if drop is None else drop.cpu().numpy(), [M.cut(p, batch, stage2) for p in perms],
                    every_state=False, **M.HP)
    assert len(log) == len(log_s) == len(want.losses) > 0 and calls["table"] == len(log)
    D_f, per_f = M.distance(before, M.state_of(pol), want.states[-1])
    D_s, per_s = M.distance(before, M.state_of(pol_s), want.states[-1])
    L_f, L_s = M.loss_distance(log, want.losses), M.loss_distance(log_s, want.losses)
    G_f, G_s = _report(f"stage{1 + stage2} {T}x{N}/{batch}: {len(log)} steps, ratios inside / below / above the clip range {inside} / {below} / "
            f"{above}", before, want, per_f, per_s, g_f["grad"], g_s["grad"])
    print(f"  D_fused = {D_f:.1e} ({max(per_f, key=per_f.get)})  D_stock = {D_s:.1e} ({max(per_s, key=per_s.get)})  "
          f"L_fused = {L_f:.1e}  L_stock = {L_s:.1e}  G_fused = {G_f:.1e}  G_stock = {G_s:.1e}")
    assert L_f <= L_BAR, (L_f, L_s)
    assert D_f <= RATIO * D_s, (D_f, D_s)
    assert G_f <= RATIO * G_s, (G_f, G_s)


# ---------------------------------------------------------------------------------------------- (c)
def _same_snapshot(a, b):
    return (all(np.array_equal(a["mem"][k], b["mem"][k]) for k in a["mem"]) and np.array_equal(a["drop"], b["drop"]) and
            all(np.array_equal(a["state"][k], b["state"][k]) for k in a["state"]) and
            len(a["perms"]) == len(b["perms"]) and all(np.array_equal(p, q) for p, q in zip(a["perms"], b["perms"])))


def test_trainer_update_on_a_stage2_env_against_the_model(hip, monkeypatch):
    """``Stage1Trainer(stage2=True)`` on a VecStageWorld: 16 eager ticks into the env-bound one-frame buffer, the 16th running the
    trainer's own update -- through the stock layers (``update_fused=False``: the yardstick) and through the fused path.  The
    model is replayed from what the trainer handed ``ppo_update_stage2``: the memory tuple, the filter index (equal to the
    reference's walk over the stored flags, and not empty), the state dict, the permutations drawn.  Asserted: L over all 16
    steps, G, and D behind the first step (D1) against the stock leg's; the whole update's D is printed -- see the head of this
    file for why it has no yardstick.  Measured on the MI355X (62 of 4224 rows dropped, 16 steps; profiles/update_path/):

                               L        G        D1       D (whole update)
        update_fused=False     9.8e-8   7.3e-7   1.4e-4   8.5e-4, and 7.2e-3 in another run of the same file
        update_fused=True      2.3e-7   4.4e-7   9.7e-5   7.4e-3
    """
    from mrca import ppo
    from mrca.trainer import HParams, Stage1Trainer
    sc, _lead = R.scenario("stage2", 16)
    seen = M.snapshot_updates(monkeypatch, ppo)
    calls = _front_end_calls(monkeypatch)
    got, want = {}, None
    for fused in (False, True):
        env = hip.VecStageWorld(sc)
        hp = HParams(horizon=16, batch_size=512, epoch=2, rollout_fused=True, update_fused=fused)
        tr = Stage1Trainer(env, hp=hp, seed=3, stage2=True)
        assert tr.buffer.env_bound and isinstance(tr.optimizer, ppo.FlatAdam) and tr.policy.fused_train == fused
        first = M.first_step(tr.optimizer, tr.policy)
        tr.start()
        for _ in range(16):
            tr.tick()
        torch.cuda.synchronize()
        assert tr.global_update == 1 and len(seen) == 1 + fused
        snap = seen[-1]
        done = tr.buffer.done.cpu().numpy()
        assert len(snap["drop"]) > 0 and sorted(snap["drop"].tolist()) == sorted(R.filter_index(done))
        assert isinstance(snap["kw"]["memory"][0], ppo.FrameRows)
        assert calls == {"table": len(tr.loss_log) if fused else 0, "tensor": 0}
        if want is not None and not _same_snapshot(seen[0], snap):
            want = None             # (the two legs' rollouts differ: the model is replayed for each)
        D, per, L, want = M.trainer_update_against_the_model(tr, snap, want)
        G, gper = M.gradient_distance({k: v.size for k, v in snap["state"].items()}, first["grad"], want.grads[0])
        D1, per1 = M.distance(snap["state"], first["after"], want.states[0])
        got[fused] = {"D": D, "L": L, "G": G, "gper": gper, "D1": D1, "per1": per1}
        print(f"update_fused={fused}: {len(snap['drop'])} of {done.size} rows dropped, {len(tr.loss_log)} steps, L = {L:.1e}  G = {G:.1e}  "
              f"D1 = {D1:.1e} ({max(per1, key=per1.get)})  whole update: D = {D:.1e} ({max(per, key=per.get)})")
        env.check()
        env.close()
    f, s = got[True], got[False]
    print(f"  {'tensor':22s} {'D1 fused':>9s} {'D1 stock':>9s}   {'g1 fused':>9s} {'g1 stock':>9s}")
    for k in M.ORDER:
        print(f"  {k:22s} {f['per1'][k]:9.1e} {s['per1'][k]:9.1e}   {f['gper'][k]:9.1e} {s['gper'][k]:9.1e}")
    assert s["L"] <= L_BAR and f["L"] <= L_BAR
    assert f["G"] <= RATIO * s["G"], (f["G"], s["G"])
    assert f["D1"] <= RATIO * s["D1"], (f["D1"], s["D1"])
