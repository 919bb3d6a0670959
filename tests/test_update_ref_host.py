"""Host: the PPO update in the form ``Stage1Trainer.update()`` runs it -- ``index_batches=None``: one ``randperm`` per epoch,
the small tensors permuted once and sliced, the stacks gathered per minibatch, ``drop_last`` for Stage 2 -- against a float64
model of the reference's update (tests/update_ref.py).

(a) grounds the model in the reference's own run (tests/golden/ppo_update.npz); (b) holds the production path, bit for bit, to
a replay of the permutations it drew, at every way a permutation can be cut; (c) holds it to the model; (d) does the same for
the update the trainer itself assembles on the C oracle env.  tests/test_gpu_update_path.py runs (b) - (d) on the device,
through the HIP kernels.

D and L below are update_ref.distance / loss_distance: the largest per-tensor ||d_got - d_model|| / ||d_model|| of the
parameters' change, and the largest |logged loss - model| / max(1, |model|)."""
import os

import numpy as np
import pytest
import torch

import cpu_train as ct
import rollout_ref as R
import update_ref as M
import util as U

GOLD = os.path.join(U.ROOT, "tests", "golden")
L_BAR = 2e-5        # the project's bar on a logged loss (tests/test_golden_learner.py)
# ten times the largest D measured on the CPU when the bar was set (4.9e-4 over eight synthetic configurations, fp32 against
# the model): the BLAS of the machine that runs this is not pinned.  (The largest the tests below measure: 1.3e-3.)
D_BAR = 5e-3


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("prefix,stage2", [("s1", False), ("s2", True)])
def test_the_model_reproduces_the_reference_run(prefix, stage2):
    """The float64 model, replaying the minibatches the reference's sampler drew, against what the reference's own
    ppo_update_stage{1,2} logged and left behind -- with the bars test_golden_learner._check_update uses on the CPU."""
    from test_golden_learner import formula_state_dict
    net = np.load(os.path.join(GOLD, "net.npz"))
    keys, shapes = [str(k) for k in net["keys"]], [eval(str(s)) for s in net["shapes"]]
    assert tuple(keys) == M.ORDER
    sd0 = formula_state_dict(keys, shapes)
    sd0["logstd"] = torch.from_numpy(net["logstd"])
    g = np.load(os.path.join(GOLD, "ppo_update.npz"), allow_pickle=True)
    P = lambda k: g[f"{prefix}_{k}"]  # noqa: E731
    mem = {"obs": P("obss"), "goal": P("goals"), "speed": P("speeds"), "action": P("actions"), "logprob": P("logprobs"),
           "target": P("targets"), "adv": P("advs")}
    batches = [np.asarray(b, np.int64) for b in P("batches")]
    half = len(batches) // 2
    out = M.update(sd0, mem, P("filter_index") if stage2 else None, [batches[:half], batches[half:]], **M.HP)
    worst = np.abs(out.losses - P("losses")).max()
    print(f"{prefix}: losses within {worst:.1e}")
    assert worst < 2e-5
    new = out.states[-1]
    assert len(out.states) == len(batches) == len(out.grads) and out.grads[0].size == sum(v.numel() for v in sd0.values())
    for i, k in enumerate(keys):
        assert abs(new[k].sum() - P("param_sum")[i]) < 1e-6 * max(1.0, new[k].size ** 0.5), k
        head = new[k].reshape(-1)[:4]
        assert np.abs(head - P("param_head")[i][: head.size]).max() < 1e-6, k
        if k != "logstd":
            delta, want = np.abs(new[k] - sd0[k].double().numpy()).sum(), P("param_delta_abs_sum")[i]
            assert abs(delta - want) <= 0.02 * want + 1e-7, (k, delta, want)


def test_cut_is_the_batch_sampler():
    perm = np.arange(65)[::-1]
    assert [len(b) for b in M.cut(perm, 32, False)] == [32, 32, 1] and [len(b) for b in M.cut(perm, 32, True)] == [32, 32]
    assert [len(b) for b in M.cut(perm[:64], 32, True)] == [32, 32] and M.cut(perm[:20], 32, True) == []
    assert np.array_equal(np.concatenate(M.cut(perm, 32, False)), perm)
    from torch.utils.data import BatchSampler
    for drop_last in (False, True):
        assert [list(b) for b in M.cut(perm, 32, drop_last)] == list(BatchSampler(list(perm), 32, drop_last))


# ---------------------------------------------------------------------------------------------- (b)
def _learner(optim, seed=11):
    """A fresh policy and the optimiser ``optim`` names -> (policy, optimizer, flat_grads)."""
    from mrca import net, ppo
    torch.manual_seed(seed)
    policy = net.CNNPolicy(frames=3, action_space=2)
    if optim == "adam":
        return policy, torch.optim.Adam(policy.parameters(), lr=M.HP["lr"]), None
    fg = ppo.FlatGrads(policy.parameters())
    return policy, ppo.FlatAdam(fg, lr=M.HP["lr"]), fg


def _opt_untouched(opt):
    from mrca import ppo
    if isinstance(opt, ppo.FlatAdam):
        return opt.steps == 0 and not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())
    return len(opt.state) == 0


# (T, N, batch, what Stage 2 drops) -- the rows and minibatches (Stage 1 | Stage 2) each leaves:
CUTS = [
    (6, 64, 128, "runs"),       # 384 = 3 x 128 | fewer: two whole minibatches, the short one dropped
    (5, 7, 8, "runs"),          # 35 = 4 x 8 + 3: a short last minibatch
    (5, 13, 32, "runs"),        # 65 = 2 x 32 + 1: a last minibatch of ONE row | 2 x 32 or fewer
    (4, 5, 64, "runs"),         # 20 < 64: one short minibatch | no step at all
    (5, 13, 32, "empty"),       # an empty drop list
    (5, 13, 32, "none"),        # filter_index=None
    (5, 13, 32, "carry"),       # one row dropped, by the cross-robot carry alone: 64 = 2 x 32 left, an exact multiple
]


def _drop_list(T, N, what, seed=3):
    """-> (the drop list ppo.get_filter_index gives for synthetic flags, or None), checked against the model's walk."""
    from mrca import ppo
    if what == "none":
        return None
    d = M.done_flags(T, N, np.random.default_rng(seed), empty=(what == "empty"), single_carry=3 if what == "carry" else None)
    drop = ppo.get_filter_index(torch.from_numpy(d))
    assert sorted(drop.tolist()) == sorted(R.filter_index(d))
    assert (len(drop) == 0) == (what == "empty")
    if what == "carry":
        assert drop.tolist() == [4]         # tick 0 of robot 4, handed the run of robot 3's last tick
    else:
        # the carry is among the dropped rows whenever anything is: robot N-1's tick 0 is done after robot N-2's last tick alone
        assert what == "empty" or N - 1 in drop.tolist()
    return drop


@pytest.mark.parametrize("store", ["frame_rows", "stacks"])
@pytest.mark.parametrize("optim", ["adam", "flat_adam"])
@pytest.mark.parametrize("T,N,batch,what,stage2", [c + (False,) for c in CUTS if c[3] == "runs"] + [c + (True,) for c in CUTS])
def test_production_path_equals_the_replay_of_its_permutations(T, N, batch, what, stage2, optim, store):
    """``index_batches=None`` against the same update handed back, through ``index_batches``, the permutations it drew, cut as
    torch's BatchSampler cuts them: parameters and loss log equal to the bit.  A slip in how the production path lines up its
    slices of the permuted small tensors with its gathers of the stacks shows here."""
    from mrca import ppo
    torch.set_num_threads(2)
    pol0, _o, _f = _learner("adam")
    mem, frames, fidx = M.synthetic_memory(M.state_of(pol0), T, N, seed=T * N)
    drop = _drop_list(T, N, what) if stage2 else None
    left = T * N - (0 if drop is None else len(drop))
    steps = 2 * (left // batch if stage2 else -(-left // batch))

    def memory():
        rows = ppo.FrameRows(torch.from_numpy(frames), torch.from_numpy(fidx)) if store == "frame_rows" else None
        return M.torch_memory(mem, "cpu", rows)

    pol, opt, fg = _learner(optim)
    before = M.state_of(pol)
    log, perms = M.run_update(ppo, pol, opt, fg, memory(), T, N, batch, stage2, drop)
    assert len(perms) == 2 and all(sorted(p.tolist()) == list(range(left)) for p in perms)
    assert len(log) == steps
    if steps == 0:
        assert stage2 and left < batch
        assert all(np.array_equal(before[k], v) for k, v in M.state_of(pol).items()) and _opt_untouched(opt)
        return
    if (T, N, batch) == (5, 13, 32) and not stage2:
        assert M.cut(perms[0], batch, False)[-1].size == 1
    if what == "carry":
        assert left == 2 * batch
    pol2, opt2, fg2 = _learner(optim)
    log2, perms2 = M.run_update(ppo, pol2, opt2, fg2, memory(), T, N, batch, stage2, drop,
                                index_batches=M.replay_batches(perms, batch, stage2, "cpu"))
    assert perms2 == []
    assert len(log2) == steps and all(torch.equal(torch.stack(a), torch.stack(b)) for a, b in zip(log, log2))
    moved = 0
    for (k, a), b in zip(pol.state_dict().items(), pol2.state_dict().values()):
        assert torch.equal(a, b), k
        moved += int((a.double().numpy() != before[k]).sum())
    assert moved > 0


# ---------------------------------------------------------------------------------------------- (c)
def _against_the_model(T, N, batch, stage2, optim="flat_adam", store="frame_rows", **opts):
    """The production path on a synthetic memory against the model replaying the permutations it drew -> (D, L, the model's
    Update, the learner's flat_grads)."""
    from mrca import ppo
    torch.set_num_threads(2)
    pol, opt, fg = _learner(optim)
    before = M.state_of(pol)
    mem, frames, fidx = M.synthetic_memory(before, T, N, seed=T * N)
    inside, below, above = M.ratio_classes(before, mem, M.HP["clip"])
    assert inside > 0 and below > 0 and above > 0, (inside, below, above)
    drop = _drop_list(T, N, "runs") if stage2 else None
    rows = ppo.FrameRows(torch.from_numpy(frames), torch.from_numpy(fidx)) if store == "frame_rows" else None
    log, perms = M.run_update(ppo, pol, opt, fg, M.torch_memory(mem, "cpu", rows), T, N, batch, stage2, drop, **opts)
    want = M.update(before, mem, None if drop is None else drop.numpy(), [M.cut(p, batch, stage2) for p in perms],
                    every_state=False, **M.HP, **opts)
    assert len(log) == len(want.losses) > 0
    D, per = M.distance(before, M.state_of(pol), want.states[-1])
    L = M.loss_distance(log, want.losses)
    print(f"stage{1 + stage2} {T}x{N}/{batch} {optim} {store} {opts}: D = {D:.1e} ({max(per, key=per.get)})  L = {L:.1e}  "
          f"ratios inside / below / above the clip range: {inside} / {below} / {above}")
    return D, L, want, fg


@pytest.mark.parametrize("optim,store", [("flat_adam", "frame_rows"), ("adam", "stacks")])
@pytest.mark.parametrize("stage2", [False, True], ids=["stage1", "stage2"])
@pytest.mark.parametrize("T,N,batch", [(6, 64, 128), (5, 13, 32)])
def test_production_path_against_the_model(T, N, batch, stage2, optim, store):
    """Measured on the CPU (fp32 against float64; 2 threads), D and L -- the same for FlatGrads + FlatAdam over a FrameRows and
    for torch.optim.Adam over materialised stacks:

        stage1 6x64/128   1.2e-4  1.1e-7        stage1 5x13/32   6.5e-4  1.0e-7
        stage2 6x64/128   4.2e-4  1.3e-7        stage2 5x13/32   1.1e-4  8.3e-8

    (the worst tensor is actor2.bias every time: one number, moved by six steps of a gradient that is a sum over the minibatch).
    """
    D, L, _want, _fg = _against_the_model(T, N, batch, stage2, optim, store)
    assert L <= L_BAR and D <= D_BAR


@pytest.mark.parametrize("optim", ["flat_adam", "adam"])
def test_production_path_against_the_model_with_a_gradient_clip(optim):
    """``max_grad_norm`` small enough to clip every step.  (Adam's first steps barely see a gradient's scale, so the clipped
    gradient itself is compared too, where the learner keeps it: the flat bucket after the last step.)  Measured: D 9.0e-4,
    L 9.8e-8, the bucket within 5.6e-6 of the model's last gradient."""
    c = 0.05
    D, L, want, fg = _against_the_model(6, 64, 128, False, optim, max_grad_norm=c)
    assert min(want.grad_norms) > 2 * c, want.grad_norms
    assert L <= L_BAR and D <= D_BAR
    if fg is not None:
        g = fg.flat.double().numpy()
        rel = np.linalg.norm(g - want.grads[-1]) / np.linalg.norm(want.grads[-1])
        print(f"clipped gradient of the last step: norm {np.linalg.norm(g):.6f}, within {rel:.1e} of the model's")
        assert abs(np.linalg.norm(g) - c) < 1e-5 and rel <= D_BAR


def test_production_path_against_the_model_with_a_logstd_floor():
    """``logstd_min`` above the initial log standard deviation (0): the floor holds it after every step, and the entropy every
    later step logs is the floor's.  Measured: D 2.2e-4, L 9.0e-8."""
    D, L, want, _fg = _against_the_model(6, 64, 128, True, logstd_min=0.1)
    assert np.allclose(want.states[-1]["logstd"], 0.1) and abs(want.losses[1, 2] - 2 * (0.5 + M._HALF_LOG_2PI + 0.1)) < 1e-12
    assert L <= L_BAR and D <= D_BAR


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("name,T", [("stage2", 16), ("stage1", 12)])
def test_trainer_update_on_the_oracle_env_against_the_model(name, T, monkeypatch):
    """``Stage1Trainer`` on the C oracle env runs a horizon and its own update; the model is replayed from what the trainer
    handed ``ppo_update_stage{1,2}``.  Pins the trainer's wiring: the order of the memory tuple, that the advantages arrive
    raw (normalised over all rows inside the update), which rows are dropped.  Measured on the CPU: stage2 (T = 16: 61 of 4224
    rows dropped, 16 steps) D 7.2e-5, L 2.5e-7; stage1 (T = 12, 3108 rows, 8 steps, the last minibatch of an epoch 36 rows)
    D 1.3e-3, L 2.3e-7.

    Over this many steps on real rollouts D is not rounding alone: a single nearly dead conv channel whose ReLU inputs sit
    within 1e-8 of zero can part from the model in one step and take the actor's trajectory with it (measured on a rollout of
    the device env replayed here: D 8.5e-4 with 2 threads, 7.2e-3 with 8; tests/test_gpu_update_path.py has the account).
    The thread count is pinned below for that reason; the rollouts of this test stay within the bar with 2 and with 8."""
    from mrca import ppo, vec_env
    from mrca.trainer import HParams, Stage1Trainer
    monkeypatch.setattr(vec_env, "gae", ct._gae_cpu)
    torch.set_num_threads(2)
    stage2 = name == "stage2"
    sc, _lead = R.scenario(name, T)
    seen = M.snapshot_updates(monkeypatch, ppo)
    hp = HParams(horizon=T, batch_size=512, epoch=2) if stage2 else HParams(horizon=T, epoch=2)
    tr = Stage1Trainer(ct.CpuEnv(sc), hp=hp, seed=3, stage2=stage2)
    tr.start()
    for _ in range(T):
        tr.tick()
    assert tr.global_update == 1 and len(seen) == 1 and seen[0]["stage2"] == stage2
    snap = seen[0]
    done = tr.buffer.done.numpy()
    if stage2:
        assert len(snap["drop"]) > 0 and sorted(snap["drop"].tolist()) == sorted(R.filter_index(done))
    else:
        assert (T * sc.num_robots) % hp.batch_size not in (0, 1)          # a short last minibatch
    D, per, L = M.trainer_update_against_the_model(tr, snap)[:3]
    print(f"{name}: {0 if snap['drop'] is None else len(snap['drop'])} of {done.size} rows dropped, {len(tr.loss_log)} steps, "
          f"D = {D:.1e} ({max(per, key=per.get)})  L = {L:.1e}")
    assert L <= L_BAR and D <= D_BAR
