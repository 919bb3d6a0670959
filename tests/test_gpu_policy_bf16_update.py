"""GPU: the opt-in fused bf16 PPO update -- the bf16 MFMA backward kernel of the lidar front end
(csrc/mrca_policy_bf16_bwd.hip) against its float64 contract reference (tests/bf16_bwd_ref.py), the row-table forward
(csrc/mrca_policy_bf16_rows.hip), the whole policy's gradients against a float64 emulation of the contract, the update's
forward against the rollout's bf16 inference, one update end to end, and the train CLI.  This is an opt-in precision, not the
reference's; fp32 stays the default.  Measured figures: profiles/bf16_update/."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_bwd_ref as B
import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pol():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca.net import CNNPolicy
    torch.manual_seed(3)
    p = CNNPolicy(3, 2).cuda()
    with torch.no_grad():                      # not the symmetric default init: distinct, sizeable biases
        for q in p.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return p


def _inputs(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, 3, 512, device="cuda", generator=g) - 0.5
    ga = torch.randn(n, 4096, device="cuda", generator=g).to(torch.bfloat16)
    gc = torch.randn(n, 4096, device="cuda", generator=g).to(torch.bfloat16)
    return x, ga, gc


def _forward_h1(x, w1, b1):
    """h1 as the forward kernel forms it, f32[2, n, 32, 255]: the bf16 forward run with conv2 = "copy tap 1" (the even
    positions) and "copy tap 2" (the odd ones) and no bias -- relu and the last rounding leave a bf16 h1 >= 0 as it is."""
    from mrca import policy_ops
    n = x.shape[0]
    h1 = torch.zeros(2, n, 32, 256, device="cuda")
    for tap in (1, 2):
        w2 = torch.zeros(2, 32, 32, 3, device="cuda")
        w2[:, torch.arange(32), torch.arange(32), tap] = 1.0
        f = policy_ops.lidar_features_bf16(x, w1, b1, w2, torch.zeros(2, 32, device="cuda")).float().view(2, n, 32, 128)
        h1[:, :, :, tap - 1::2] = f
    assert float(h1[..., 255].abs().max()) == 0.0           # "h1[255]" is conv2's padding
    return h1[..., :255].contiguous()


@pytest.mark.parametrize("n", [1, 2, 3, 7, 255, 512])
def test_backward_kernel_follows_the_contract(pol, n):
    """Each of dw1, db1, dw2, db2 within 2e-5 of its largest element of the float64 contract reference -- the project's gate for
    an fp32-accumulated MFMA backward against float64 (tests/test_gpu_policy_bwd.py).  feat comes from the bf16 forward kernel,
    so both sides use the same second ReLU mask -- and so does h1 ("recomputed exactly as the forward forms it"), read out of
    the forward kernel by _forward_h1: the hardware's fp32 sum and the reference's float64 sum land a few h1 values per sample
    on different sides of a bf16 rounding boundary (a contract point, not a stray rounding), and ONE such value moves 96 entries
    of dw2 by |g2| x one bf16 ulp -- first measurement, float64 h1 on the reference's side: n = 1, actor dw2 7.3e-5 of the
    largest element, the critic's (no such value) 5.8e-8, dw1 1.1e-7, db1 = db2 = 0.  The handed-in h1 is itself held to the
    reference's: at most one bf16 ulp apart, on at most 1e-3 of the values.  The figure with the reference's own h1 is
    printed beside the asserted one.  MEASURED (profiles/bf16_update/test_gpu_policy_bf16_update.txt), worst ratio with the
    handed-in h1 / with the reference's own: n = 1: 1.4e-7 / 7.3e-5, 2: 1.4e-7 / 3.3e-6, 3: 1.0e-7 / 1.0e-7, 7: 9.6e-7 / 4.0e-5,
    255: 1.45e-5 / 1.66e-5, 512: 1.96e-5 / 2.02e-5 (1 .. 79 h1 values of up to 8.4 M round the other way).  At 255 and 512
    the figure is conv1's: dw1 / db1, where g1 -- a rounding point INSIDE the backward kernel, fp32 sum against float64 sum --
    rounds the other way now and then; dw2 / db2 stay below 1e-7."""
    from mrca import policy_ops
    rc = pol.refresh_rollout_cache()
    x, ga, gc = _inputs(n, 40 + n)
    feat = policy_ops.lidar_features_bf16(x, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    got = policy_ops.lidar_features_bf16_backward(x, rc["w1"], rc["b1"], rc["w2"], feat, ga, gc)
    h1_hw = _forward_h1(x, rc["w1"], rc["b1"])
    h = lambda t: t.float().cpu().numpy()          # noqa: E731
    report, own_worst, flips = [], 0.0, 0
    for t, g in enumerate((ga, gc)):
        args = (h(x), h(rc["w1"][t]), h(rc["b1"][t]), h(rc["w2"][t]), h(rc["b2"][t]), h(g))
        *own, h1_ref = B.front_end_bwd_ref(*args, feat=h(feat[t]), return_h1=True)
        hw = h(h1_hw[t]).astype(np.float64)
        differ = hw != h1_ref
        flips += int(differ.sum())
        assert differ.mean() <= 1e-3, (t, n, float(differ.mean()))
        # one bf16 ulp (<= 2^-7 of the value), or -- around the ReLU's zero -- the error of an fp32 sum of 16 terms of size <= 1
        assert (np.abs(hw - h1_ref) <= 2.0 ** -7 * np.maximum(np.abs(h1_ref), np.abs(hw)) + 2.0 ** -18).all(), (t, n)
        want = B.front_end_bwd_ref(*args, feat=h(feat[t]), h1=hw)
        for name, a, b, o in zip(("dw1", "db1", "dw2", "db2"), got, want, own):
            a64 = a[t].cpu().numpy().astype(np.float64)
            scale = float(np.abs(b).max())
            report.append((t, name, float(np.abs(a64 - b).max()) / scale, scale))
            own_worst = max(own_worst, float(np.abs(a64 - o).max()) / float(np.abs(o).max()))
    worst = max(r for _t, _k, r, _s in report)
    print(f"n={n}: worst |kernel - contract reference| / largest element = {worst:.3g} "
          f"(with the reference's own float64 h1: {own_worst:.3g}; {flips} of {2 * n * 8160} h1 values round the other way)  "
          + " ".join(f"{'ac'[t]}.{k}={r:.2g}" for t, k, r, _ in report))
    for t, name, ratio, scale in report:
        assert scale > 0.1, (t, name, n, scale)
        assert ratio < 2e-5, (t, name, n, ratio, scale)


def _table(n, seed):
    from mrca import policy_ops
    g = torch.Generator().manual_seed(seed)
    store = (torch.rand(3 * n + 11, 512, generator=g) - 0.5).cuda()
    rows = torch.randint(0, store.shape[0], (n, 3), generator=g, dtype=torch.int32).cuda()        # any rows, repeats included
    return policy_ops.FrameTable(store, rows)


@pytest.mark.parametrize("n", [1, 7, 300, 4097])
def test_row_table_form_equals_the_gathered_form_bit_for_bit(pol, n):
    from mrca import policy_ops
    rc = pol.refresh_rollout_cache()
    w = (rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    table = _table(n, 900 + n)
    x = table.gather().contiguous()
    feat_t = policy_ops.lidar_features_bf16_rows(table, *w)
    feat_x = policy_ops.lidar_features_bf16(x, *w)
    assert feat_t.dtype == torch.bfloat16 and torch.equal(feat_t, feat_x)
    assert float(feat_x.float().abs().max()) > 0.05
    _x, ga, gc = _inputs(n, 7 + n)
    got_t = policy_ops.lidar_features_bf16_backward(table, *w[:3], feat_t, ga, gc)
    got_x = policy_ops.lidar_features_bf16_backward(x, *w[:3], feat_x, ga, gc)
    again = policy_ops.lidar_features_bf16_backward(x, *w[:3], feat_x, ga, gc)
    for name, a, b, c in zip(("dw1", "db1", "dw2", "db2"), got_t, got_x, again):
        assert torch.equal(a, b), name
        assert torch.equal(b, c), name           # two launches agree bit for bit
        assert float(b.abs().max()) > 0, name


def test_minibatch_size_is_deterministic_whatever_else_the_gpu_runs(pol):
    """n = 16 384: the same bits from a launch on an idle GPU and from one that shares the CUs with a stream of GEMMs (the
    waves then fill the grid in another order; the partial sums are combined in a fixed order)."""
    from mrca import policy_ops
    rc = pol.refresh_rollout_cache()
    n = 16384
    x, ga, gc = _inputs(n, 5)
    ga, gc = (ga.float() / n).to(torch.bfloat16), (gc.float() / n).to(torch.bfloat16)
    feat = policy_ops.lidar_features_bf16(x, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    torch.cuda.synchronize()
    idle = policy_ops.lidar_features_bf16_backward(x, rc["w1"], rc["b1"], rc["w2"], feat, ga, gc)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.mm(a, a).clamp_(-1, 1)
    busy = policy_ops.lidar_features_bf16_backward(x, rc["w1"], rc["b1"], rc["w2"], feat, ga, gc)
    torch.cuda.synchronize()
    for name, u, v in zip(("dw1", "db1", "dw2", "db2"), idle, busy):
        assert torch.equal(u, v), name
        assert torch.isfinite(u).all() and float(u.abs().max()) > 0, name


# ---------------------------------------------------------------------------------------------- the whole policy
class _RoundGrad(torch.autograd.Function):
    """identity whose backward rounds the gradient to bf16 (a backward rounding point of the contract).  ``hw``: the rounded
    gradient as the GPU formed it at this point -- passed on in place of this function's own rounding, the pair appended to
    ``log`` so that the caller can hold the one to the other"""

    @staticmethod
    def forward(ctx, t, hw=None, log=None):
        ctx.hw, ctx.log = hw, log
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        own = g.float().to(torch.bfloat16).to(g.dtype)
        if ctx.hw is None:
            return own, None, None
        ctx.log.append((own, ctx.hw.to(g.dtype)))
        return ctx.hw.to(g.dtype), None, None


def _st(t):
    """round to bf16, straight-through"""
    return t + (t.float().to(torch.bfloat16).to(t.dtype) - t).detach()


def _as(hw, t):
    """the value the hardware formed (None: t's own), the gradient of t"""
    return t if hw is None else t + (hw.to(t.dtype) - t).detach()


def _emulated_mean_value(p, x, goal, speed, h1_hw=None, feat_hw=None, g_hw=None, gfeat_hw=None, log=None):
    """float64 torch emulation of CNNPolicy.mean_value under fused_train_bf16: explicit roundings at the contract points.
    ``h1_hw`` [2,n,32,255] / ``feat_hw`` [2,n,4096]: the forward's two ROUNDED activations as the kernel formed them (their few
    values that the fp32 sums round the other way, see test_backward_kernel_follows_the_contract), gradients straight-through;
    ``g_hw`` [2][n,256] / ``gfeat_hw`` [2][n,4096]: the two backward roundings OUTSIDE the kernel (fc1's incoming gradient, gfeat)
    as the GPU formed them; ``log`` collects (own rounding, handed-in one) pairs"""
    z = []
    xr = _st(x)
    for t, tw in enumerate(p.TOWERS):
        c1, c2 = getattr(p, f"{tw}_fea_cv1"), getattr(p, f"{tw}_fea_cv2")
        fc1, fc2 = getattr(p, f"{tw}_fc1"), getattr(p, f"{tw}_fc2")
        pre1 = _RoundGrad.apply(F.conv1d(xr, _st(c1.weight), c1.bias, stride=2, padding=1))       # g1 is rounded
        h1 = _as(None if h1_hw is None else h1_hw[t], _st(torch.relu(pre1)))
        feat = _st(torch.relu(F.conv1d(h1, _st(c2.weight), c2.bias, stride=2, padding=1))).flatten(1)
        feat = _as(None if feat_hw is None else feat_hw[t], feat)
        feat = _RoundGrad.apply(feat, None if gfeat_hw is None else gfeat_hw[t], log)           # gfeat is stored as bf16
        h = _RoundGrad.apply(feat @ _st(fc1.weight).t(), None if g_hw is None else g_hw[t], log) + fc1.bias   # fc1's output gradient is rounded
        z.append(torch.relu(F.linear(torch.cat((torch.relu(h), goal, speed), dim=-1), fc2.weight, fc2.bias)))
    mean = torch.cat((torch.sigmoid(p.actor1(z[0])), torch.tanh(p.actor2(z[0]))), dim=-1)
    return mean, p.critic(z[1])


def _ppo_loss(mean, value, logstd, action, old_logprob, adv, target, clip_value, value_coef, coeff_entropy):
    from mrca.net import _HALF_LOG_2PI, gaussian_logprob
    ls = logstd.expand_as(mean)
    ratio = torch.exp(gaussian_logprob(action, mean, ls) - old_logprob)
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip_value, 1 + clip_value) * adv).mean()
    entropy = (0.5 + _HALF_LOG_2PI + ls).sum(-1).mean()
    return policy_loss + value_coef * F.mse_loss(value, target) - coeff_entropy * entropy


def _loss_inputs(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, 3, 512, device="cuda", generator=g) - 0.5
    goal = torch.rand(n, 2, device="cuda", generator=g) * 10 - 5
    speed = torch.rand(n, 2, device="cuda", generator=g)
    act = torch.rand(n, 2, device="cuda", generator=g)
    old_lp = torch.randn(n, 1, device="cuda", generator=g) * 0.1 - 2.0
    adv = torch.randn(n, 1, device="cuda", generator=g)
    tgt = torch.randn(n, 1, device="cuda", generator=g)
    return x, goal, speed, act, old_lp, adv, tgt


def test_policy_gradients_follow_the_contract(pol, monkeypatch):
    """fused_train_bf16, n = 64: the gradient of every parameter from mean_value + ppo_loss against a float64 torch emulation
    with explicit .to(bfloat16) roundings at the contract points (straight-through).  Bar: 2e-5 of each gradient's largest
    element.
    A bf16 rounding of an fp32 sum (the GPU) and of a float64 sum (the emulation) take different sides where the value lies
    within ~1e-7 of a rounding boundary, and at n = 64 one such value is one term of 64 in its row of a weight gradient.  So the
    emulation takes the GPU's choice at the four rounding points that can be read from outside -- h1 and feat out of the
    forward kernel (as test_backward_kernel_follows_the_contract does), fc1's incoming gradient and gfeat off autograd hooks
    while mean_value itself runs -- and holds each handed-in tensor to its own rounding: at most one bf16 ulp apart, on at
    most 1e-3 of the values.  g1, inside the backward kernel, stays the emulation's own.
    MEASURED (profiles/bf16_update/test_gpu_policy_bf16_update.txt), worst error over largest element: every rounding the
    emulation's own 9.5e-4; h1 and feat handed in 3.7e-4 (act_fea_cv1.weight; act_fc1.weight 2.65e-4); all four handed in
    2.7e-6 (act_fea_cv1.weight; its bias 2.3e-6; every other tensor 3e-10 .. 3e-7) -- the GPU took 2 + 15 + 1 + 8 of the
    2 x (16 384 + 262 144) backward values the other way, 8 features and a handful of h1 values forward.  The forward agrees to
    1.1e-7 (mean) / 1.4e-7 (value)."""
    from mrca import policy_ops
    n = 64
    x, goal, speed, act, old_lp, adv, tgt = _loss_inputs(n, 21)
    p = copy.deepcopy(pol)
    p.fused_train = p.fused_train_bf16 = True
    p.zero_grad()
    # what the GPU forms at the two backward rounding points outside the kernel, read off autograd as mean_value runs
    g_rec, gfeat_rec, fc1_bf16 = {}, {}, policy_ops.fc1_bf16

    def recording_fc1(feat, weight, weight_bf16):
        k = len(g_rec) + len(gfeat_rec)
        g_rec[k], gfeat_rec[k] = None, None
        feat.register_hook(lambda g: gfeat_rec.__setitem__(k, g.detach().clone()))
        out = fc1_bf16(feat, weight, weight_bf16)
        out.register_hook(lambda g: g_rec.__setitem__(k, g.detach().to(torch.bfloat16)))
        return out

    monkeypatch.setattr(policy_ops, "fc1_bf16", recording_fc1)
    mean, value = p.mean_value(x, goal, speed)
    monkeypatch.undo()
    loss, _stats = policy_ops.ppo_loss(mean, value, p.logstd, act, old_lp, adv, tgt, 0.1, 20.0, 5e-4)
    loss.backward()
    got = {k: q.grad.detach().double().cpu() for k, q in p.named_parameters()}
    keys = sorted(g_rec)
    assert len(keys) == 2 and all(g_rec[k] is not None and gfeat_rec[k] is not None for k in keys)
    g_hw = [g_rec[k].double().cpu() for k in keys]                  # actor, critic: the order mean_value calls fc1 in
    gfeat_hw = [gfeat_rec[k].double().cpu() for k in keys]
    assert gfeat_rec[keys[0]].dtype == torch.bfloat16
    rc = p.refresh_rollout_cache()
    feat_hw = policy_ops.lidar_features_bf16(x, rc["w1"], rc["b1"], rc["w2"], rc["b2"]).double().cpu()
    h1_hw = _forward_h1(x, rc["w1"], rc["b1"]).double().cpu()
    ref = copy.deepcopy(pol).cpu().double()
    d = lambda t: t.cpu().double()          # noqa: E731

    def emulate(**hw):
        ref.zero_grad()
        m64, v64 = _emulated_mean_value(ref, d(x), d(goal), d(speed), **hw)
        _ppo_loss(m64, v64, ref.logstd, d(act), d(old_lp), d(adv), d(tgt), 0.1, 20.0, 5e-4).backward()
        return m64.detach(), v64.detach(), {k: q.grad.detach().clone() for k, q in ref.named_parameters()}

    worst = lambda w: max(float((got[k] - w[k]).abs().max()) / float(w[k].abs().max()) for k in w)      # noqa: E731
    print("with the emulation's own float64 roundings everywhere: worst ratio %.3g" % worst(emulate()[2]))
    print("with the forward's h1 and feat handed in: worst ratio %.3g" % worst(emulate(h1_hw=h1_hw, feat_hw=feat_hw)[2]))
    log = []
    m64, v64, want = emulate(h1_hw=h1_hw, feat_hw=feat_hw, g_hw=g_hw, gfeat_hw=gfeat_hw, log=log)
    # the handed-in roundings are held to the emulation's own: one bf16 ulp apart at most (or, around zero, the error of an
    # fp32 sum: 2^-18 of the tensor's largest value), on at most 1e-3 of the values
    assert len(log) == 4
    flips = []
    for own, hw in log:
        differ = own != hw
        flips.append(int(differ.sum()))
        assert float(differ.double().mean()) <= 1e-3, flips
        assert bool(((own - hw).abs() <= 2.0 ** -7 * torch.maximum(own.abs(), hw.abs()) + 2.0 ** -18 * own.abs().max()).all())
    print(f"backward roundings the GPU took the other way (crt g, crt gfeat, act g, act gfeat in backward order): {flips}")
    print(f"forward: max |d mean| {float((mean.detach().double().cpu() - m64).abs().max()):.3g}, "
          f"max |d value| {float((value.detach().double().cpu() - v64).abs().max()):.3g}")
    ratios = {}
    for k in want:
        scale = float(want[k].abs().max())
        ratios[k] = float((got[k] - want[k]).abs().max()) / scale
        print(f"  {k:22s} max error / largest element {ratios[k]:.3g}   (largest element {scale:.3g})")
    print(f"whole policy, n={n}: worst ratio {max(ratios.values()):.3g}")
    for k, r in ratios.items():
        assert r < 2e-5, (k, r)


def _pair_distance(p, x, goal, speed, bf16):
    from mrca import ppo
    lo, hi = ppo._bounds(((0.0, -1.0), (1.0, 1.0)), x.device, torch.float32)
    p.fused_train, p.fused_train_bf16 = True, bf16
    with torch.no_grad():
        mean, value = p.mean_value(x, goal, speed)
        v_a, _a, _lp, _s, m_a = p.act_fused(x, goal, speed, None, lo, hi, bf16=bf16)
        m_f, v_f = p.mean_value_fused(x, goal, speed, bf16=bf16)
    d = 0.0
    for m, v in ((m_a, v_a), (m_f, v_f)):
        d = max(d, float((mean - m).abs().max()), float(((value - v).abs() / (1.0 + v.abs())).max()))
    return d


def test_update_forward_is_the_rollouts_forward(pol):
    """mean and value of the update's bf16 forward against act_fused(bf16=True) / mean_value_fused(bf16=True) on the same
    observations: identical rounding points (the front end is the same device code: identical features), so they differ by
    fc1's and fc2's GEMM summation order only.  Yardstick: the same distance of the fp32 pair (the fused fp32 update forward
    against act_fused(bf16=False), code this change does not touch), measured here beside it; the bf16 pair gets 4x that
    (fc1's output is fp32 in both paths).  Distance = max(|d mean|, |d value| / (1 + |value|)) over 1000 robots.
    MEASURED (profiles/bf16_update/test_gpu_policy_bf16_update.txt): fp32 pair 1.19e-7, bf16 pair 1.19e-7 (allowed 4.77e-7)."""
    n = 1000
    x, goal, speed = _loss_inputs(n, 33)[:3]
    p = copy.deepcopy(pol)
    d32 = _pair_distance(p, x, goal, speed, False)
    d16 = _pair_distance(p, x, goal, speed, True)
    print(f"update forward vs rollout forward: fp32 pair {d32:.3g}, bf16 pair {d16:.3g} (allowed {4 * d32:.3g})")
    assert d32 > 0 or d16 == 0
    assert d16 <= 4 * d32


def _real_buffer(horizon=32):
    from mrca import ppo
    from mrca.trainer import HParams, Stage1Trainer
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(U.S.stage1(num_worlds=8, robots_per_world=24, seed=5), device="cuda:0")
    hp = HParams(horizon=horizon, batch_size=1024, epoch=2, rollout_fused=True, update_fused=True)
    tr = Stage1Trainer(env, hp=hp, seed=2)
    tr.start()
    for _ in range(horizon - 1):
        tr.tick()
    # the last tick without the trainer's own update: the buffer stays as the rollout left it
    obs, head = ppo.policy_input(env, True)
    v, a, logprob, scaled = ppo.generate_action(tr.policy, obs, env.local_goal, env.speed, hp.action_bound, tr.gen, None, True, head)
    so, sn = tr._stored_obs()
    tr.buffer.store_state(tr.t, so, env.local_goal, env.speed, a, logprob, v, env.fresh, newest=sn)
    env.step(scaled.contiguous())
    tr.buffer.store_outcome(tr.t, env.reward, env.done)
    with torch.no_grad():
        obs, head = ppo.policy_input(env, True)
        _m, last_v = tr.policy.mean_value_fused(obs, env.local_goal, env.speed, head=head)
    buf = tr.buffer
    targets, advs = ppo.generate_train_data(buf.reward, hp.gamma, buf.value, last_v, buf.done, hp.lam)
    memory = (buf.obs_rows(), buf.goal, buf.speed, buf.action, buf.logprob, targets, buf.value, buf.reward, advs)
    return env, tr, hp, memory


def test_one_update_end_to_end():
    """ppo_update_stage1 on a real 8 x 24-robot buffer: fused bf16, fused fp32 and the autocast bf16 path (the bf16 update
    that existed before) from the same parameters on the same minibatches.  The fused bf16 parameter change correlates with
    fused fp32's, and its relative distance to it is at most 2x the autocast path's: both round at comparable points.
    MEASURED (profiles/bf16_update/test_gpu_policy_bf16_update.txt), 8 x 24 robots x 32 ticks, 12 minibatches of 1024: autocast
    bf16 0.0810 of the fp32 parameter change (measured first, the yardstick), fused bf16 0.0755; cosine 0.99715."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import ppo
    env, tr, hp, memory = _real_buffer()
    start = copy.deepcopy(tr.policy.state_dict())
    batches = lambda n: list(torch.arange(n, device="cuda").split(hp.batch_size))      # noqa: E731
    deltas, logs = {}, {}
    for name, fused, bf16, autocast in (("fp32", True, False, None), ("fused_bf16", True, True, None),
                                        ("autocast_bf16", False, False, torch.bfloat16)):
        p = copy.deepcopy(tr.policy)
        p.load_state_dict(start)
        p.fused_train, p.fused_train_bf16 = fused, bf16
        opt = torch.optim.Adam(p.parameters(), lr=hp.learning_rate)
        log = []
        before = torch.cat([q.detach().flatten().clone() for q in p.parameters()])
        ppo.ppo_update_stage1(p, opt, hp.batch_size, memory, epoch=hp.epoch, coeff_entropy=hp.coeff_entropy,
                              clip_value=hp.clip_value, num_step=hp.horizon, num_env=env.N, frames=3, obs_size=512, act_size=2,
                              value_coef=hp.value_coef, index_batches=batches, log=log, autocast_dtype=autocast)
        after = torch.cat([q.detach().flatten() for q in p.parameters()])
        assert torch.isfinite(after).all(), name
        deltas[name] = (after - before).double()
        logs[name] = log
        if name == "fused_bf16":
            assert memory[0].lazy, "the fused bf16 update did not read the frame store through row tables"
    d32 = deltas["fp32"]
    cos = float(F.cosine_similarity(deltas["fused_bf16"], d32, dim=0))
    rel_fused = float((deltas["fused_bf16"] - d32).norm() / d32.norm())
    rel_auto = float((deltas["autocast_bf16"] - d32).norm() / d32.norm())
    print(f"one update, 8 x 24 robots x {hp.horizon} ticks: cosine(fused bf16, fp32) {cos:.5f}; relative distance to the fp32 "
          f"parameter change: fused bf16 {rel_fused:.4g}, autocast bf16 {rel_auto:.4g} (allowed {2 * rel_auto:.4g})")
    for name, log in logs.items():
        assert len(log) == hp.epoch * len(batches(env.N * hp.horizon)), name
        for row in log:                   # policy loss, value loss, entropy: the three figures of a ppo log line
            assert len(row) == 3 and all(bool(torch.isfinite(v)) for v in row), name
    assert cos > 0.9
    assert rel_fused <= 2 * rel_auto
    env.close()


def test_trainer_runs_with_both_bf16_flags():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mrca.trainer import HParams, Stage1Trainer
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(U.S.stage1(num_worlds=4, robots_per_world=24, seed=8))
    with pytest.raises(ValueError):
        Stage1Trainer(env, hp=HParams(update_bf16=True), seed=4)
    hp = HParams(horizon=16, batch_size=192, epoch=1, rollout_fused=True, rollout_bf16=True, update_fused=True, update_bf16=True)
    tr = Stage1Trainer(env, hp=hp, seed=4)
    tr.start()
    for _ in range(2 * hp.horizon):
        tr.tick()
    torch.cuda.synchronize()
    assert tr.global_update == 2 and len(tr.loss_log) > 0
    assert all(torch.isfinite(torch.stack(x)).all() for x in tr.loss_log)
    # the update's bf16 copy of fc1 and the rollout cache's are casts of the same master weights
    wb = tr.policy._fc1_train_bf16()
    assert torch.equal(wb["act"].t(), tr.policy._rc_bf16[0]) and torch.equal(wb["crt"].t(), tr.policy._rc_bf16[1])
    assert all(q.dtype == torch.float32 for q in tr.policy.parameters())
    env.close()


def test_train_cli_fused_bf16_update(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pdir = tmp_path / "policy"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), U.ROOT]))
    r = subprocess.run([sys.executable, "-m", "mrca.train", "--stage", "1", "--worlds", "8", "--robots-per-world", "24",
                        "--fused-bf16-update", "--fused-bf16-inference", "--updates", "2", "--save-every", "1", "--horizon", "32",
                        "--policy-dir", str(pdir)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = r.stdout + r.stderr
    for f in os.listdir(tmp_path):
        if f.endswith(".log"):
            text += open(tmp_path / f).read()
    assert "update precision: bf16" in text, text[-3000:]
    logs = [f for _d, _s, fs in os.walk(tmp_path / "log") for f in fs]
    assert sorted(logs) == ["cal.log", "output.log", "ppo.log"], logs           # the three log streams, unchanged
    saved = sorted(f for f in os.listdir(pdir) if not f.endswith(".state"))
    assert saved, os.listdir(pdir)
    from mrca.net import CNNPolicy
    sd = torch.load(os.path.join(pdir, saved[-1]), map_location="cpu")
    assert set(sd.keys()) == set(CNNPolicy(3, 2).state_dict().keys())
    assert all(v.dtype == torch.float32 for v in sd.values())
    r = subprocess.run([sys.executable, "-m", "mrca.evaluate", "--circles", "1", "--policy", os.path.join(pdir, saved[-1]),
                        "--max-ticks", "50"], cwd=U.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
