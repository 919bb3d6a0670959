"""Host: what tests/inference_ref.py adds to tests/update_ref.py is grounded here, before tests/test_gpu_rollout_inference.py
holds the HIP kernels to it.

(a) the model's chain (features -> fc1 -> tail, the parameters in the rollout cache's layouts) against ``CNNPolicy(...).double()``
on the CPU (1e-12) and against the reference's own forward (tests/golden/net.npz: 1e-5, fp32 on the reference's side -- the bars
of tests/test_golden_learner.py); (b) ``deque_obs`` against a three-robot case written out by hand, one robot per head; (c) for
every ``exact_case`` the GPU file uses, the conditions that entitle it to bit equality: every pre-activation a multiple of the
unit, the sum of ABSOLUTE products far below 2^24 units, and an fp32 evaluation in REVERSED summation order equal to the float64
result to the bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inference_ref as I
import update_ref as M
import util as U

GOLD = os.path.join(U.ROOT, "tests", "golden")
f32 = np.float32


# ---------------------------------------------------------------------------------------------- (a)
def _golden_policy():
    from test_golden_learner import _policy
    pol, g, _keys, _shapes, sd = _policy()
    return pol, g, sd


def test_the_chain_equals_the_double_policy_and_the_reference_forward():
    pol, g, sd = _golden_policy()
    x, goal, speed = g["x"], g["goal"], g["speed"]
    rng = np.random.default_rng(0)
    noise = rng.standard_normal((x.shape[0], 2))
    lo, hi = np.array([0.0, -1.0]), np.array([1.0, 1.0])
    got = I.act(sd, x, goal, speed, noise, lo, hi)
    # ... the reference's own run (fp32 there)
    assert np.abs(got.mean - g["mean"]).max() < 1e-5 and np.abs(got.value - g["value"]).max() < 1e-5
    # ... the module in float64
    pd = pol.double()
    from mrca.net import gaussian_logprob
    with torch.no_grad():
        mean, value = pd.mean_value(*(torch.from_numpy(np.asarray(a, np.float64)) for a in (x, goal, speed)))
        action = mean + torch.exp(pd.logstd.expand_as(mean)) * torch.from_numpy(noise)
        logprob = gaussian_logprob(action, mean, pd.logstd.expand_as(mean))
        scaled = torch.minimum(torch.maximum(action, torch.from_numpy(lo)), torch.from_numpy(hi))
    for name, a, b in (("mean", got.mean, mean), ("value", got.value, value), ("action", got.action, action),
                       ("logprob", got.logprob, logprob), ("scaled", got.scaled, scaled)):
        assert a.shape == tuple(b.shape) and np.abs(a - b.numpy()).max() < 1e-12, name
    assert (got.scaled != got.action).any()            # (the clip does something on these draws)
    # ... update_ref.forward, which test_update_ref_host.py grounds in the reference's update
    m2, v2 = I.act_by_forward(sd, x, goal, speed)
    assert np.abs(got.mean - m2).max() < 1e-12 and np.abs(got.value - v2).max() < 1e-12
    # noise=None: the mean action; ``at``: the density evaluated where the caller says
    det = I.act(sd, x, goal, speed, None, lo, hi)
    assert np.array_equal(det.action, det.mean) and np.array_equal(det.mean, got.mean)
    assert np.allclose(det.logprob, -2 * M._HALF_LOG_2PI - np.asarray(sd["logstd"], np.float64).sum(), atol=1e-12)
    a32, m32 = got.action.astype(f32), got.mean.astype(f32)
    at = I.act(sd, x, goal, speed, noise, lo, hi, at=(a32, m32))
    ls = torch.from_numpy(np.asarray(sd["logstd"], np.float64)).expand(x.shape[0], 2)
    want = M.log_density(torch.from_numpy(a32.astype(np.float64)), torch.from_numpy(m32.astype(np.float64)), ls).numpy()
    assert np.array_equal(at.logprob, want) and np.array_equal(at.action, got.action)


def test_features_are_the_towers_conv_stack():
    pol, g, sd = _golden_policy()
    pd = pol.double()
    x = torch.from_numpy(np.asarray(g["x"], np.float64))
    feat = I.features(sd, x)
    assert feat.shape == (2, x.shape[0], 4096) and feat.dtype == np.float64
    with torch.no_grad():
        for t, tw in enumerate(I.TOWERS):
            h = torch.relu(getattr(pd, f"{tw}_fea_cv2")(torch.relu(getattr(pd, f"{tw}_fea_cv1")(x)))).flatten(1)
            assert np.abs(feat[t] - h.numpy()).max() < 1e-12 and float(h.abs().max()) > 0.01
    h1 = I.fc1(sd, feat)
    with torch.no_grad():
        want = F.linear(torch.from_numpy(feat[1]), pd.crt_fc1.weight)
    assert np.abs(h1[1] - want.numpy()).max() < 1e-12


# ---------------------------------------------------------------------------------------------- (b)
def test_deque_obs_on_three_robots_written_out_by_hand():
    """Robot r has head r.  Slot s of robot r holds the constant 10 r + s (beam b adds b / 1024).  With head h the newest frame is
    slot h, the one before it slot h - 1, the oldest slot h + 1 (mod 3)."""
    ring = np.zeros((3, 3, 512), f32)
    for r in range(3):
        for s in range(3):
            ring[r, s] = 10 * r + s + np.arange(512, dtype=f32) / 1024
    slots = np.array([0, 1, 2], np.uint8)
    got = I.deque_obs(ring, slots, raw=False)
    want_slots = [[1, 2, 0],        # head 0: oldest 1, then 2, newest 0
                  [2, 0, 1],        # head 1
                  [0, 1, 2]]        # head 2: the identity
    for r in range(3):
        for f in range(3):
            assert np.array_equal(got[r, f], ring[r, want_slots[r][f]]), (r, f)
            assert got[r, f, 0] == 10 * r + want_slots[r][f]
    assert np.array_equal(I.ring_of(got, slots), ring)
    assert np.array_equal(I.deque_obs(torch.from_numpy(ring), torch.from_numpy(slots), raw=False), got)
    # raw: |x| / 6 - 0.5, the quotient correctly rounded
    raw = np.array([0.0, -0.0, 6.0, 3.0, 1.0, 5.9999995, 0.1, -2.5], f32)
    ring[:] = 0.0
    ring[1, 2, :8] = raw
    out = I.deque_obs(ring, slots, raw=True)
    want = (np.abs(raw.astype(np.float64)) / 6.0).astype(f32) - f32(0.5)        # f64 quotient rounded once = the correctly rounded quotient
    assert np.array_equal(out[1, 0, :8], want) and out[1, 0, 0] == -0.5 and out[1, 0, 1] == -0.5 and out[1, 0, 2] == 0.5
    assert out[1, 0, 7] == want[7] > -0.5 and (out[1, 1:] == -0.5).all()


# ---------------------------------------------------------------------------------------------- (c)
def _conv_reversed_fp32(x, w, b, taps, pad_to):
    """relu'd input x f32[m, C, L] -> the pre-activation of Conv1d(C, 32, taps, stride 2, padding 1) in fp32, every product and
    every partial sum rounded on its own (numpy), the bias LAST and k = (ci, tap) DESCENDING: the reverse of the natural order."""
    m, C, L = x.shape
    xp = np.zeros((m, C, L + 2), f32)
    xp[:, :, 1:L + 1] = x
    acc = np.zeros((m, 32, pad_to), f32)
    for ci in reversed(range(C)):
        for tap in reversed(range(taps)):
            col = xp[:, ci, tap: tap + 2 * pad_to: 2][:, None, :]            # x[ci][2 l + tap - 1]
            acc = acc + w[None, :, ci, tap, None] * col
    return acc + b[None, :, None]


def test_exact_front_end_is_entitled_to_bit_equality():
    n = 3 * 2 * 256 + 5
    c = I.exact_case(I.EXACT_SEED, n)
    assert c.obs.shape == (n, 3, 512) and set(np.unique(c.obs * 8).tolist()) == set(range(-4, 5))
    assert c.raw.min() == 0.0 and c.raw.max() == 6.0 and np.signbit(c.raw).any() and (c.raw[~np.signbit(c.raw)] == 0.0).any()
    assert set(c.slots.tolist()) == {0, 1, 2}
    # the ring form and the deque form are the same observations, and normalising the raw ranges is exact
    assert np.array_equal(I.deque_obs(c.ring, c.slots, raw=True), c.obs) and np.array_equal(I.deque_obs(c.ring, c.slots, raw=False), c.raw)
    # same parameters whatever n
    c2 = I.exact_case(I.EXACT_SEED, 9)
    assert all(np.array_equal(getattr(c, k), getattr(c2, k)) for k in ("w1", "b1", "w2", "b2")) and c2.obs.shape[0] == 9
    assert np.array_equal(c.w1, np.round(c.w1)) and np.abs(c.w1).max() == 2 and np.array_equal(c.b2 * 8, np.round(c.b2 * 8))
    # every robot: multiples of 1/8, absolute sums far below 2^24 units
    feat, units, worst = I.exact_front_end(c)
    print(f"exact front end, n = {n}: largest sum of absolute products {units:.0f} units of 1/8; largest feature {feat.max():.3f}")
    assert worst == 0.0 and units < 2 ** 24 and np.array_equal(feat * 8, np.round(feat * 8))
    assert np.array_equal(feat, feat.astype(f32).astype(np.float64))
    # about half of the pre-activations <= 0, exact zeros among them; fp32 conv1d equals float64 to the bit
    sub = np.r_[0:4, n - 3:n]
    w = [torch.from_numpy(a) for a in (c.w1, c.b1, c.w2, c.b2)]
    with torch.no_grad():
        f32feat, pres = I.features_of(*w, torch.from_numpy(c.obs[sub]), pre=True)
    assert np.array_equal(f32feat.numpy().astype(np.float64), feat[:, sub])
    for z1, z2 in pres:
        for z in (z1, z2):
            share = float((z <= 0).float().mean())
            assert 0.35 < share < 0.65 and int((z == 0).sum()) > 0, share
    # an fp32 evaluation in reversed order
    for t in range(2):
        z1 = _conv_reversed_fp32(c.obs[sub], c.w1[t], c.b1[t], 5, 255)
        z2 = _conv_reversed_fp32(np.maximum(z1, f32(0)), c.w2[t], c.b2[t], 3, 128)
        assert z1.dtype == f32 and z2.dtype == f32
        assert np.array_equal(np.maximum(z2, f32(0)).reshape(len(sub), -1).astype(np.float64), feat[t, sub]), t


def _tail_by_hand(t, dtype, reverse):
    """The exact tail, written out: every product and partial sum rounded on its own in ``dtype``; ``reverse``: k descending,
    the bias last.  -> (head pre-activations [n, 2], value [n, 1], fc2 outputs [2, n, 128], largest sum of absolute products
    in units of 1/64)"""
    h1, fc1_b = t["h1"].astype(dtype), t["fc1_b"].astype(dtype)
    n = h1.shape[1]
    x = np.concatenate([np.maximum(h1 + fc1_b.reshape(2, 1, 256), 0), np.broadcast_to(np.concatenate([t["goal"], t["speed"]], 1).astype(dtype), (2, n, 4))], 2)
    W, b = t["fc2_w"].astype(dtype), t["fc2_b"].astype(dtype).reshape(2, 1, 128)
    ks = lambda m: reversed(range(m)) if reverse else range(m)          # noqa: E731
    acc = np.zeros((2, n, 128), dtype) if reverse else np.broadcast_to(b, (2, n, 128)).copy()
    mass = np.abs(b) * np.ones((2, n, 1), dtype)
    for k in ks(260):
        acc = acc + x[:, :, k, None] * W[:, None, k, :]
        mass = mass + np.abs(x[:, :, k, None] * W[:, None, k, :])
    z = np.maximum(acc + b if reverse else acc, 0)
    hw, cw = t["head_w"].astype(dtype), t["critic_w"].astype(dtype)
    m = np.zeros((n, 2), dtype)
    v = np.zeros((n, 1), dtype)
    hm = np.zeros((n, 2), dtype)
    vm = np.zeros((n, 1), dtype)
    for u in ks(128):
        m = m + z[0][:, u, None] * hw[None, u, :]
        v = v + z[1][:, u, None] * cw[u]
        hm = hm + np.abs(z[0][:, u, None] * hw[None, u, :])
        vm = vm + np.abs(z[1][:, u, None] * cw[u])
    m, v = m + t["head_b"].astype(dtype)[None, :], v + t["critic_b"].astype(dtype)
    units = 64 * max(float(mass.max()), float(hm.max()) + 1, float(vm.max()) + 1)
    return m, v, z, units


@pytest.mark.parametrize("n", I.TAIL_NS)
def test_exact_tail_is_entitled_to_bit_equality(n):
    t = I.exact_case(I.EXACT_SEED, n).tail
    m64, v64, z64, units = _tail_by_hand(t, np.float64, False)
    m32, v32, z32, _u = _tail_by_hand(t, f32, True)
    assert m32.dtype == f32 and v32.dtype == f32
    print(f"exact tail, n = {n}: largest sum of absolute products {units:.0f} units of 1/64, head pre-activations within "
          f"{np.abs(m64).max():.3f}, fc2 within {np.abs(z64).max():.3f}")
    assert units < 2 ** 24
    for a in (m64, v64, z64 * 8):
        assert np.array_equal(a * 64, np.round(a * 64))
    assert np.abs(m64).max() <= 8.0 and np.abs(z64).max() <= 12.5
    assert np.array_equal(m32.astype(np.float64), m64) and np.array_equal(v32.astype(np.float64), v64)
    assert 0.3 < float((z64 == 0).mean()) < 0.7            # (about half of fc2's units are cut by the ReLU)
    got = I.tail(*I.tail_args(t))
    assert np.array_equal(got.value, v64)
    want = np.stack([1 / (1 + np.exp(-m64[:, 0])), np.tanh(m64[:, 1])], 1)
    assert np.abs(got.mean - want).max() < 1e-15 and np.array_equal(got.action, got.mean)
    assert 3e-4 < got.mean[:, 0].min() and got.mean[:, 0].max() < 1 - 3e-4 and np.abs(got.mean[:, 1]).max() < 1 - 2e-7


@pytest.mark.parametrize("n", [1, 33])
def test_tail_in_the_kernels_order_is_the_same_function(n):
    """``tail_kernel_order``: on the exact case it IS the model (every unit and every k taken once, whatever the order); on random
    inputs it is the model up to fp32 rounding."""
    t = I.exact_case(I.EXACT_SEED, n).tail
    names = ("h1", "fc1_b", "goal", "speed", "fc2_w", "fc2_b", "head_w", "head_b", "critic_w", "critic_b")
    value, pre = I.tail_kernel_order(*(t[k] for k in names))
    want = I.tail(*I.tail_args(t))
    assert np.array_equal(value.astype(np.float64), want.value) and np.abs(I.squash(pre) - want.mean).max() < 1e-15
    rng = np.random.default_rng(n)
    r = dict(t, h1=rng.standard_normal((2, n, 256)).astype(f32) * 30, goal=(rng.random((n, 2)) * 40 - 20).astype(f32),
             fc2_w=(rng.standard_normal((2, 260, 128)) * 0.06).astype(f32), head_w=(rng.standard_normal((128, 2)) * 0.09).astype(f32),
             critic_w=(rng.standard_normal(128) * 0.09).astype(f32))
    value, pre = I.tail_kernel_order(*(r[k] for k in names))
    want = I.tail(*I.tail_args(r))
    # (fc2 outputs of size ~100 cancel in the heads: a few 1e-6 absolute)
    assert 0 < I.distance(value, want.value) < 1e-4 and 0 < I.distance(I.squash(pre), want.mean) < 1e-4
    no_bias = I.tail_kernel_order(r["h1"] + r["fc1_b"], None, *(r[k] for k in names[2:]))
    assert np.array_equal(no_bias[0], value) and np.array_equal(no_bias[1], pre)
    assert np.array_equal(I.squash(np.array([[-1000.0, 1000.0], [1000.0, -1000.0]])), np.array([[0.0, 1.0], [1.0, -1.0]]))
