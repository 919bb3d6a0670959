"""The rollout inference -- what ``CNNPolicy.act_fused`` computes: the conv front end of both towers, fc1, and everything behind
it down to the sampled action, its log-probability and the clip -- as plain float64 on the CPU (tests only): the model
tests/test_gpu_rollout_inference.py holds the HIP kernels (csrc/mrca_policy.hip, mrca_policy_bf16.hip, mrca_policy_tail.hip) to.

Nothing of the code under test is in here (no ``mrca.net``, ``mrca.ppo``, ``mrca.policy_ops``): the towers, the heads and the log density
are ``update_ref._tower`` / ``forward`` / ``log_density``, which tests/test_update_ref_host.py grounds in the reference's own run;
tests/test_inference_ref_host.py grounds what is added here.

``deque_obs``      the env's frame ring -> the observation stacks in deque order (fp32: it restates a bit-exact contract)
``features``       relu(conv2(relu(conv1(obs)))) of both towers, f64[2, n, 4096]
``tail``           everything behind fc1, from h1 and the parameters in the rollout cache's layouts
``act``            the chain, from a state dict
``tail_kernel_order``  fc2 and the heads in fp32 in the kernel's own summation order, on the host: what shows that a distance is the
                   order's and nothing else's
``exact_case``     inputs on which fp32 arithmetic is EXACT in any summation order: a kernel must then equal the model to the bit

What the model does not say: the kernels' ReLU sends a NaN to 0 where ``torch.relu`` keeps it (noted in csrc/mrca_policy.hip); the
layers produce none from finite inputs, and no test feeds one."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import update_ref as M

TOWERS = ("act", "crt")

Tail = namedtuple("Tail", "value mean action logprob scaled")


def _f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().clone()
    return torch.from_numpy(np.array(x, dtype=np.float64))


def _np32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the frame ring
def normalize(raw):
    """|x| / 6 - 0.5 in fp32 with the correctly rounded quotient (numpy's): the contract ``policy_ops.normalize_scans`` documents
    and the env's own observation view keeps (stage_world1.py:140)."""
    a = np.abs(_np32(raw))
    return a / np.float32(6.0) - np.float32(0.5)


def deque_obs(ring, slots, raw):
    """ring f32[n, 3, 512] used as a ring, slots[n] the slot of robot n's NEWEST frame -> f32[n, 3, 512] in deque order (oldest
    first): frame f of robot n is slot (slots[n] + 1 + f) % 3.  ``raw``: the ring holds raw ranges, normalised on the way."""
    ring = _np32(ring)
    slots = np.asarray(slots.detach().cpu().numpy() if isinstance(slots, torch.Tensor) else slots).astype(np.int64)
    n = ring.shape[0]
    assert ring.shape[1] == 3 and slots.shape == (n,) and slots.min() >= 0 and slots.max() <= 2
    order = (slots[:, None] + 1 + np.arange(3)[None, :]) % 3
    out = ring[np.arange(n)[:, None], order]
    return normalize(out) if raw else np.ascontiguousarray(out)


def ring_of(deque, slots):
    """The inverse of ``deque_obs`` (raw=False): stacks in deque order -> the ring whose newest slots are ``slots``."""
    deque = _np32(deque)
    slots = np.asarray(slots).astype(np.int64)
    n = deque.shape[0]
    ring = np.empty_like(deque)
    order = (slots[:, None] + 1 + np.arange(3)[None, :]) % 3
    ring[np.arange(n)[:, None], order] = deque
    return ring


# ------------------------------------------------------------------------------------------------ the model
def conv_params(sd):
    """A state dict -> the front end's parameters tower-major, float64: w1 [2,32,3,5], b1 [2,32], w2 [2,32,32,3], b2 [2,32]."""
    st = lambda k: torch.stack([_f64(sd[f"{tw}_fea_{k}"]) for tw in TOWERS])           # noqa: E731
    return st("cv1.weight"), st("cv1.bias"), st("cv2.weight"), st("cv2.bias")


def features_of(w1, b1, w2, b2, obs, pre=False):
    """relu(conv2(relu(conv1(obs)))) of both towers (model/net.py:42-44, 61-63) from tower-major parameters, in the dtype of
    ``obs`` -> [2, n, 4096] (rows in the flatten order of [32, 128]).  ``pre``: also the two layers' pre-activations."""
    out, pres = [], []
    for t in range(2):
        z1 = F.conv1d(obs, w1[t], b1[t], stride=2, padding=1)
        z2 = F.conv1d(F.relu(z1), w2[t], b2[t], stride=2, padding=1)
        out.append(F.relu(z2).reshape(obs.shape[0], -1))
        pres.append((z1, z2))
    return (torch.stack(out), pres) if pre else torch.stack(out)


def features(sd, obs):
    """-> f64[2, n, 4096] (numpy)"""
    with torch.no_grad():
        return features_of(*conv_params(sd), _f64(obs)).numpy()


def tail_params(sd):
    """A state dict -> what ``tail`` takes, in the layouts of ``CNNPolicy.refresh_rollout_cache`` (float64): fc1_w [2,4096,256],
    fc1_b [2,1,256], fc2_w [2,260,128], fc2_b [2,1,128], head_w [128,2], head_b [2], critic_w [128], critic_b [1], logstd [2]."""
    st = lambda k, f=lambda x: x: torch.stack([f(_f64(sd[f"{tw}_{k}"])) for tw in TOWERS])           # noqa: E731
    return {"fc1_w": st("fc1.weight", lambda x: x.t()), "fc1_b": st("fc1.bias").unsqueeze(1),
            "fc2_w": st("fc2.weight", lambda x: x.t()), "fc2_b": st("fc2.bias").unsqueeze(1),
            "head_w": torch.cat([_f64(sd["actor1.weight"]), _f64(sd["actor2.weight"])]).t().contiguous(),
            "head_b": torch.cat([_f64(sd["actor1.bias"]), _f64(sd["actor2.bias"])]),
            "critic_w": _f64(sd["critic.weight"]).reshape(-1), "critic_b": _f64(sd["critic.bias"]).reshape(1),
            "logstd": _f64(sd["logstd"]).reshape(-1)}


def tail(h1, fc1_b, goal, speed, fc2_w, fc2_b, head_w, head_b, critic_w, critic_b, logstd, noise, lo, hi, at=None):
    """Everything behind fc1 (model/net.py:45-51, 64-67; model/ppo.py:73-82), float64.  ``h1`` [2, n, 256]: fc1's outputs before
    the ReLU, with their bias or -- ``fc1_b`` given, 512 elements -- without it; the fc2 / head / critic parameters in the cache's
    layouts (``tail_params``); ``noise`` [n, 2] standard normal draws or None (the mean action); ``lo``, ``hi`` the clip bounds.
    ``at`` = (action, mean), fp32 as a kernel returned them: the log density is evaluated THERE, in float64 -- what is measured is
    a kernel's arithmetic, not the rounding of its sample; None: at the model's own action and mean.
    -> Tail(value [n,1], mean [n,2], action [n,2], logprob [n,1], scaled [n,2]), numpy float64"""
    with torch.no_grad():
        h = _f64(h1)
        n = h.shape[1]
        if fc1_b is not None:
            h = h + _f64(fc1_b).reshape(2, 1, 256)
        gs = torch.cat((_f64(goal), _f64(speed)), dim=-1)                                   # the cat order of model/net.py:45
        z = [F.relu(torch.cat((F.relu(h[t]), gs), dim=-1) @ _f64(fc2_w)[t] + _f64(fc2_b).reshape(2, 128)[t]) for t in range(2)]
        m = z[0] @ _f64(head_w) + _f64(head_b)
        mean = torch.stack((torch.sigmoid(m[:, 0]), torch.tanh(m[:, 1])), dim=-1)
        value = (z[1] @ _f64(critic_w).reshape(128, 1)) + _f64(critic_b)
        ls = _f64(logstd).reshape(1, 2).expand(n, 2)
        action = mean if noise is None else mean + torch.exp(ls) * _f64(noise)
        a_at, m_at = (action, mean) if at is None else (_f64(at[0]), _f64(at[1]))
        logprob = M.log_density(a_at, m_at, ls)
        scaled = torch.minimum(torch.maximum(action, _f64(lo)), _f64(hi))
        return Tail(*(x.numpy() for x in (value, mean, action, logprob, scaled)))


def fc1(sd, feat):
    """feat f64[2, n, 4096] -> h1 f64[2, n, 256], before bias and ReLU"""
    return torch.bmm(_f64(feat), tail_params(sd)["fc1_w"]).numpy()


def act(sd, obs, goal, speed, noise, lo, hi, at=None):
    """The chain ``CNNPolicy.act_fused`` runs (features -> fc1 -> tail) -> Tail"""
    p = tail_params(sd)
    h1 = torch.bmm(_f64(features(sd, obs)), p["fc1_w"])
    return tail(h1, p["fc1_b"], goal, speed, p["fc2_w"], p["fc2_b"], p["head_w"], p["head_b"], p["critic_w"], p["critic_b"],
                p["logstd"], noise, lo, hi, at=at)


def act_by_forward(sd, obs, goal, speed):
    """(mean, value) by ``update_ref.forward``: what the chain above must equal (tests/test_inference_ref_host.py)."""
    p = {k: _f64(sd[k]) for k in M.ORDER}
    with torch.no_grad():
        mean, value = M.forward(p, _f64(obs), _f64(goal), _f64(speed))
    return mean.numpy(), value.numpy()


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in float64; the sum is rounded to float64 and then to fp32
    (a double rounding that differs from fmaf only where the float64 sum lands within 2^-29 of an fp32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def tail_kernel_order(h1, fc1_b, goal, speed, fc2_w, fc2_b, head_w, head_b, critic_w, critic_b):
    """fc2 and the three heads in fp32 in the summation order of csrc/mrca_policy_tail.hip, on the host: fc1's bias added to the
    stored fp32 h1, ReLU; fc2 as ONE fmaf chain per (robot, unit) over k = 0 .. 259 ascending from 0 (v_mfma_f32_32x32x2_f32 with
    A[unit][k = 2 s + hl]: a k-ordered fmaf chain); the bias added behind it, ReLU; a head's dot product as the kernel deals it
    out -- per wave q and half hl the 16 units 32 q + rowmap(r, hl) in register order, product and sum rounded apart
    (-ffp-contract=off), the two halves added, the four waves added in order from 0, the head's bias last.
    -> (value f32[n, 1], head pre-activations f32[n, 2]: what the kernel hands to its sigmoid and its tanh)"""
    h = _np32(h1)
    n = h.shape[1]
    if fc1_b is not None:
        h = h + _np32(fc1_b).reshape(2, 1, 256)
    gs = np.concatenate([_np32(goal), _np32(speed)], 1)
    x = np.concatenate([np.maximum(h, np.float32(0)), np.broadcast_to(gs, (2, n, 4))], 2)
    W, b = _np32(fc2_w), _np32(fc2_b).reshape(2, 1, 128)
    acc = np.zeros((2, n, 128), np.float32)
    for k in range(260):
        acc = _fma32(x[:, :, k, None], W[:, None, k, :], acc)
    z = np.maximum(acc + b, np.float32(0))

    def head(zt, w):
        d = np.zeros(n, np.float32)
        for q in range(4):
            halves = []
            for hl in range(2):
                p = np.zeros(n, np.float32)
                for r in range(16):
                    u = 32 * q + (r & 3) + 8 * (r >> 2) + 4 * hl
                    p = p + zt[:, u] * w[u]
                halves.append(p)
            d = d + (halves[0] + halves[1])
        return d
    hw, cw = _np32(head_w), _np32(critic_w).reshape(128)
    pre = np.stack([head(z[0], hw[:, 0]), head(z[0], hw[:, 1])], 1) + _np32(head_b).reshape(1, 2)
    value = (head(z[1], cw) + _np32(critic_b).reshape(1)[0])[:, None]
    assert value.dtype == np.float32 and pre.dtype == np.float32
    return value, pre


def squash(pre):
    """head pre-activations [n, 2] -> [sigmoid, tanh] in float64"""
    pre = np.asarray(pre, np.float64)
    with np.errstate(over="ignore"):
        return np.stack([1.0 / (1.0 + np.exp(-pre[:, 0])), np.tanh(pre[:, 1])], 1)


def distance(got, want):
    """E: max |got - model| / max(1, max |model|)"""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


# ------------------------------------------------------------------------------------------------ exact inputs
def _eighths(rng, lo, hi, shape):
    """multiples of 1/8 in [lo / 8, hi / 8]"""
    return (rng.integers(lo, hi + 1, shape) / 8.0).astype(np.float32)


def _sparse(rng, shape, per_column, values):
    """A matrix [rows, columns] with ``per_column`` non-zeros in every column, drawn from ``values``."""
    w = np.zeros(shape, np.float32)
    for c in range(shape[1]):
        rows = rng.choice(shape[0], per_column, replace=False)
        w[rows, c] = rng.choice(values, per_column)
    return w


def exact_case(seed, n):
    """Inputs on which every sum either kernel forms is a sum of multiples of one power of two that stays far below 2^24 units:
    fp32 is exact at every step in ANY order, and so is an MFMA chain -- the result is the float64 result to the bit.  The
    parameters depend on ``seed`` alone, the per-robot data on ``seed`` and ``n``.

    Front end: observations k / 8 with k in -4 .. 4 -- as raw ranges 0.75 k + 3 in [0, 6], whose quotient by 6 is exact (``ring``
    holds them as a ring with per-robot ``slots``; the ranges 0.0 are written -0.0 for every other robot); w1, w2 integers in
    -2 .. 2; b1, b2 multiples of 1/8 in [-1, 1].  In units of 1/8: |conv1| <= 15 * 2 * 4 + 8 = 128, |conv2| <= 96 * 2 * 128 + 8.
    The weights are symmetric around 0, so about half of the pre-activations are <= 0, exact zeros among them.

    The tail's twin: h1, fc1_b, goal, speed multiples of 1/8 (|h1| <= 1.5, |fc1_b| <= 0.5, |goal| <= 2, speed in [0, 1]); fc2_w
    with six entries of +-1 per unit; fc2_b multiples of 1/8 in [-0.5, 0.5]: |fc2| <= 6 * 2 + 0.5 = 12.5.  The two heads have four
    weights of +-1/8 each and biases in [-1, 1]: products in units of 1/64, |pre-activation| <= 4 * 12.5 / 8 + 1 = 7.25 < 8, no
    head saturated.  The critic has eight weights that are multiples of 1/8 in [-1/2, 1/2]: the value is exact too.

    -> a namespace: w1 b1 w2 b2 (tower-major fp32 numpy), obs (deque order, normalised), raw (deque order, raw ranges), slots,
    ring (raw, ring order), and ``tail``: a dict of ``tail``'s arguments (fp32 numpy; noise None)."""
    rng = np.random.default_rng(seed)
    c = SimpleNamespace()
    c.w1 = rng.integers(-2, 3, (2, 32, 3, 5)).astype(np.float32)
    c.b1 = _eighths(rng, -8, 8, (2, 32))
    c.w2 = rng.integers(-2, 3, (2, 32, 32, 3)).astype(np.float32)
    c.b2 = _eighths(rng, -8, 8, (2, 32))
    t = {"fc1_b": _eighths(rng, -4, 4, (2, 1, 256)),
         "fc2_w": np.stack([_sparse(rng, (260, 128), 6, np.array([-1.0, 1.0], np.float32)) for _ in range(2)]),
         "fc2_b": _eighths(rng, -4, 4, (2, 1, 128)),
         "head_w": _sparse(rng, (128, 2), 4, np.array([-0.125, 0.125], np.float32)),
         "head_b": _eighths(rng, -8, 8, (2,)),
         "critic_w": _sparse(rng, (128, 1), 8, np.array([-0.5, -0.375, -0.25, -0.125, 0.125, 0.25, 0.375, 0.5], np.float32)).reshape(128),
         "critic_b": _eighths(rng, -8, 8, (1,)),
         "logstd": np.zeros(2, np.float32), "noise": None,
         "lo": np.array([0.0, -1.0], np.float32), "hi": np.array([1.0, 1.0], np.float32)}
    rng = np.random.default_rng([seed, n])
    k = rng.integers(-4, 5, (n, 3, 512))
    c.obs = (k / 8.0).astype(np.float32)
    c.raw = (0.75 * k + 3.0).astype(np.float32)
    c.raw[1::2][c.raw[1::2] == 0.0] = -0.0
    c.slots = rng.integers(0, 3, n).astype(np.uint8)
    c.ring = ring_of(c.raw, c.slots)
    t.update(h1=_eighths(rng, -12, 12, (2, n, 256)), goal=_eighths(rng, -16, 16, (n, 2)), speed=_eighths(rng, 0, 8, (n, 2)))
    c.tail = t
    return c


# the exact cases the GPU tests use (tests/test_inference_ref_host.py asserts the exactness conditions for these): the front end
# at EXACT_SEED and the device's n (3 x 2 x CUs + 5; the host file takes 256 CUs and the GPU file re-asserts the cheap
# conditions at its own n), the tail at EXACT_SEED and every n of TAIL_NS
EXACT_SEED = 7
TAIL_NS = (1, 31, 32, 33, 64, 65)          # the tail's tile is 32 robots; rows past the batch are clamped loads

TAIL_ARGS = ("h1", "fc1_b", "goal", "speed", "fc2_w", "fc2_b", "head_w", "head_b", "critic_w", "critic_b", "logstd", "noise", "lo", "hi")


def tail_args(t):
    """``tail``'s positional arguments out of a dict of them"""
    return [t[k] for k in TAIL_ARGS]


def exact_front_end(c, robots=None):
    """For the exact case ``c`` (its robots ``robots``, default all): -> (feat f64[2, m, 4096], units, worst) with ``units`` the
    largest sum of ABSOLUTE products (bias included) any output of either layer has, in units of 1/8, and ``worst`` the largest
    |8 x pre-activation - its nearest integer| (0.0 when every pre-activation is a multiple of 1/8)."""
    obs = _f64(c.obs if robots is None else c.obs[robots])
    w1, b1, w2, b2 = (_f64(x) for x in (c.w1, c.b1, c.w2, c.b2))
    with torch.no_grad():
        feat, pres = features_of(w1, b1, w2, b2, obs, pre=True)
        units, worst = 0.0, 0.0
        for t in range(2):
            z1, z2 = pres[t]
            a1 = F.conv1d(obs.abs(), w1[t].abs(), b1[t].abs(), stride=2, padding=1)
            a2 = F.conv1d(F.relu(z1), w2[t].abs(), b2[t].abs(), stride=2, padding=1)
            units = max(units, float(a1.max()) * 8, float(a2.max()) * 8)
            worst = max(worst, *(float((8 * z - torch.round(8 * z)).abs().max()) for z in (z1, z2)))
    return feat.numpy(), units, worst
