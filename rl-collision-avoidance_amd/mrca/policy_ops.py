"""HIP ops of the policy's lidar front end (csrc/mrca_policy.hip, csrc/mrca_policy_bwd.hip through the C ABI): the
fused forward of both towers' Conv1d + ReLU pairs (rollout AND update) and its backward pass, tied together as a
``torch.autograd.Function`` (``lidar_features_fn``) so that the PPO update (model/ppo.py:158-192) differentiates through
hand-written fp32 MFMA kernels instead of MIOpen.  The rest of the policy stays stock PyTorch.
The opt-in fused bf16 update is the same function at the other precision (``lidar_features_bf16_fn``; csrc/mrca_policy_bf16_rows.hip
and csrc/mrca_policy_bf16_bwd.hip) with an fc1 of its own (``fc1_bf16``).  There is no fallback: without the HIP library these
raise."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _check(who, dtype, *expected, device=None):
    """Raise a ``ValueError`` in ``who``'s name unless every ``(tensor, shape)`` of ``expected`` is a contiguous CUDA tensor of
    ``dtype`` and of that shape -- an int: of that many elements, whatever their shape -- on ``device`` where one is given."""
    for t, shape in expected:
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and (device is None or t.device == device) and
                (t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == shape)):
            raise ValueError(f"{who}: expected a contiguous cuda {dtype} tensor of shape {shape}"
                             f"{'' if device is None else f' on {device}'}, got {tuple(t.shape)} {t.dtype} {t.device}")


class _stream_on(torch.cuda.device):
    """``with _stream_on(device) as stream``: selects ``device`` as ``torch.cuda.device`` does and hands out its current stream
    as the ``c_void_p`` the library's entry points take.  (A class, not a generator: this runs twice per eager rollout tick.)"""

    def __init__(self, device):
        super().__init__(device)
        self.device = device

    def __enter__(self):
        super().__enter__()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


# The ops that keep partial results between two launches: display name -> (the library's size query, buffer starts zeroed).
# The loss kernel's buffer holds a ticket, which its first launch expects at zero; the others are written before they are read.
_SCRATCH_OPS = {
    "lidar_features_backward": ("mrca_lidar_features_backward_scratch", False),
    "lidar_features_bf16_backward": ("mrca_lidar_features_bf16_backward_scratch", False),
    "ppo_loss": ("mrca_ppo_loss_scratch", True),
    "policy_heads backward": ("mrca_policy_heads_backward_scratch", False),
    "relu_cat backward": ("mrca_relu_cat_backward_bias_scratch", False),
}
_scratch = {}


def _scratch_of(op, device, stream):
    """``op``'s scratch bytes, one buffer per (op, device, STREAM): the partial sums (and the loss kernel's ticket) live between
    a kernel and its finalize launch on one stream, and two trainers, rank threads or side streams of one process must not
    overwrite each other's.  Allocated outside any graph capture: a buffer first created inside a capture would live in that
    graph's private pool."""
    key = (op, device.type, device.index, stream.value or 0)
    if key not in _scratch:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{op}: first use on this stream inside a graph capture -- call it once before capturing")
        size_fn, zeroed = _SCRATCH_OPS[op]
        n = C.c_size_t()
        with torch.cuda.device(device):
            _lib.check(getattr(_lib.load(), size_fn)(C.byref(n)), size_fn)
        _scratch[key] = (torch.zeros if zeroed else torch.empty)(n.value, dtype=torch.uint8, device=device)
    return _scratch[key]


class RingHead:
    """The head slots of a frame ring plus what the ring holds: ``raw`` = raw lidar ranges (the env's MRCA_F_SCAN_RING;
    the front end applies x / 6 - 0.5 while it stages) or normalised observations.  Travels opaquely through
    ppo.generate_action / CNNPolicy.act_fused as their ``head`` argument; a plain u8 tensor means "normalised"."""
    __slots__ = ("slots", "raw")

    def __init__(self, slots, raw):
        self.slots, self.raw = slots, bool(raw)

    def __getitem__(self, idx):
        return RingHead(self.slots[idx], self.raw)


def unwrap_head(head):
    """-> (u8 tensor or None, raw)"""
    if isinstance(head, RingHead):
        return head.slots, head.raw
    return head, False


def normalize_scans(scans):
    """x / 6 - 0.5 (stage_world1.py:140) of raw lidar ranges, rounded exactly as the env's own MRCA_F_OBS view is
    (mrca_normalize_scans).  torch's ``x / 6.0`` is NOT that on the GPU: a scalar divisor becomes a multiplication by
    RN(1/6).  CPU tensors (the tests' stand-ins) take numpy's correctly rounded quotient, which equals the kernel's
    result."""
    if not scans.is_cuda:
        a = np.abs(scans.numpy())           # (|x| as the kernel does: rows stored under ABI 4-5 carried a flag in the sign bit)
        return torch.from_numpy(a / a.dtype.type(6.0) - a.dtype.type(0.5))
    x = scans.contiguous()
    if x.dtype != torch.float32 or x.numel() % 4:
        raise ValueError("normalize_scans: expected a float32 tensor with a multiple of 4 elements")
    out = torch.empty_like(x)
    with _stream_on(x.device) as stream:
        _lib.check(_lib.load().mrca_normalize_scans(x.data_ptr(), out.data_ptr(), x.numel(), stream), "mrca_normalize_scans")
    return out


class FrameTable:
    """Observation stacks addressed through a row table instead of gathered: ``frames`` f32[*, 512] (a matrix of normalised
    frames: the rollout buffer's one-frame-per-tick store, flattened) and ``rows`` i32[n, 3], the row of each sample's three
    frames, oldest first.  What ``lidar_features_fn`` takes in place of a [n, 3, 512] tensor (mrca_lidar_features_rows):
    the minibatch's copy of its stacks -- 100 MB written and read per 16 384 samples -- is never made.  ``gather()`` makes it
    for whoever needs a tensor (the stock policy path)."""

    def __init__(self, frames, rows):
        if not (frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 2 and frames.shape[1] == 512):
            raise ValueError("FrameTable: frames must be a contiguous float32 matrix [*, 512]")
        if not (rows.dtype == torch.int32 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == 3 and
                rows.device == frames.device):
            raise ValueError("FrameTable: rows must be a contiguous int32 tensor [n, 3] on the frames' device")
        self.frames, self.rows = frames, rows

    @property
    def shape(self):
        return (self.rows.shape[0], 3, 512)

    @property
    def device(self):
        return self.frames.device

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    def gather(self):
        return self.frames[self.rows.long()]

    def record_stream(self, stream):
        if self.rows.is_cuda:
            self.rows.record_stream(stream)


# the conv front end's two precisions, ``bf16`` -> (dtype of the features and of their gradients, stem of the entry points'
# names: mrca_<stem>[_rows], mrca_<stem>_backward[_rows])
_FRONT_END = {False: (torch.float32, "lidar_features"), True: (torch.bfloat16, "lidar_features_bf16")}
_CONV_SHAPES = ((2, 32, 3, 5), (2, 32), (2, 32, 32, 3), (2, 32))        # w1, b1, w2, b2, tower-major


def _front_end_forward(who, bf16, obs, w1, b1, w2, b2, out, head, scale=None):
    """The forward of the conv front end at either precision, for a stack tensor (with or without ring heads) or a
    ``FrameTable`` -> features [2, N, 4096].  The weights are fp32 either way.  ``scale`` f32[N]: the per-robot scan scale of
    the safe policy (mrca_<stem>_scaled; raw ring form only)."""
    lib = _lib.load()
    dtype, stem = _FRONT_END[bf16]
    _check(who, torch.float32, *zip((w1, b1, w2, b2), _CONV_SHAPES))
    if isinstance(obs, FrameTable):
        if head is not None:
            raise ValueError(f"{who}: a FrameTable is in deque order already (no head)")
        if not obs.is_cuda:
            raise ValueError(f"{who}: the FrameTable must live on the GPU")
        if scale is not None:
            raise ValueError(f"{who}: scale needs the ring of RAW scans, head=RingHead(slots, raw=True), not a FrameTable")
        entry, source = f"mrca_{stem}_rows", (obs.frames.data_ptr(), obs.rows.data_ptr())
    else:
        head, raw = unwrap_head(head)
        if obs.dim() != 3:
            raise ValueError(f"{who}: expected obs of shape [N, 3, 512], got {tuple(obs.shape)}")
        _check(who, torch.float32, (obs, (obs.shape[0], 3, 512)))
        if head is not None:        # one entry per robot
            _check(who, torch.uint8, (head, obs.shape[0]))
        entry, source = f"mrca_{stem}", (obs.data_ptr(), None if head is None else head.data_ptr(), int(raw))
        if scale is not None:
            if head is None or not raw:
                raise ValueError(f"{who}: scale needs the ring of RAW scans, head=RingHead(slots, raw=True) -- normalised "
                                 "observations cannot be rescaled")
            _check(who, torch.float32, (scale, (obs.shape[0],)), device=obs.device)
            entry, source = f"mrca_{stem}_scaled", (obs.data_ptr(), head.data_ptr(), scale.data_ptr())
    N = obs.shape[0]
    if out is None:
        out = torch.empty(2, N, 4096, dtype=dtype, device=obs.device)
    elif bf16:      # (the kernel stores 16 bytes at a time; an fp32 buffer is the caller's to get right)
        _check(who, dtype, (out, (2, N, 4096)), device=obs.device)
        if out.data_ptr() % 16:
            raise ValueError(f"{who}: out must be 16-byte aligned")
    with _stream_on(obs.device) as stream:
        _lib.check(getattr(lib, entry)(*source, N, 3, 512, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                       out.data_ptr(), stream), entry)
    return out


def lidar_features(obs, w1, b1, w2, b2, out=None, head=None, scale=None):
    """relu(conv2(relu(conv1(obs)))) of the actor and the critic tower in one launch.
    obs f32[N,3,512]; w1 f32[2,32,3,5], b1 f32[2,32], w2 f32[2,32,32,3], b2 f32[2,32] (tower-major: actor, critic)
    -> f32[2,N,4096], rows in the flatten order of [32,128].
    ``head`` u8[N] or a ``RingHead``: ``obs`` is a frame RING (VecStageWorld.policy_obs()) and head[n] the slot of
    robot n's newest frame; the kernel reads the frames in deque order while staging -- and, for a ring of RAW scans,
    forms the observation x / 6 - 0.5 on the way.  None: ``obs`` is in deque order.
    ``scale`` f32[N] (needs ``head=RingHead(..., raw=True)``): the safe policy's scan (mrca_lidar_features_scaled) -- every
    return of robot n, in all three frames, is seen at ``scale[n]`` times its range (a beam that returned nothing stays
    nothing); ones give the bits of ``scale=None``, which calls the unscaled entry point."""
    return _front_end_forward("lidar_features", False, obs, w1, b1, w2, b2, out, head, scale)


def lidar_features_bf16(obs, w1, b1, w2, b2, out=None, head=None, scale=None):
    """lidar_features on bf16 MFMAs (csrc/mrca_policy_bf16.hip): same arguments (fp32 weights, tower-major), returns
    bf16[2,N,4096].  Rounding points (include/mrca_env.h: mrca_lidar_features_bf16): the observation, w1, w2, h1 and the
    output are rounded to bf16 (nearest even); the biases are added in fp32.  Rollout inference only: a FrameTable (the
    update's row-table form) is refused.  ``scale``: as ``lidar_features`` (the multiply happens in fp32, in front of the
    observation's rounding)."""
    if isinstance(obs, FrameTable):
        raise ValueError("lidar_features_bf16: inference only -- a FrameTable (the update path) is not supported")
    return _front_end_forward("lidar_features_bf16", True, obs, w1, b1, w2, b2, out, head, scale)


def lidar_features_bf16_rows(table, w1, b1, w2, b2, out=None):
    """lidar_features_bf16 with the stacks addressed through a ``FrameTable`` (normalised frames; csrc/mrca_policy_bf16_rows.hip):
    the forward of the fused bf16 update.  Same rounding points and device code as the rollout's kernel; bit for bit what
    ``lidar_features_bf16(table.gather(), ...)`` returns.  -> bf16[2,N,4096]"""
    if not isinstance(table, FrameTable):
        raise ValueError("lidar_features_bf16_rows: expected a FrameTable on the GPU")
    return _front_end_forward("lidar_features_bf16_rows", True, table, w1, b1, w2, b2, out, None)


def policy_tail(h1, goal, speed, fc2_w, fc2_b, head_w, head_b, critic_w, critic_b, logstd, noise, lo, hi, fc1_b=None):
    """Everything of the rollout inference behind fc1 in one launch (include/mrca_env.h: mrca_policy_tail).
    h1 f32[2,N,256] = fc1 outputs before the ReLU -- with their bias, or without it and ``fc1_b`` f32[2,256] (any shape
    of 512 elements) given: the kernel adds it while it stages h1.  noise f32[N,2] or None (deterministic mean action).
    -> value [N,1], action [N,2], logprob [N,1], scaled [N,2], mean [N,2]"""
    lib = _lib.load()
    N = h1.shape[1]
    dev = h1.device
    _check("policy_tail", torch.float32, (h1, (2, N, 256)), (goal, (N, 2)), (speed, (N, 2)), (fc2_w, (2, 260, 128)), (fc2_b, 256),
           (head_w, (128, 2)), (head_b, (2,)), (critic_w, 128), (critic_b, 1), (logstd, (2,)), (lo, (2,)), (hi, (2,)),
           *(() if noise is None else ((noise, (N, 2)),)))
    if fc1_b is not None:       # 2 x 256 elements in any shape, on h1's device
        _check("policy_tail", torch.float32, (fc1_b, 512), device=dev)
    value = torch.empty(N, 1, dtype=torch.float32, device=dev)
    action = torch.empty(N, 2, dtype=torch.float32, device=dev)
    logprob = torch.empty(N, 1, dtype=torch.float32, device=dev)
    scaled = torch.empty(N, 2, dtype=torch.float32, device=dev)
    mean = torch.empty(N, 2, dtype=torch.float32, device=dev)
    with _stream_on(dev) as stream:
        _lib.check(lib.mrca_policy_tail(h1.data_ptr(), None if fc1_b is None else fc1_b.data_ptr(), goal.data_ptr(), speed.data_ptr(), N, fc2_w.data_ptr(), fc2_b.data_ptr(),
                                        head_w.data_ptr(), head_b.data_ptr(), critic_w.data_ptr(), critic_b.data_ptr(),
                                        logstd.data_ptr(), None if noise is None else noise.data_ptr(), lo.data_ptr(),
                                        hi.data_ptr(), value.data_ptr(), action.data_ptr(), logprob.data_ptr(),
                                        scaled.data_ptr(), mean.data_ptr(), stream), "mrca_policy_tail")
    return value, action, logprob, scaled, mean


def _front_end_backward(bf16, obs, w1, b1, w2, feat, gfeat_act, gfeat_crt):
    """The backward of the conv front end at either precision: ``feat`` and the two gradients are of the precision's dtype,
    everything else -- and the four gradients returned -- fp32."""
    lib = _lib.load()
    dtype, stem = _FRONT_END[bf16]
    who = stem + "_backward"
    N = obs.shape[0]
    table = isinstance(obs, FrameTable)
    _check(who, torch.float32, *zip((w1, b1, w2), _CONV_SHAPES), *(() if table else ((obs, (N, 3, 512)),)))
    _check(who, dtype, (feat, (2, N, 4096)), (gfeat_act, (N, 4096)), (gfeat_crt, (N, 4096)))
    dev = obs.device
    dw1, db1 = torch.empty_like(w1), torch.empty_like(b1)
    dw2, db2 = torch.empty_like(w2), torch.empty(2, 32, dtype=torch.float32, device=dev)
    entry = f"mrca_{who}_rows" if table else f"mrca_{who}"
    source = (obs.frames.data_ptr(), obs.rows.data_ptr()) if table else (obs.data_ptr(),)
    with _stream_on(dev) as stream:
        scratch = _scratch_of(who, dev, stream)
        _lib.check(getattr(lib, entry)(*source, N, 3, 512, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), feat.data_ptr(),
                                       gfeat_act.data_ptr(), gfeat_crt.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                                       db2.data_ptr(), scratch.data_ptr(), scratch.numel(), stream), entry)
    return dw1, db1, dw2, db2


def lidar_features_backward(obs, w1, b1, w2, feat, gfeat_act, gfeat_crt):
    """Gradients of lidar_features with respect to (w1, b1, w2, b2) given dLoss/dfeat of the two towers (two [N,4096]
    buffers: they come out of two independent fc1 backward GEMMs); see include/mrca_env.h.
    -> dw1 f32[2,32,3,5], db1 f32[2,32], dw2 f32[2,32,32,3], db2 f32[2,32]"""
    return _front_end_backward(False, obs, w1, b1, w2, feat, gfeat_act, gfeat_crt)


def lidar_features_bf16_backward(obs, w1, b1, w2, feat, gfeat_act, gfeat_crt):
    """Gradients of the bf16 front end with respect to (w1, b1, w2, b2) on bf16 MFMAs (csrc/mrca_policy_bf16_bwd.hip; the
    numerical contract: include/mrca_env.h, mrca_lidar_features_bf16_backward).  ``obs`` f32[N,3,512] normalised observations
    or a ``FrameTable``; fp32 weights (tower-major); ``feat`` bf16[2,N,4096] the bf16 forward's output; ``gfeat_act`` /
    ``gfeat_crt`` bf16[N,4096].  -> fp32 dw1 [2,32,3,5], db1 [2,32], dw2 [2,32,32,3], db2 [2,32]"""
    return _front_end_backward(True, obs, w1, b1, w2, feat, gfeat_act, gfeat_crt)


class _LidarFeatures(torch.autograd.Function):
    """-> (actor features [N,4096], critic features [N,4096]) at the precision ``bf16`` selects: two outputs, so that autograd
    hands the backward kernel the two fc1 gradients as they are (one stacked output cost a zero-fill + two copies + an add of
    [2,N,4096] per minibatch: profiles/r03a_update_bench.txt).  Under bf16 the roundings are straight-through."""

    @staticmethod
    def forward(ctx, bf16, obs, w1, b1, w2, b2):
        w1, b1, w2, b2 = (t.detach().contiguous() for t in (w1, b1, w2, b2))
        table = obs if isinstance(obs, FrameTable) else None
        if table is None:
            obs = obs.detach().contiguous()
        feat = _front_end_forward(_FRONT_END[bf16][1] + "_fn", bf16, obs, w1, b1, w2, b2, None, None)
        if table is None:
            ctx.save_for_backward(obs, w1, b1, w2, feat)
        else:       # (the frame store and the row table are data: kept by reference, like a saved tensor)
            ctx.save_for_backward(table.frames, table.rows, w1, b1, w2, feat)
        ctx.table, ctx.bf16 = table is not None, bf16
        return feat[0], feat[1]

    @staticmethod
    def backward(ctx, g_act, g_crt):
        if ctx.table:
            frames, rows, w1, b1, w2, feat = ctx.saved_tensors
            obs = FrameTable(frames, rows)
        else:
            obs, w1, b1, w2, feat = ctx.saved_tensors
        if ctx.bf16:        # the fc1 gradients arrive in whatever precision fc1's backward produced: rounded to bf16 once
            g_act, g_crt = (None if g is None else g.to(torch.bfloat16) for g in (g_act, g_crt))
        g_act = torch.zeros_like(feat[0]) if g_act is None else g_act.contiguous()
        g_crt = torch.zeros_like(feat[1]) if g_crt is None else g_crt.contiguous()
        dw1, db1, dw2, db2 = _front_end_backward(ctx.bf16, obs, w1, b1, w2, feat, g_act, g_crt)
        return None, None, dw1, db1, dw2, db2


def lidar_features_fn(obs, w1, b1, w2, b2):
    """Differentiable lidar_features: same arguments, returns (actor features, critic features), gradients flow to
    w1 / b1 / w2 / b2 (the scan is data)."""
    return _LidarFeatures.apply(False, obs, w1, b1, w2, b2)


def lidar_features_bf16_fn(obs, w1, b1, w2, b2):
    """Differentiable bf16 front end of the opt-in fused bf16 update: ``obs`` f32[N,3,512] (normalised) or a ``FrameTable``, fp32
    weights (tower-major) -> (actor features, critic features), two bf16 matrices [N,4096]; fp32 gradients flow to
    w1 / b1 / w2 / b2 through csrc/mrca_policy_bf16_bwd.hip (the scan is data).  Not the reference's precision."""
    return _LidarFeatures.apply(True, obs, w1, b1, w2, b2)


# ---------------------------------------------------------------------------------------- the opt-in fused bf16 update's fc1
class _Fc1Bf16(torch.autograd.Function):
    """fc1 of the fused bf16 update as three library GEMMs with bf16 operands and fp32 accumulation:
    forward   h = feat x Wb^T                       fp32 result (the bias is the caller's, added in fp32)
    dgrad     gfeat = bf16(g) x Wb                  stored as bf16 (the front end's backward reads it)
    wgrad     dW = bf16(g)^T x feat                 fp32 result: the gradient of the fp32 master weight
    g = the fp32 gradient that reaches fc1's output, rounded to bf16 once; the roundings are straight-through."""

    @staticmethod
    def forward(ctx, feat, weight, weight_bf16):
        ctx.save_for_backward(feat, weight_bf16)
        return torch.mm(feat, weight_bf16.t(), out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        feat, wb = ctx.saved_tensors
        gb = g.to(torch.bfloat16)
        gfeat = torch.mm(gb, wb) if ctx.needs_input_grad[0] else None
        dw = torch.mm(gb.t(), feat, out_dtype=torch.float32) if ctx.needs_input_grad[1] else None
        return gfeat, dw, None


def fc1_bf16(feat, weight, weight_bf16):
    """``feat`` bf16[N,4096] x fc1's weight -> f32[N,256] (no bias).  ``weight`` f32[256,4096] is the master parameter (it
    receives the fp32 weight gradient), ``weight_bf16`` its bf16 copy, the operand of the GEMMs."""
    if not (feat.dtype == torch.bfloat16 and weight_bf16.dtype == torch.bfloat16 and weight.dtype == torch.float32 and
            weight.shape == weight_bf16.shape):
        raise ValueError("fc1_bf16: expected bf16 features, the fp32 master weight and its bf16 copy of the same shape")
    return _Fc1Bf16.apply(feat, weight, weight_bf16)


# ------------------------------------------------------------------------------------------------ the PPO loss tail
class _PPOLoss(torch.autograd.Function):
    """loss = L_pi + value_coef * L_v - coeff_entropy * H of model/ppo.py:172-185 with its gradients with respect to the
    network's outputs (mean, value, logstd) from ONE launch (csrc/mrca_ppo_loss.hip); backward scales them by the incoming
    gradient (1 for ``loss.backward()``)."""

    @staticmethod
    def forward(ctx, mean, value, logstd, action, old_logprob, adv, target, clip_value, value_coef, coeff_entropy):
        lib = _lib.load()
        n = mean.shape[0]
        args = [t.detach().contiguous().view(-1) for t in (mean, value, logstd, action, old_logprob, adv, target)]
        # mean [n,2], value [n,1], logstd [2], action [n,2], old_logprob / adv / target [n,1], flattened
        _check("ppo_loss", torch.float32, *zip(args, (2 * n, n, 2, 2 * n, n, n, n)))
        dev = mean.device
        out = torch.empty(8, dtype=torch.float32, device=dev)
        gmean = torch.empty(n, 2, dtype=torch.float32, device=dev)
        gvalue = torch.empty(n, 1, dtype=torch.float32, device=dev)
        with _stream_on(dev) as stream:
            scratch = _scratch_of("ppo_loss", dev, stream)
            _lib.check(lib.mrca_ppo_loss(*[t.data_ptr() for t in args], n, float(clip_value), float(value_coef),
                                         float(coeff_entropy), out.data_ptr(), gmean.data_ptr(), gvalue.data_ptr(),
                                         scratch.data_ptr(), scratch.numel(), stream), "mrca_ppo_loss")
        ctx.save_for_backward(gmean, gvalue, out)
        ctx.value_shape, ctx.logstd_shape = value.shape, logstd.shape
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        gmean, gvalue, out = ctx.saved_tensors
        return (gmean * g_loss, (gvalue * g_loss).view(ctx.value_shape), (out[5:7] * g_loss).view(ctx.logstd_shape),
                None, None, None, None, None, None, None)


def ppo_loss(mean, value, logstd, action, old_logprob, adv, target, clip_value, value_coef, coeff_entropy):
    """-> (loss, stats): ``loss`` differentiable with respect to mean [n,2], value [n,1] and logstd [2]; ``stats`` f32[8] =
    loss, policy loss, value loss, entropy, k3 KL(old || new), dloss/dlogstd[0], dloss/dlogstd[1], 0."""
    return _PPOLoss.apply(mean, value, logstd, action, old_logprob, adv, target, clip_value, value_coef, coeff_entropy)


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    """One Adam step on flat CUDA buffers in ONE launch (include/mrca_env.h: mrca_adam_step; torch.optim.Adam's rule, no
    weight decay, no amsgrad).  ``param``, ``exp_avg``, ``exp_avg_sq`` are updated in place; ``step`` counts from 1."""
    lib = _lib.load()
    n = param.numel()
    _check("adam_step", torch.float32, (param, (n,)), (grad, (n,)), (exp_avg, (n,)), (exp_avg_sq, (n,)), device=param.device)
    with _stream_on(param.device) as stream:
        _lib.check(lib.mrca_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
                                      float(lr), float(beta1), float(beta2), float(eps), int(step), stream), "mrca_adam_step")


class _PolicyHeads(torch.autograd.Function):
    """mean = [sigmoid(actor1(a)), tanh(actor2(a))], value = critic(c) (model/net.py:47-55,61-63) and their gradients as
    row kernels (csrc/mrca_policy_heads.hip) instead of three skinny GEMMs forward and six backward."""

    @staticmethod
    def forward(ctx, a, c, w1, b1, w2, b2, wc, bc, relu_inputs=False, zb_a=None, zb_c=None):
        # zb_a / zb_c: the biases of the layers that produced a / c (act_fc2.bias / crt_fc2.bias), or None.  Not used forward --
        # the caller added them with the bias DETACHED (F.linear(x, W, b.detach())) -- they are here to receive their gradient:
        # the column sums of da / dc, which the backward kernel forms on the way (mrca_policy_heads_backward_bias)
        lib = _lib.load()
        n = a.shape[0]
        a, c = a.detach().contiguous(), c.detach().contiguous()
        ws = [t.detach().contiguous().view(-1) for t in (w1, b1, w2, b2, wc, bc)]
        # a, c [n,128], then three pairs of a weight row [1,128] and its bias [1]
        _check("policy_heads", torch.float32, *zip([a, c] + ws, (n * 128, n * 128, 128, 1, 128, 1, 128, 1)), device=a.device)
        mean = torch.empty(n, 2, dtype=torch.float32, device=a.device)
        value = torch.empty(n, 1, dtype=torch.float32, device=a.device)
        with _stream_on(a.device) as stream:
            _lib.check(lib.mrca_policy_heads(a.data_ptr(), c.data_ptr(), n, *[t.data_ptr() for t in ws], int(bool(relu_inputs)),
                                             mean.data_ptr(), value.data_ptr(), stream), "mrca_policy_heads")
        ctx.save_for_backward(a, c, mean, ws[0], ws[2], ws[4])
        ctx.shapes = (w1.shape, b1.shape, w2.shape, b2.shape, wc.shape, bc.shape)
        ctx.relu_inputs = bool(relu_inputs)
        ctx.z_bias = (zb_a is not None, zb_c is not None)
        return mean, value

    @staticmethod
    def backward(ctx, gmean, gvalue):
        lib = _lib.load()
        a, c, mean, w1, w2, wc = ctx.saved_tensors
        n, dev = a.shape[0], a.device
        gmean = None if gmean is None else gmean.contiguous()
        gvalue = None if gvalue is None else gvalue.contiguous()
        da, dc = torch.empty_like(a), torch.empty_like(c)
        dw = torch.empty(3 * 128 + 3, dtype=torch.float32, device=dev)
        with _stream_on(dev) as stream:
            scratch = _scratch_of("policy_heads backward", dev, stream)
            head = (a.data_ptr(), c.data_ptr(), mean.data_ptr(), None if gmean is None else gmean.data_ptr(),
                    None if gvalue is None else gvalue.data_ptr(), n, w1.data_ptr(), w2.data_ptr(), wc.data_ptr(),
                    int(ctx.relu_inputs), da.data_ptr(), dc.data_ptr(), dw.data_ptr())
            dzb = None
            if any(ctx.z_bias):
                dzb = torch.empty(256, dtype=torch.float32, device=dev)
                _lib.check(lib.mrca_policy_heads_backward_bias(*head, dzb.data_ptr(), scratch.data_ptr(), scratch.numel(), stream),
                           "mrca_policy_heads_backward_bias")
            else:
                _lib.check(lib.mrca_policy_heads_backward(*head, scratch.data_ptr(), scratch.numel(), stream),
                           "mrca_policy_heads_backward")
        s = ctx.shapes
        return (da, dc, dw[0:128].view(s[0]), dw[384:385].view(s[1]), dw[128:256].view(s[2]), dw[385:386].view(s[3]),
                dw[256:384].view(s[4]), dw[386:387].view(s[5]), None,
                dzb[0:128] if ctx.z_bias[0] else None, dzb[128:256] if ctx.z_bias[1] else None)


def policy_heads(a, c, w_actor1, b_actor1, w_actor2, b_actor2, w_critic, b_critic, relu_inputs=False, z_bias=None):
    """-> (mean [n,2], value [n,1]) of the three output heads, differentiable with respect to the first eight arguments
    (include/mrca_env.h: mrca_policy_heads / _backward).  ``relu_inputs``: ``a`` / ``c`` are fc2's outputs BEFORE their ReLU --
    the kernels apply it (and its mask on the way back).  ``z_bias`` = (bias of the layer that produced a, ... that produced c):
    they receive the column sums of da / dc as their gradient -- for a caller that formed a / c with those biases detached
    (``F.linear(x, W, b.detach())``), so that autograd does not sum the same columns again."""
    zb_a, zb_c = z_bias if z_bias is not None else (None, None)
    return _PolicyHeads.apply(a, c, w_actor1, b_actor1, w_actor2, b_actor2, w_critic, b_critic, relu_inputs, zb_a, zb_c)


class _ReluCat(torch.autograd.Function):
    """[relu(h1), goal, speed] (model/net.py:43-45) and dh1 = gout[:, :256] where h1 > 0, one launch each."""

    @staticmethod
    def forward(ctx, h1, goal, speed, h1_bias=None):
        # h1_bias: the bias of the layer that produced h1 (act_fc1.bias / crt_fc1.bias) or None -- not used forward (the caller
        # added it DETACHED), here to receive its gradient: the column sums of dh1 (mrca_relu_cat_backward_bias)
        lib = _lib.load()
        n = h1.shape[0]
        h1, goal, speed = h1.detach().contiguous(), goal.detach().contiguous(), speed.detach().contiguous()
        _check("relu_cat", torch.float32, (h1, (n, 256)), (goal, (n, 2)), (speed, (n, 2)), device=h1.device)
        out = torch.empty(n, 260, dtype=torch.float32, device=h1.device)
        with _stream_on(h1.device) as stream:
            _lib.check(lib.mrca_relu_cat(h1.data_ptr(), goal.data_ptr(), speed.data_ptr(), n, out.data_ptr(), stream), "mrca_relu_cat")
        ctx.save_for_backward(h1)
        ctx.h1_bias = h1_bias is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        (h1,) = ctx.saved_tensors
        gout = gout.contiguous()
        dh1 = torch.empty_like(h1)
        db = None
        with _stream_on(h1.device) as stream:
            if ctx.h1_bias:
                db = torch.empty(256, dtype=torch.float32, device=h1.device)
                scratch = _scratch_of("relu_cat backward", h1.device, stream)
                _lib.check(lib.mrca_relu_cat_backward_bias(h1.data_ptr(), gout.data_ptr(), h1.shape[0], dh1.data_ptr(), db.data_ptr(),
                                                           scratch.data_ptr(), scratch.numel(), stream), "mrca_relu_cat_backward_bias")
            else:
                _lib.check(lib.mrca_relu_cat_backward(h1.data_ptr(), gout.data_ptr(), h1.shape[0], dh1.data_ptr(), stream),
                           "mrca_relu_cat_backward")
        return dh1, None, None, db


def relu_cat(h1, goal, speed, h1_bias=None):
    """-> f32[n,260] = cat(relu(h1), goal, speed); differentiable with respect to ``h1`` (goal and speed are data).
    ``h1_bias``: the bias of the layer that produced ``h1``, for a caller that added it detached: it receives the column sums of
    dh1 as its gradient (see ``policy_heads``' ``z_bias``)."""
    return _ReluCat.apply(h1, goal, speed, h1_bias)
