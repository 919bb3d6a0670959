"""Reference arithmetic of the bf16 front end (csrc/mrca_policy_bf16.hip, include/mrca_env.h: mrca_lidar_features_bf16),
shared by tests/test_policy_bf16_layout.py (CPU) and tests/test_gpu_policy_bf16.py.  Rounding points: the observation,
w1 and w2 to bf16; fp32 biases; h1 = relu(conv1 + b1) to bf16; feat = relu(conv2 + b2) to bf16 -- every rounding to
nearest even."""
import numpy as np


def rne_bf16(a):
    """float32 values -> the nearest bf16 values (ties to even), as float32.  NaN stays NaN (quietened), infinities and
    overflow to infinity as IEEE rounding has them."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32).copy()
    nan = np.isnan(a)
    out[nan] = np.float32("nan")
    return out


def _conv_rows(x, w, stride=2, pad=1):
    """x f64[N, C, L], w f64[O, C, k] -> f64[N, O, Lout] (zero padding): each output a float64 sum of its products"""
    N, C, L = x.shape
    O, _, k = w.shape
    xp = np.zeros((N, C, L + 2 * pad))
    xp[:, :, pad:pad + L] = x
    Lout = (L + 2 * pad - k) // stride + 1
    idx = np.arange(Lout)[:, None] * stride + np.arange(k)[None, :]          # [Lout, k]
    win = xp[:, :, idx].transpose(0, 2, 1, 3).reshape(N * Lout, C * k)       # [N Lout, C k]
    return (win @ w.reshape(O, C * k).T).reshape(N, Lout, O).transpose(0, 2, 1)


def front_end_ref(x, w1, b1, w2, b2, chunk=512):
    """One tower.  x f32[N, 3, 512] (normalised observations), w1 f32[32, 3, 5], b1 f32[32], w2 f32[32, 32, 3], b2 f32[32]
    -> (feat: f32[N, 4096] the rounded outputs, exact: f64[N, 4096] conv2 + b2 after the ReLU on the bf16 h1 but before the
    last rounding, S: f64[N, 4096] the sum of the absolute values of each output's conv2 terms and bias)."""
    if x.shape[0] > chunk:
        parts = [front_end_ref(x[i:i + chunk], w1, b1, w2, b2, chunk) for i in range(0, x.shape[0], chunk)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    xb = rne_bf16(x).astype(np.float64)
    w1b, w2b = rne_bf16(w1).astype(np.float64), rne_bf16(w2).astype(np.float64)
    c1 = _conv_rows(xb, w1b) + b1.astype(np.float64)[None, :, None]
    h1 = rne_bf16(np.maximum(c1, 0.0).astype(np.float32)).astype(np.float64)
    c2 = _conv_rows(h1, w2b) + b2.astype(np.float64)[None, :, None]
    exact = np.maximum(c2, 0.0)
    feat = rne_bf16(exact.astype(np.float32))
    S = _conv_rows(np.abs(h1), np.abs(w2b)) + np.abs(b2.astype(np.float64))[None, :, None]
    n = x.shape[0]
    return feat.reshape(n, -1), exact.reshape(n, -1), S.reshape(n, -1)
