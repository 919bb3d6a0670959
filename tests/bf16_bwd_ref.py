"""Reference arithmetic of the bf16 front end's BACKWARD (csrc/mrca_policy_bf16_bwd.hip, include/mrca_env.h:
mrca_lidar_features_bf16_backward), beside bf16_ref.py's forward: a float64 NumPy statement of the numerical contract.

Per tower, with R() = round to nearest even to bf16 (of the fp32 value):
    x = R(obs), w1 = R(w1), w2 = R(w2); b1 fp32
    h1 = R(relu(conv1(x) + b1))                                          as the forward forms it
    g2 = gfeat * (feat > 0)                                              exact (gfeat and feat are bf16 values)
    dw2[c][ci][k] = sum g2[c][l] h1[ci][2l + k - 1]      db2[c] = sum g2[c][l]
    dh1[ci][p] = sum_{c, k: 2l + k - 1 = p} w2[c][ci][k] g2[c][l];  g1 = R(dh1 * (h1 > 0))
    dw1[c][ci][k] = sum g1[c][p] x[ci][2p + k - 1]       db1[c] = sum g1[c][p]
The roundings are straight-through.  Every sum here is float64 (the kernel's are fp32 sums of exact products).
``rounding=False`` switches every R() off: the plain gradients of the two Conv1d + ReLU layers (the self-check of
tests/test_policy_bf16_bwd_host.py compares them with torch's float64 autograd)."""
import numpy as np

from bf16_ref import rne_bf16


def _r(a, rounding):
    return rne_bf16(np.asarray(a, dtype=np.float64).astype(np.float32)).astype(np.float64) if rounding else np.asarray(a, np.float64)


def front_end_bwd_ref(x, w1, b1, w2, b2, gfeat, feat=None, rounding=True, chunk=128, h1=None, return_h1=False):
    """One tower.  x f32[N,3,512] (normalised observations), w1 [32,3,5], b1 [32], w2 [32,32,3], b2 [32] (used only when
    ``feat`` is None: the second ReLU's mask then comes from this function's own forward), gfeat [N,4096] dLoss / dfeat,
    feat [N,4096] the forward's output or None; h1 [N,32,255] or None: h1 "as the forward forms it" handed in -- the
    hardware's fp32 accumulation puts a few of its 8160 values per sample on the other side of a bf16 rounding boundary than
    this function's float64 sum does (tests/test_gpu_policy_bf16_update.py reads it out of the forward kernel), as ``feat``
    hands in the second ReLU's mask.  -> float64 dw1 [32,3,5], db1 [32], dw2 [32,32,3], db2 [32] (and, ``return_h1``, this
    function's own h1 [N,32,255])"""
    N = x.shape[0]
    w1b, w2b = _r(w1, rounding), _r(w2, rounding)
    b1d, b2d = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    idx1 = 2 * np.arange(255)[:, None] + np.arange(5)[None, :]           # into x padded by 1: x[2p + k - 1]
    idx2 = 2 * np.arange(128)[:, None] + np.arange(3)[None, :]           # into h1 padded by 1: h1[2l + k - 1]
    dw1, db1 = np.zeros((32, 3, 5)), np.zeros(32)
    dw2, db2 = np.zeros((32, 32, 3)), np.zeros(32)
    own = []
    for i in range(0, N, chunk):
        xb = _r(x[i:i + chunk], rounding)
        n = xb.shape[0]
        xp = np.zeros((n, 3, 514))
        xp[:, :, 1:513] = xb
        win1 = xp[:, :, idx1]                                            # [n, 3, 255, 5]
        c1 = np.einsum("ncpk,ock->nop", win1, w1b) + b1d[None, :, None]
        own_h1 = _r(np.maximum(c1, 0.0), rounding)                       # [n, 32, 255]
        own.append(own_h1)
        h1c = own_h1 if h1 is None else np.asarray(h1[i:i + chunk], np.float64)
        h1p = np.zeros((n, 32, 257))
        h1p[:, :, 1:256] = h1c
        win2 = h1p[:, :, idx2]                                           # [n, 32, 128, 3]
        if feat is None:
            mask = (np.einsum("ncls,ocs->nol", win2, w2b) + b2d[None, :, None]) > 0
        else:
            mask = np.asarray(feat[i:i + chunk], np.float64).reshape(n, 32, 128) > 0
        g2 = np.asarray(gfeat[i:i + chunk], np.float64).reshape(n, 32, 128) * mask
        dw2 += np.einsum("nol,ncls->ocs", g2, win2)
        db2 += g2.sum(axis=(0, 2))
        dh1p = np.zeros((n, 32, 257))
        for k in range(3):
            dh1p[:, :, k:k + 256:2] += np.einsum("nol,oc->ncl", g2, w2b[:, :, k])
        g1 = _r(dh1p[:, :, 1:256] * (h1c > 0), rounding)
        dw1 += np.einsum("nop,ncpk->ock", g1, win1)
        db1 += g1.sum(axis=(0, 2))
    if return_h1:
        return dw1, db1, dw2, db2, np.concatenate(own)
    return dw1, db1, dw2, db2
