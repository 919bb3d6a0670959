"""NumPy float32 / uint32 restatement of the lidar noise rule (csrc/mrca_noise_device.h), one separately rounded operation per
line in the header's order, with the oracle's Philox and u01 -- and ``RingModel``, the scan ring as the rule leaves it when it
is applied once behind every cast (what tests/test_gpu_scan_noise.py holds the device to)."""
import numpy as np

import util as U

O = U.O
f32, u32 = np.float32, np.uint32
FIELDS = ("sigma_const", "sigma_prop", "dropout", "quantum")
RANGE_MAX = f32(6.0)
STREAM_NOISE = 2
ZERO = dict.fromkeys(FIELDS, 0.0)
DEFAULTS = dict(sigma_const=0.01, sigma_prop=0.01, dropout=0.005, quantum=0.0)       # mrca_scan_noise_default_params


def params(**kw):
    """all-zero params with ``kw`` set"""
    assert set(kw) <= set(FIELDS), kw
    return {**ZERO, **kw}


def key_of(seed):
    return u32(seed & 0xFFFFFFFF), u32((seed >> 32) & 0xFFFFFFFF)


def counter_word(t):
    """counter word 3 of the draw: (T << 2) | 2 as uint32"""
    return ((((np.asarray(t).astype(np.int64)) << 2) | STREAM_NOISE) & 0xFFFFFFFF).astype(u32)


def draw(gid, episode, t, beams, key):
    """the four words of every (robot, beam): gid / episode / t [N] -> 4 x uint32[N, beams]"""
    gid, episode = (np.asarray(a).astype(np.int64) for a in (gid, episode))
    N = len(gid)
    c0 = np.broadcast_to((gid & 0xFFFFFFFF).astype(u32)[:, None], (N, beams))
    c1 = np.broadcast_to((episode & 0xFFFFFFFF).astype(u32)[:, None], (N, beams))
    c2 = np.broadcast_to(np.arange(beams, dtype=u32)[None, :], (N, beams))
    c3 = np.broadcast_to(counter_word(t)[:, None], (N, beams))
    return O.philox4x32(c0, c1, c2, c3, key[0], key[1])


def deviate(ux, uy, uz):
    """the three-uniform Irwin-Hall deviate: unit variance, support +-3"""
    s = O.u01(ux, f32) + O.u01(uy, f32)
    s = s + O.u01(uz, f32)
    s = s - f32(1.5)
    return s * f32(2.0)


def apply(p, rows, words):
    """The rule on rows f32[N, B] with the draws ``words`` (4 x uint32[N, B]) -> (noisy rows, clear bool[N, B]: the beams
    whose hit bit goes, dropped bool[N, B])."""
    r = np.ascontiguousarray(rows, f32)
    sc, sp, dr, qu = (f32(p[k]) for k in FIELDS)
    returns = ~(r >= RANGE_MAX)
    with np.errstate(all="ignore"):
        if sc > 0 or sp > 0:
            z = deviate(words[0], words[1], words[2])
            s = sp * r
            s = sc + s
            s = s * z
            r1 = r + s
        else:
            r1 = r
        if qu > 0:
            q = r1 / qu
            q = np.rint(q)
            r2 = qu * q
        else:
            r2 = r1
        r2 = np.where(r2 > 0, r2, f32(0.0)).astype(f32)
        over = r2 >= RANGE_MAX
        dropped = O.u01(words[3], f32) < dr
    clear = (over | dropped) & returns
    out = np.where(clear, RANGE_MAX, r2).astype(f32)
    out = np.where(returns, out, r).astype(f32)
    return out, clear, dropped & returns


def noise_rows(p, rows, gid, episode, t, key):
    """The rule on the clean rows f32[N, B] of robots ``gid`` -> (noisy rows, clear)"""
    out, clear, _d = apply(p, rows, draw(gid, episode, t, np.shape(rows)[1], key))
    return out, clear


def pack_hits(hit):
    """bool[..., B] -> uint64[..., B / 64], bit b & 63 of word b >> 6 (MRCA_F_HIT_BITS)"""
    hit = np.asarray(hit).astype(bool)
    w = hit.reshape(hit.shape[:-1] + (hit.shape[-1] // 64, 64)).astype(np.uint64)
    return (w << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def norm_obs(x):
    """x / 6 - 0.5 as the views' writers round it (RN(RN(x / 6) - 0.5) on [0, 6]: mrca_device.h norm_obs)"""
    return (np.asarray(x, f32) / f32(6.0) - f32(0.5)).astype(f32)


class RingModel:
    """The scan ring, its heads and its hit plane under `one cast, one noise call`: a fresh robot's row goes to all F slots
    and leaves the head where it is, any other robot's row goes behind the head."""

    def __init__(self, N, F, B, seed):
        self.N, self.F, self.B = N, F, B
        self.key = key_of(seed)
        self.ring = np.zeros((N, F, B), f32)
        self.hit = np.zeros((N, F, B), bool)
        self.head = np.zeros(N, np.uint8)

    def cast(self, p, clean, clean_hit, fresh, episode, t, robots=None):
        """robots (indices, default all) have cast ``clean`` [N, B] / ``clean_hit`` [N, B]; p: the noise params or None"""
        idx = np.arange(self.N) if robots is None else np.asarray(robots)
        rows, hit = np.asarray(clean, f32)[idx], np.asarray(clean_hit).astype(bool)[idx]
        if p is not None:
            rows, clear = noise_rows(p, rows, idx, np.asarray(episode)[idx], np.asarray(t)[idx], self.key)
            hit = hit & ~clear
        fr = np.asarray(fresh).astype(bool)[idx]
        stale = idx[~fr]
        self.head[stale] = (self.head[stale] + 1) % self.F
        self.ring[idx[fr]] = rows[fr][:, None, :]
        self.hit[idx[fr]] = hit[fr][:, None, :]
        self.ring[stale, self.head[stale]] = rows[~fr]
        self.hit[stale, self.head[stale]] = hit[~fr]

    def newest(self):
        ar = np.arange(self.N)
        return self.ring[ar, self.head]

    def stack(self):
        """f32[N, F, B]: the normalised frames in deque order (oldest first), MRCA_F_OBS"""
        ar = np.arange(self.N)
        order = (self.head[:, None].astype(np.int64) + 1 + np.arange(self.F)[None, :]) % self.F
        return norm_obs(np.abs(self.ring[ar[:, None], order]))

    def hit_words(self):
        return pack_hits(self.hit)
