"""The lidar noise rule (csrc/mrca_noise_device.h) compiled for the host with g++ -ffp-contract=off: the very functions the
gfx950 kernel calls, held EQUAL bit for bit to the NumPy float32 restatement of tests/noise_ref.py on random and on crafted
rows; the rule's properties; the statistics of the restatement's draws; the library's defaults and validation table.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32, u32 = np.float32, np.uint32
SEED = 0x5EED0123456789AB          # the env seed of every test here (chosen once; the statistics below are of its draws)
KEY = R.key_of(SEED)
FULL = u32(0xFFFFFFFF)

SHIM = r"""
#include <stdint.h>
#include "mrca_noise_device.h"
using namespace mrca;
// rows[N][B] and hits[N][B / 64] in place, robot n with (gid, episode, t)[n]
extern "C" void shim_rows(const ScanNoiseParams* p, int N, int B, const uint32_t* gid, const int32_t* episode, const int32_t* t,
                          uint32_t k0, uint32_t k1, float* rows, unsigned long long* hits) {
    for (int n = 0; n < N; ++n) noise_row(*p, gid[n], episode[n], t[n], k0, k1, B, rows + (size_t)n * B, hits + (size_t)n * (B / 64));
}
// one beam with the draw given
extern "C" float shim_beam(const ScanNoiseParams* p, float r, uint32_t x, uint32_t y, uint32_t z, uint32_t w, int* clear) {
    const NoisyBeam nb = noise_beam(*p, r, U4{x, y, z, w});
    *clear = nb.clear;
    return nb.range;
}
extern "C" uint32_t shim_counter_word(int32_t t) { return noise_counter_word(t); }
extern "C" uint32_t shim_reset_streams(void) { return kStreamPose | (kStreamGoal << 8); }
"""


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in R.FIELDS]


def cparams(p):
    return Params(**{k: float(p[k]) for k in R.FIELDS})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_host")
    src, so = d / "shim.cpp", d / "libnoise_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    lib.shim_rows.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                              C.c_void_p, C.c_void_p]
    lib.shim_beam.argtypes = [C.POINTER(Params), C.c_float] + [C.c_uint32] * 4 + [C.POINTER(C.c_int)]
    lib.shim_beam.restype = C.c_float
    lib.shim_counter_word.argtypes = [C.c_int32]
    lib.shim_counter_word.restype = C.c_uint32
    lib.shim_reset_streams.restype = C.c_uint32
    return lib


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def host_rows(shim, p, rows, hit, gid, episode, t, key=KEY):
    """the host build of the rule -> (rows, hit bool[N, B])"""
    rows = np.ascontiguousarray(rows, f32).copy()
    N, B = rows.shape
    words = R.pack_hits(hit).copy()
    gid, episode, t = np.ascontiguousarray(gid, u32), np.ascontiguousarray(episode, np.int32), np.ascontiguousarray(t, np.int32)
    q = cparams(p)
    shim.shim_rows(C.byref(q), N, B, gid.ctypes.data, episode.ctypes.data, t.ctypes.data, int(key[0]), int(key[1]), rows.ctypes.data,
                   words.ctypes.data)
    unpacked = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(N, B)
    return rows, unpacked


def host_beam(shim, p, r, words):
    clear = C.c_int(-1)
    q = cparams(p)
    out = shim.shim_beam(C.byref(q), float(f32(r)), *[int(w) for w in words], C.byref(clear))
    return f32(out), bool(clear.value)


def ref_beam(p, r, words):
    out, clear, _d = R.apply(p, np.array([[r]], f32), [np.array([[w]], u32) for w in words])
    return out[0, 0], bool(clear[0, 0])


def random_rows(rng, N, B):
    rows = rng.uniform(0.0, 6.0, (N, B)).astype(f32)
    rows[rng.random((N, B)) < 0.3] = 6.0                 # beams that see nothing
    rows[rng.random((N, B)) < 0.05] = f32(np.nextafter(f32(6.0), f32(0.0)))
    rows[rng.random((N, B)) < 0.05] = 0.0
    hit = (rng.random((N, B)) < 0.4) & (rows < 6.0)      # a set bit never stands on a 6.0
    gid = rng.permutation(1 << 20)[:N]
    episode = rng.integers(0, 50, N)
    t = rng.integers(0, 400, N)
    return rows, hit, gid, episode, t


PARAM_SETS = [
    R.params(sigma_const=0.05),
    R.params(sigma_prop=0.03),
    R.params(dropout=0.1),
    R.params(quantum=0.01),
    R.params(sigma_const=0.02, sigma_prop=0.01, dropout=0.005, quantum=0.01),
    R.params(sigma_prop=0.05, quantum=0.25),
    R.params(dropout=1.0),
]


# ------------------------------------------------------------------------------------------------ equality with noise_ref
@pytest.mark.parametrize("beams", [64, 192, 1024])
@pytest.mark.parametrize("pi", range(len(PARAM_SETS)))
def test_host_build_equals_the_restatement(shim, beams, pi):
    p = PARAM_SETS[pi]
    rows, hit, gid, episode, t = random_rows(np.random.default_rng(100 * pi + beams), 9, beams)
    got, got_hit = host_rows(shim, p, rows, hit, gid, episode, t)
    want, clear = R.noise_rows(p, rows, gid, episode, t, KEY)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    assert np.array_equal(got_hit, hit & ~clear)
    assert not (got_hit & (got >= 6.0)).any()            # a set bit never stands on a 6.0
    assert (got >= 0).all() and (got <= 6.0).all() and not np.signbit(got).any()
    if p["dropout"] == 1.0:
        assert (got == 6.0).all() and not got_hit.any()
    else:
        assert (bits(got) != bits(rows)).any()           # the set does something


def test_crafted_beams(shim):
    """every branch of the rule with the draw given: z = -3 is the words 0, 0, 0 and z just below +3 the words of all ones"""
    below6 = f32(np.nextafter(f32(6.0), f32(0.0)))
    lo, hi = (u32(0), u32(0), u32(0)), (FULL, FULL, FULL)
    keep, drop = FULL, u32(0)                             # word 3: u01 just below 1 / u01 = 0
    c = R.params(sigma_const=0.05)
    cases = [
        # (params, range, words, the range expected or None, cleared)
        (c, 6.0, lo + (drop,), f32(6.0), False),                         # no return: not even dropout's business
        (R.params(dropout=1.0), 6.0, hi + (drop,), f32(6.0), False),
        (c, 7.5, lo + (keep,), f32(7.5), False),                         # (>= 6 is left as it is, whatever it is)
        (R.params(quantum=0.01), 0.0, hi + (keep,), f32(0.0), False),
        (R.params(quantum=0.01), -0.0, hi + (keep,), f32(0.0), False),   # -0.0 leaves as +0.0
        (R.params(dropout=0.5), -0.0, hi + (keep,), f32(0.0), False),
        (c, below6, hi + (keep,), f32(6.0), True),                       # noise lifts it over the range: 6.0, bit cleared
        (c, below6, lo + (keep,), None, False),                          # ... or leaves it a return
        (R.params(quantum=0.5), 5.9, lo + (keep,), f32(6.0), True),      # the read-out step rounds it to exactly 6
        (R.params(sigma_prop=1.0), 3.0, hi + (keep,), f32(6.0), True),
        (c, 0.01, lo + (keep,), f32(0.0), False),                        # driven below 0: +0.0, still a return
        (R.params(sigma_prop=1.0), 2.0, lo + (keep,), f32(0.0), False),
        (R.params(quantum=0.25), 0.125, lo + (keep,), f32(0.0), False),  # ties go to even: 0.5 -> 0
        (R.params(quantum=0.25), 0.375, lo + (keep,), f32(0.5), False),  # 1.5 -> 2
        (R.params(quantum=0.25), 0.625, lo + (keep,), f32(0.5), False),  # 2.5 -> 2
        (R.params(quantum=0.25), 0.875, lo + (keep,), f32(1.0), False),  # 3.5 -> 4
        (R.params(sigma_const=0.05, dropout=0.25), 2.0, lo + (u32(0x3FFFFFFF),), f32(6.0), True),      # u01 just below 0.25
        (R.params(sigma_const=0.05, dropout=0.25), 2.0, lo + (u32(0x40000000),), None, False),         # u01 = 0.25: kept
    ]
    for p, r, words, want, cleared in cases:
        got, got_clear = host_beam(shim, p, r, words)
        ref, ref_clear = ref_beam(p, r, words)
        assert bits(got) == bits(ref) and got_clear == ref_clear, (p, r, words, got, ref)
        assert got_clear == cleared, (p, r, words)
        if want is not None:
            assert bits(got) == bits(want), (p, r, words, got, want)
        else:
            assert 0 < got < 6
    # the deviate itself: -3 exactly, and the greatest one just below +3
    assert R.deviate(*[np.array([w], u32) for w in lo])[0] == -3.0
    assert 2.999 < R.deviate(*[np.array([w], u32) for w in hi])[0] < 3.0


# ------------------------------------------------------------------------------------------------ properties
def test_zero_params_change_nothing(shim):
    rows, hit, gid, episode, t = random_rows(np.random.default_rng(1), 8, 192)
    got, got_hit = host_rows(shim, R.params(), rows, hit, gid, episode, t)
    want, clear = R.noise_rows(R.params(), rows, gid, episode, t, KEY)
    assert np.array_equal(bits(got), bits(rows)) and np.array_equal(got_hit, hit)
    assert np.array_equal(bits(want), bits(rows)) and not clear.any()


def test_dropout_alone_leaves_the_other_beams_alone(shim):
    rows, hit, gid, episode, t = random_rows(np.random.default_rng(2), 8, 512)
    p = R.params(dropout=0.2)
    got, got_hit = host_rows(shim, p, rows, hit, gid, episode, t)
    _w, _c, dropped = R.apply(p, rows, R.draw(gid, episode, t, 512, KEY))
    assert 0.1 < dropped[rows < 6].mean() < 0.3
    assert np.array_equal(bits(got[~dropped]), bits(rows[~dropped])) and np.array_equal(got_hit[~dropped], hit[~dropped])
    assert (got[dropped] == 6.0).all() and not got_hit[dropped].any()


def test_a_beam_without_a_return_never_changes(shim):
    rows, hit, gid, episode, t = random_rows(np.random.default_rng(3), 8, 192)
    for p in PARAM_SETS:
        got, got_hit = host_rows(shim, p, rows, hit, gid, episode, t)
        none = rows >= 6.0
        assert none.any() and np.array_equal(bits(got[none]), bits(rows[none])) and not got_hit[none].any()


def test_the_counter_does_not_meet_the_reset_streams(shim):
    streams = shim.shim_reset_streams()
    pose, goal = streams & 0xFF, streams >> 8
    assert (pose, goal) == (R.O.STREAM_POSE, R.O.STREAM_GOAL) == (0, 1)
    ts = np.concatenate([np.arange(0, 4096), [2 ** 29, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, -1]]).astype(np.int64)
    words = R.counter_word(ts)
    assert ((words & 3) == R.STREAM_NOISE).all() and not np.isin(words, [pose, goal]).any()
    assert [shim.shim_counter_word(int(np.int32(t))) for t in ts[-5:].astype(np.int32)] == words[-5:].tolist()
    assert len(set(words[:4096].tolist())) == 4096       # ... and a robot's ticks do not meet each other
    # the same robot, episode and beam on the three streams: three different draws
    a = R.O.philox4x32(u32(5), u32(7), u32(9), u32(pose), *KEY)
    b = R.O.philox4x32(u32(5), u32(7), u32(9), u32(goal), *KEY)
    c = R.O.philox4x32(u32(5), u32(7), u32(9), R.counter_word(0), *KEY)
    assert len({tuple(int(w) for w in x) for x in (a, b, c)}) == 3


def test_two_disjoint_masks_equal_one_call(shim):
    """the draw hangs on the robot, not on who else is in the call or in which order"""
    rows, hit, gid, episode, t = random_rows(np.random.default_rng(4), 10, 192)
    p = PARAM_SETS[4]
    one, one_hit = host_rows(shim, p, rows, hit, gid, episode, t)
    two, two_hit = rows.copy(), hit.copy()
    for part in (np.arange(10) % 3 == 1, np.arange(10) % 3 != 1):
        idx = np.flatnonzero(part)[::-1]                                     # (and backwards)
        two[idx], two_hit[idx] = host_rows(shim, p, rows[idx], hit[idx], gid[idx], episode[idx], t[idx])
    assert np.array_equal(bits(one), bits(two)) and np.array_equal(one_hit, two_hit)
    # not idempotent: a second call draws the same numbers and adds them again
    again, _h = host_rows(shim, p, one, one_hit, gid, episode, t)
    assert (bits(again) != bits(one)).any()


# ------------------------------------------------------------------------------------------------ statistics of the draws
def test_statistics_of_the_restatement():
    """64 robots x 1024 beams at 3 m, env seed SEED, episode 0, T 1.  The draws are deterministic: what passes here passes on
    the device, which is held to these very bits."""
    N, B = 64, 1024
    M = N * B
    words = R.draw(np.arange(N), np.zeros(N, np.int64), np.ones(N, np.int64), B, KEY)
    z = R.deviate(words[0], words[1], words[2]).astype(np.float64)
    assert abs(z.mean()) <= 5 / np.sqrt(M), z.mean()
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(1.6 / M), z.var()           # (Irwin-Hall of three: kurtosis 2.6, var(z^2) = 1.6)
    assert np.abs(z).max() < 3.0 and np.abs(z).max() > 2.5
    rows = np.full((N, B), 3.0, f32)
    for pd in (0.005, 0.05, 0.5):
        out, clear, dropped = R.apply(R.params(dropout=pd), rows, words)
        assert abs(dropped.mean() - pd) <= 5 * np.sqrt(pd * (1 - pd) / M), (pd, dropped.mean())
        assert np.array_equal(clear, dropped) and (out[dropped] == 6.0).all() and (out[~dropped] == 3.0).all()
    # the range noise at 3 m: sigma = 0.02 + 0.01 * 3
    out, clear, _d = R.apply(R.params(sigma_const=0.02, sigma_prop=0.01), rows, words)
    err = out.astype(np.float64) - 3.0
    assert not clear.any() and abs(err.mean()) <= 5 * 0.05 / np.sqrt(M) and abs(err.std() / 0.05 - 1.0) < 0.02


# ------------------------------------------------------------------------------------------------ the library's own defaults
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.noise import ScanNoiseParams
    assert "mrca_scan_noise" in _lib.EXPORTS and "mrca_scan_noise_default_params" in _lib.EXPORTS
    assert built_lib.mrca_scan_noise_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.ScanNoiseParamsStruct()
    assert built_lib.mrca_scan_noise_default_params(C.byref(st)) == 0
    assert {k: getattr(st, k) for k in R.FIELDS} == {k: float(f32(v)) for k, v in R.DEFAULTS.items()}
    assert [n for n, _t in _lib.ScanNoiseParamsStruct._fields_] == list(R.FIELDS) and C.sizeof(st) == 16
    p = ScanNoiseParams(sigma_const=0.05)
    assert p.sigma_const == 0.05 and p.struct().dropout == f32(0.005) and p.quantum == 0.0
    q = ScanNoiseParams.from_assignments("const=0.02,prop=0.01,dropout=0.005,quantum=0.01")
    assert (q.sigma_const, q.sigma_prop, q.dropout, q.quantum) == (0.02, 0.01, 0.005, 0.01)
    assert ScanNoiseParams.from_assignments(["const=0.05"]).as_dict() == dict(sigma_const=0.05, sigma_prop=0.0, dropout=0.0, quantum=0.0)
    assert ScanNoiseParams.from_assignments("default").as_dict() == ScanNoiseParams().as_dict()
    for bad in ("nonsense=1", "const"):
        with pytest.raises(ValueError):
            ScanNoiseParams.from_assignments(bad)

    # a refused call touches nothing: `mask` stands where the device buffer would (host memory -- no call gets as far as a launch)
    mask = np.full(64, 7, np.uint8)

    def call(params=None):
        return built_lib.mrca_scan_noise(None, None if params is None else C.byref(params), C.c_void_p(mask.ctypes.data), None)
    # what can be judged without an env is judged before the env is looked at
    assert call() == -1 and b"env is NULL" in built_lib.mrca_last_error()
    bad = [("sigma_const", -0.01), ("sigma_const", 6.5), ("sigma_prop", -0.01), ("sigma_prop", 1.5), ("dropout", -0.1), ("dropout", 1.01),
           ("quantum", -0.01), ("quantum", 1.5)]
    bad += [(k, v) for k in R.FIELDS for v in (float("nan"), float("inf"), float("-inf"))]
    for k, v in bad:
        st = _lib.ScanNoiseParamsStruct()
        built_lib.mrca_scan_noise_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(st) == -1 and k.encode() in built_lib.mrca_last_error() and b"env is NULL" not in built_lib.mrca_last_error(), \
            (k, v, built_lib.mrca_last_error())
    # the edges of the table are inside it, and so are the all-zero params: these get as far as the env
    for k, v in [("sigma_const", 0.0), ("sigma_const", 6.0), ("sigma_prop", 1.0), ("dropout", 0.0), ("dropout", 1.0), ("quantum", 1.0)]:
        st = _lib.ScanNoiseParamsStruct()
        built_lib.mrca_scan_noise_default_params(C.byref(st))
        setattr(st, k, v)
        assert call(st) == -1 and b"env is NULL" in built_lib.mrca_last_error(), (k, v, built_lib.mrca_last_error())
    assert call(_lib.ScanNoiseParamsStruct()) == -1 and b"env is NULL" in built_lib.mrca_last_error()
    assert (mask == 7).all()
