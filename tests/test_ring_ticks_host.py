"""The parts ring_rule (csrc/mrca_device.h) is made of -- ring_ticks (what hangs on the launch's fresh flags, j and T alone:
wave-uniform on the device), ring_wrap and ring_fresh_stores (what hangs on the head) -- and the two fields the ray cast of
several ticks takes from the rule instead of recovering them from the store mask: ``slot`` and ``any``.  The kernel
(csrc/mrca_raycast_body.h) composes the parts itself, so each is swept here on the host against a replay of the sequential rule
(a fresh tick writes all F slots and leaves the head; any other tick advances the head and writes that slot) for every ring size
F <= 8, launch length T <= F, head, pattern of restarts and tick j -- once through a shared object and once as a stand-alone
program built with -fsanitize=undefined (the closed form is shifts by run-time amounts)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")

SHIM = r"""
#include <stdint.h>
#include "mrca_device.h"
extern "C" void ring_ticks_shim(int T, uint32_t fresh_bits, int j, int* out) {
    const mrca::RingTicks u = mrca::ring_ticks(T, fresh_bits, j);
    out[0] = u.stale_to_j; out[1] = u.stale; out[2] = u.fresh; out[3] = u.later;
}
extern "C" int ring_wrap_shim(int h, int F) { return mrca::ring_wrap(h, F); }
extern "C" uint32_t ring_fresh_stores_shim(int F, int slot, int m) { return mrca::ring_fresh_stores(F, slot, m); }
extern "C" void ring_rule_shim(int F, int T, int h0, uint32_t fresh_bits, int j, int* out) {
    const mrca::RingStores r = mrca::ring_rule(F, T, h0, fresh_bits, j);
    out[0] = (int)r.stores; out[1] = r.head; out[2] = r.slot; out[3] = r.any;
}
"""

# the same sweep with no Python in the process: every case against the loop over the launch's ticks the closed form replaced
MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include "mrca_device.h"
int main() {
    long cases = 0;
    for (int F = 1; F <= 8; ++F)
        for (int T = 1; T <= F; ++T)
            for (int h0 = 0; h0 < F; ++h0)
                for (uint32_t bits = 0; bits < (1u << T); ++bits)
                    for (int j = 0; j < T; ++j)
                        for (uint32_t high = 0; high < 2; ++high) {      // (bits T and up are ignored)
                            const uint32_t all = (1u << F) - 1u;
                            int h = h0, hj = h0;
                            uint32_t mine = 0u, later = 0u;
                            for (int t = 0; t < T; ++t) {
                                const bool fresh = ((bits >> t) & 1u) != 0u;
                                h = fresh ? h : (h + 1 == F ? 0 : h + 1);
                                const uint32_t w = fresh ? all : 1u << h;
                                if (t == j) { mine = w; hj = h; }
                                if (t > j) later |= w;
                            }
                            const mrca::RingStores r = mrca::ring_rule(F, T, h0, bits | (high ? 0xffffffffu << T : 0u), j);
                            if (r.stores != (mine & ~later) || r.head != h || r.slot != hj || r.any != (r.stores != 0u)) {
                                printf("F %d T %d h0 %d bits %u j %d: stores %u head %d slot %d any %d\n", F, T, h0, bits, j, r.stores,
                                       r.head, r.slot, (int)r.any);
                                return 1;
                            }
                            ++cases;
                        }
    printf("%ld\n", cases);
    return 0;
}
"""


def sequential(F, T, h0, fresh_bits):
    """the rule tick after tick -> per tick (head after it, slots it writes), the head after the launch"""
    ticks, h = [], h0
    for t in range(T):
        if (fresh_bits >> t) & 1:
            ticks.append((h, set(range(F))))
        else:
            h = (h + 1) % F
            ticks.append((h, {h}))
    return ticks, h


def cases():
    for F in range(1, 9):
        for T in range(1, F + 1):
            for h0 in range(F):
                for fresh_bits in range(1 << T):
                    yield F, T, h0, fresh_bits


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ring_ticks")
    src, so = d / "shim.cpp", d / "libring_ticks.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True, capture_output=True)
    lib = C.CDLL(str(so))
    lib.ring_ticks_shim.argtypes = [C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    lib.ring_wrap_shim.argtypes = [C.c_int, C.c_int]
    lib.ring_fresh_stores_shim.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ring_fresh_stores_shim.restype = C.c_uint32
    lib.ring_rule_shim.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    return lib


def test_uniform_part_counts_stale_ticks_and_finds_restarts(lib):
    out = (C.c_int * 4)()
    for T in range(1, 9):
        for fresh_bits in range(1 << T):
            for j in range(T):
                for high in (0, 0xffffffff << T & 0xffffffff):        # bits T and up are ignored
                    lib.ring_ticks_shim(T, fresh_bits | high, j, out)
                    stale_to_j = sum(1 for t in range(j + 1) if not (fresh_bits >> t) & 1)
                    stale = sum(1 for t in range(T) if not (fresh_bits >> t) & 1)
                    want = [stale_to_j, stale, (fresh_bits >> j) & 1, int(fresh_bits >> (j + 1) != 0)]
                    assert list(out) == want, (T, fresh_bits, j, high, list(out), want)


def test_wrap_is_one_conditional_subtract(lib):
    # what the rule feeds it: h0 < F plus at most T <= F stale ticks
    for F in range(1, 9):
        for h in range(2 * F):
            assert lib.ring_wrap_shim(h, F) == h % F, (F, h)


def test_fresh_tick_stores_all_but_the_slots_behind_its_head(lib):
    for F in range(1, 9):
        for slot in range(F):
            for m in range(F):         # m = T - 1 - j <= F - 1 later ticks, none of them fresh
                want = sum(1 << s for s in set(range(F)) - {(slot + 1 + q) % F for q in range(m)})
                assert lib.ring_fresh_stores_shim(F, slot, m) == want, (F, slot, m)


def test_rule_names_the_slot_and_whether_it_stores(lib):
    out = (C.c_int * 4)()
    n = 0
    for F, T, h0, fresh_bits in cases():
        ticks, head = sequential(F, T, h0, fresh_bits)
        for j in range(T):
            lib.ring_rule_shim(F, T, h0, fresh_bits, j, out)
            stores, got_head, slot, any_ = out[0], out[1], out[2], out[3]
            later = set().union(*[w for _h, w in ticks[j + 1:]]) if j + 1 < T else set()
            want = ticks[j][1] - later
            assert stores == sum(1 << s for s in want), (F, T, h0, fresh_bits, j)
            assert got_head == head and slot == ticks[j][0], (F, T, h0, fresh_bits, j)
            assert any_ == int(bool(want)), (F, T, h0, fresh_bits, j)
            # what the kernel relies on: a stale tick's one slot is `slot`; the launch's last tick leaves `slot` as the head;
            # a tick stores nothing exactly when a later tick of the launch is fresh
            if not (fresh_bits >> j) & 1:
                assert want in (set(), {slot}), (F, T, h0, fresh_bits, j)
            if j == T - 1:
                assert slot == head, (F, T, h0, fresh_bits, j)
            assert bool(want) == (fresh_bits >> (j + 1) == 0), (F, T, h0, fresh_bits, j)
            n += 1
    assert n == sum(F * (1 << T) * T for F in range(1, 9) for T in range(1, F + 1))


def test_sweep_as_a_program_under_the_undefined_behaviour_sanitizer(tmp_path):
    src, exe = tmp_path / "main.cpp", tmp_path / "ring_rule_sweep"
    src.write_text(MAIN)
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout[-400:], run.stderr[-400:])
    assert int(run.stdout) == 2 * sum(F * (1 << T) * T for F in range(1, 9) for T in range(1, F + 1))
