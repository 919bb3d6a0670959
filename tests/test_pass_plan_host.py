"""The plan of a run-ahead pass of mrca_step_many (csrc/mrca_pass_plan.h: blocks, ray-cast launches, ring slots, host order),
compiled for the host and checked for every pass length K = 1 .. 256 at T = 1 .. 8 ticks per ray-cast launch: against the
Python restatement the GPU test stands on (pass_plan_ref.launch_plan) and against what mrca_abi.hip's executor and the
kernels rely on -- the ring heads end every pass in the env's field, a block's ray casts wait for an event the host has
already recorded, no launch of several ticks reads the env's own fields except as the pass's last tick."""
import ctypes as C
import os
import subprocess

import pytest

from pass_plan_ref import PASS_TICKS, launch_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
LEAD = 3            # blocks the move launches are enqueued ahead of the ray casts
MAX_T = 8

SHIM = r"""
#include "mrca_pass_plan.h"
extern "C" void pass_plan_constants(int* out) {
    out[0] = mrca::kAheadTicks;
    out[1] = mrca::kRayTicksGroups;
    out[2] = mrca::kMoveLead;
    out[3] = mrca::kOwnTicks;
}
// sizes: [blocks, launches, ops]; first_of [blocks + 1]; launches_of [blocks + 1]; launch [launches + 1][3]; ops [ops][2];
// slots [K][2] (write, read)
extern "C" void pass_plan_shim(int K, int T, int* sizes, int* first_of, int* launches_of, int* launch, int* ops, int* slots) {
    static mrca::PassPlan p;
    mrca::plan_pass(K, T, &p);
    sizes[0] = p.num_blocks;
    sizes[1] = p.num_launches;
    sizes[2] = p.num_ops;
    for (int b = 0; b <= p.num_blocks; ++b) {
        first_of[b] = p.first_of[b];
        launches_of[b] = p.launches_of[b];
    }
    for (int l = 0; l <= p.num_launches; ++l) {
        launch[3 * l] = p.launch[l].first;
        launch[3 * l + 1] = p.launch[l].ticks;
        launch[3 * l + 2] = p.launch[l].heads_in_scratch;
    }
    for (int i = 0; i < p.num_ops; ++i) {
        ops[2 * i] = p.ops[i].kind == mrca::PassPlan::kMoves ? 0 : p.ops[i].kind == mrca::PassPlan::kRays ? 1 : -1;
        ops[2 * i + 1] = p.ops[i].block;
    }
    for (int k = 0; k < K; ++k) {
        slots[2 * k] = p.write_slot(k);
        slots[2 * k + 1] = p.read_slot(k);
    }
}
extern "C" int ticks_per_launch_shim(int lazy_obs, int ring_ticks, int forced, int raster, int W, int R, int P) {
    return mrca::ticks_per_launch(lazy_obs, ring_ticks, forced != 0, raster != 0, W, R, P);
}
"""


class Plan:
    def __init__(self, K, T, first_of, launches_of, launches, heads_after, ops, write_slot, read_slot):
        self.K, self.T = K, T
        self.first_of = first_of            # [blocks + 1]
        self.launches_of = launches_of      # [blocks + 1]
        self.launches = launches            # (first tick, ticks, heads in scratch)
        self.heads_after = heads_after      # where the ring heads are after the pass
        self.ops = ops                      # ("moves" | "rays", block)
        self.write_slot, self.read_slot = write_slot, read_slot


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_plan")
    src, so = d / "shim.cpp", d / "libpass_plan.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)],
                   check=True, capture_output=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def plans(lib):
    """every plan, built once"""
    n = PASS_TICKS + 2
    sizes, first_of, launches_of = (C.c_int * 3)(), (C.c_int * n)(), (C.c_int * n)()
    launch, ops, slots = (C.c_int * (3 * n))(), (C.c_int * (4 * n))(), (C.c_int * (2 * n))()
    out = {}
    for K in range(1, PASS_TICKS + 1):
        for T in range(1, MAX_T + 1):
            lib.pass_plan_shim(K, T, sizes, first_of, launches_of, launch, ops, slots)
            nb, nl, no = sizes
            assert 1 <= nb <= K and 1 <= nl <= K and no == 2 * nb, (K, T, nb, nl, no)
            out[K, T] = Plan(K, T, first_of[:nb + 1], launches_of[:nb + 1], [tuple(launch[3 * l:3 * l + 3]) for l in range(nl)],
                             launch[3 * nl + 2], [(("moves", "rays")[ops[2 * i]], ops[2 * i + 1]) for i in range(no)],
                             [slots[2 * k] for k in range(K)], [slots[2 * k + 1] for k in range(K)])
    return out


def test_constants(lib):
    c = (C.c_int * 4)()
    lib.pass_plan_constants(c)
    assert list(c) == [PASS_TICKS, 3 * 2048, LEAD, 1]


def test_launches_equal_the_python_restatement(plans):
    for (K, T), p in plans.items():
        assert [(k, n) for k, n, _h in p.launches] == launch_plan(K, T), (K, T)


def test_launches_tile_the_pass_inside_the_blocks(plans):
    for (K, T), p in plans.items():
        assert p.first_of[0] == 0 and p.first_of[-1] == K and all(a < e for a, e in zip(p.first_of, p.first_of[1:])), (K, T)
        at = 0
        for k, n, _h in p.launches:
            assert k == at and 1 <= n <= T, (K, T, k, n)
            at += n
        assert at == K, (K, T)
        assert len(p.launches) <= K, (K, T)
        # a launch lies inside one block, and launches_of names exactly the launches of each block
        assert p.launches_of[0] == 0 and p.launches_of[-1] == len(p.launches), (K, T)
        for b, (a, e) in enumerate(zip(p.first_of, p.first_of[1:])):
            mine = p.launches[p.launches_of[b]:p.launches_of[b + 1]]
            assert mine and mine[0][0] == a and mine[-1][0] + mine[-1][1] == e, (K, T, b)


def test_ring_heads_alternate_and_end_in_the_env(plans):
    for (K, T), p in plans.items():
        several = 0
        for k, n, in_scratch in p.launches:
            assert in_scratch == several % 2, (K, T, k)
            several += n > 1
        assert several % 2 == 0 and p.heads_after == 0, (K, T, several)


def test_no_more_blocks_than_with_a_launch_per_tick(plans):
    """a block costs every range one wait: at no length of a pass more waits than with a launch per tick"""
    for (K, T), p in plans.items():
        assert len(p.first_of) <= len(plans[K, 1].first_of), (K, T)


def test_host_order(plans):
    """A wait for an event that has not been recorded yet is no wait: the ray casts of a block, which wait for the event behind
    the block's move launches, are enqueued after them -- and the move launches stay LEAD blocks ahead."""
    for (K, T), p in plans.items():
        nb = len(p.first_of) - 1
        for kind in ("moves", "rays"):
            assert [b for what, b in p.ops if what == kind] == list(range(nb)), (K, T, kind)
        at = {op: i for i, op in enumerate(p.ops)}
        for b in range(nb):
            assert at["moves", b] < at["rays", b], (K, T, b)
            if b + LEAD < nb:
                assert at["moves", b + LEAD] < at["rays", b], (K, T, b)


def test_slots(plans):
    for (K, T), p in plans.items():
        assert sorted(p.write_slot) == list(range(K)) and p.write_slot[K - 1] == 0, (K, T)
        assert p.read_slot[0] == 0 and p.read_slot[1:] == p.write_slot[:-1], (K, T)
        # a launch of several ticks reads a descending run of slots; slot 0, the env's own fields, only as the last tick of
        # the launch that ends the pass
        for k, n, _h in p.launches:
            if n > 1:
                run = p.write_slot[k:k + n]
                assert run == list(range(run[0], run[0] - n, -1)), (K, T, k)
                assert 0 not in run[:-1] and (run[-1] == 0) == (k + n == K), (K, T, k)


# (lazy_obs, ring's ticks, forced, raster, worlds, robots per world, ranges) -> ticks per launch; the ring has F = 3 frames
TICKS_CASES = [
    ((0, 3, False, False, 128, 32, 2), 1),      # lazy_obs = 0: a launch per tick ...
    ((0, 3, True, False, 128, 32, 2), 1),       # ... forced or not
    ((0, 2, True, False, 4, 8, 3), 1),
    ((1, 3, False, False, 128, 32, 2), 3),      # 2048 robots per range
    ((1, 3, False, False, 128, 32, 1), 1),      # 4096
    ((1, 3, False, False, 187, 44, 2), 1),      # the larger range: 94 worlds = 4136 robots
    ((1, 3, False, False, 200, 64, 1), 1),      # 12800 robots: the quotient is 0
    ((1, 3, False, False, 4, 8, 3), 3),         # the largest of three ranges: 2 worlds = 16 robots
    ((1, 3, False, True, 128, 32, 2), 1),       # raster mode, not forced ...
    ((1, 3, False, True, 4, 8, 3), 1),
    ((1, 3, True, True, 128, 32, 2), 3),        # ... forced to 3
    ((1, 3, True, True, 4, 8, 1), 3),
    ((1, 2, True, False, 128, 32, 1), 2),       # forced to 2 at 4096 robots
]


@pytest.mark.parametrize("args,want", TICKS_CASES)
def test_ticks_per_launch(lib, args, want):
    assert lib.ticks_per_launch_shim(*[int(a) for a in args]) == want
