"""The preparing wave's prefix sum over the lanes as the device runs it (csrc/mrca_device.h: kLaneScanNet, six DPP steps over four
rows of 16 lanes), through the header's plain model of such a network (lane_scan_network), compiled into a stand-alone program
and held to std::partial_sum on 64 lanes:

  * all zeros; one non-zero lane at each of 0, 15, 16, 31, 32, 47, 48 and 63 (the first and last lane of every row); all lanes 512
    (the largest interval); 4000 seeded random length vectors with random runs of zeros (dropped candidates);
  * the same inputs against the network's neighbours -- each step dropped in turn, each broadcast with a wrong row mask, each
    broadcast out of lane 16 resp. 32 of the lanes below instead of 15 resp. 31 (the row's own first lane), a shift one lane off --:
    every mutant must differ from the partial sum somewhere, which shows that the inputs can tell the network from them.

The program prints one line per network: its name and the number of inputs it got wrong.  It is built with g++'s address and
undefined-behaviour sanitizers (host code only, its own main)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")

MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <numeric>
#include <string>
#include <vector>
#include "mrca_device.h"

using mrca::LaneScanStep;

static std::vector<std::vector<int>> inputs() {
    std::vector<std::vector<int>> in;
    in.push_back(std::vector<int>(64, 0));
    for (int lane : {0, 15, 16, 31, 32, 47, 48, 63})
        for (int v : {1, 512}) {
            std::vector<int> x(64, 0);
            x[lane] = v;
            in.push_back(x);
        }
    in.push_back(std::vector<int>(64, 512));
    uint32_t rnd = 2026u;
    auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd >> 8; };
    for (int k = 0; k < 4000; ++k) {
        std::vector<int> x(64);
        for (int l = 0; l < 64;) {
            const bool zeros = next() % 3u == 0u;             // a run of dropped candidates, or of kept ones
            int run = 1 + (int)(next() % 20u);
            for (; run > 0 && l < 64; --run, ++l) x[l] = zeros ? 0 : 1 + (int)(next() % 512u);
        }
        in.push_back(x);
    }
    return in;
}

// the inputs a network gets wrong
static long wrong(const LaneScanStep* net, int steps, const std::vector<std::vector<int>>& in) {
    long bad = 0;
    for (const auto& x : in) {
        int want[64], got[64];
        std::partial_sum(x.begin(), x.end(), want);
        memcpy(got, x.data(), sizeof got);
        mrca::lane_scan_network(net, steps, got);
        bad += memcmp(want, got, sizeof want) != 0;
    }
    return bad;
}

int main() {
    const auto in = inputs();
    const int S = mrca::kLaneScanSteps;
    printf("inputs %zu\n", in.size());
    printf("network %ld\n", wrong(mrca::kLaneScanNet, S, in));
    for (int drop = 0; drop < S; ++drop) {
        LaneScanStep net[8];
        int n = 0;
        for (int i = 0; i < S; ++i) if (i != drop) net[n++] = mrca::kLaneScanNet[i];
        printf("mutant dropped_step_%d %ld\n", drop, wrong(net, n, in));
    }
    for (int i = 0; i < S; ++i) {
        LaneScanStep net[8];
        memcpy(net, mrca::kLaneScanNet, sizeof(LaneScanStep) * S);
        if (net[i].span) {
            for (unsigned rows : {0x8u, 0x2u, 0x4u, 0x6u, net[i].rows ^ 0xfu}) {
                net[i].rows = rows;
                printf("mutant step_%d_rows_%x %ld\n", i, rows, wrong(net, S, in));
            }
            net[i] = mrca::kLaneScanNet[i];
            net[i].shift += 1;                                 // lane 16 (32) of the lanes below: the row's (half's) own first lane
            printf("mutant step_%d_broadcast_from_%d %ld\n", i, net[i].shift, wrong(net, S, in));
            net[i].shift -= 2;
            printf("mutant step_%d_broadcast_from_%d %ld\n", i, net[i].shift, wrong(net, S, in));
        } else {
            net[i].shift += 1;
            printf("mutant step_%d_shift_%d %ld\n", i, net[i].shift, wrong(net, S, in));
            net[i] = mrca::kLaneScanNet[i];
            net[i].rows = 0x7u;
            printf("mutant step_%d_rows_7 %ld\n", i, wrong(net, S, in));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_scan")
    src, exe = d / "main.cpp", d / "prep_scan"
    src.write_text(MAIN)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout[-400:], run.stderr[-800:])
    return [line.split() for line in run.stdout.splitlines()]


def test_the_network_is_the_inclusive_sum_over_the_lanes(report):
    head = {r[0]: r[1:] for r in report if r[0] != "mutant"}
    assert int(head["inputs"][0]) == 1 + 16 + 1 + 4000
    assert int(head["network"][0]) == 0


def test_the_inputs_tell_the_network_from_its_neighbours(report):
    mutants = {r[1]: int(r[2]) for r in report if r[0] == "mutant"}
    # a step dropped (six), a wrong row mask (five per broadcast, one per shift), a broadcast out of another lane, a shift off by one
    assert sum(k.startswith("dropped_step_") for k in mutants) == 6
    assert sum("_rows_" in k for k in mutants) == 2 * 5 + 4
    assert {"step_4_broadcast_from_16", "step_4_broadcast_from_14", "step_5_broadcast_from_32", "step_5_broadcast_from_30"} <= set(mutants)
    assert sum("_shift_" in k for k in mutants) == 4
    passed = sorted(k for k, bad in mutants.items() if bad == 0)
    assert not passed, f"the inputs cannot tell these from the network: {passed}"
