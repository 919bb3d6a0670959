// mrca_scatter.hip -- the scenario sampler (mrca_scatter): one launch, one WORKGROUP per world.
// The rule is mrca_scatter_device.h's; what is decided here is who computes what.
//
// The order over a world's robots is serial by definition (robot i keeps its distance from every j < i), and it stays inside
// the workgroup: a loop over i with a barrier per robot.  The parallelism is over CANDIDATES: in round r lane l tries
// candidate k = r * blockDim + l -- one Philox block, one byte of the cell field, then the points placed so far out of LDS,
// every lane reading the same address (a broadcast, no bank conflict).  The wave's lowest passing lane is the lowest bit of
// ONE ballot; the workgroup's least k is the minimum of the waves' through LDS.  A minimum does not care for order, so any
// schedule gives the sequential definition's answer.  Rounds go on until a candidate passes or r * blockDim >= max_tries; a
// lane with k >= max_tries never passes.  The start phase runs first and stores to poses_dev; the goal phase reuses the LDS
// array for the goals placed and reads only its own start besides (the workgroup's own store, behind a barrier).
// No grid barrier, no waiting on the device, no atomics; the kernel writes its three output buffers and nothing of the env.
#include <limits.h>

#include "mrca_scatter.h"

namespace mrca {

namespace {

struct ScatterArgs {
    int32_t R;
    uint32_t key0, key1;
    GridGeom g;
    const uint8_t* cellfield;
    const float* boxes;     // [R,8]
    float* poses;           // [N,3]
    float* goals;           // [N,2]
    int32_t* tries;         // [N,2] or nullptr
    ScatterParams p;
};

template <int kBlock> __global__ __launch_bounds__(kBlock) void scatter_kernel(const ScatterArgs a) {
    extern __shared__ ScatterXY placed[];                // [R]
    constexpr int kWaves = kBlock / kWave;
    __shared__ int wave_least[2][kWaves];                // per round parity: one barrier per round is enough (a wave reaches the
                                                         // second write of a parity only behind the barrier of the round between)
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R, w = blockIdx.x;
    const ScatterParams p = a.p;
    const float min2 = p.min_sep * p.min_sep, sep2 = p.goal_sep * p.goal_sep;
    const float lo2 = p.goal_min * p.goal_min, hi2 = p.goal_max * p.goal_max;
    int parity = 0;

    for (int phase = 0; phase < 2; ++phase) {
        const uint32_t word = phase ? kStreamScatterGoal : kStreamScatterStart;
        const float apart2 = phase ? sep2 : min2;
        for (int i = 0; i < R; ++i) {
            const size_t n = (size_t)w * (size_t)R + (size_t)i;
            const uint32_t gid = (uint32_t)n;
            float box[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) box[c] = a.boxes[8 * i + 4 * phase + c];
            // the robot's own start: this workgroup's store of the start phase (a barrier stands behind every robot)
            const float sx = phase ? a.poses[3 * n] : 0.0f, sy = phase ? a.poses[3 * n + 1] : 0.0f;
            int found = INT_MAX;
            for (int base = 0; base < p.max_tries && found == INT_MAX; base += kBlock) {
                const int k = base + tid;
                const ScatterCandidate c = scatter_candidate(box, gid, p.draw, (uint32_t)k, word, a.key0, a.key1);
                bool ok = k < p.max_tries && scatter_clear(a.cellfield, a.g, p.clear_cells, c.x, c.y);
                if (phase) ok = ok && scatter_in_band(c.x, c.y, sx, sy, lo2, hi2);
                // The placed points, kChunk at a time: the LDS reads of a chunk are in flight together, and a wave leaves once none
                // of its candidates is left standing (a wave-uniform trip count).  `ok` is the AND over every j < i either way.
                constexpr int kChunk = 8;
                for (int j = 0; j < i && __ballot(ok) != 0ull; j += kChunk) {
                    ScatterXY q[kChunk];
#pragma unroll
                    for (int u = 0; u < kChunk; ++u) q[u] = placed[min(j + u, i - 1)];
#pragma unroll
                    for (int u = 0; u < kChunk; ++u) ok = ok & ((j + u >= i) | scatter_apart(c.x, c.y, q[u], apart2));
                }
                const unsigned long long pass = __ballot(ok);
                const int least = pass ? base + (wave << 6) + __builtin_ctzll(pass) : INT_MAX;
                if (kWaves == 1) {
                    found = least;
                } else {
                    if (lane == 0) wave_least[parity][wave] = least;
                    __syncthreads();
                    int m = INT_MAX;
#pragma unroll
                    for (int v = 0; v < kWaves; ++v) m = min(m, wave_least[parity][v]);
                    found = m;
                    parity ^= 1;
                }
            }
            // the winner, or candidate max_tries - 1 as it is: one more draw, the same in every lane
            const ScatterCandidate c =
                scatter_candidate(box, gid, p.draw, (uint32_t)(found == INT_MAX ? p.max_tries - 1 : found), word, a.key0, a.key1);
            __syncthreads();       // every lane is done reading placed[] (and the start of robot i) before anything moves on
            if (tid == 0) {
                placed[i] = ScatterXY{c.x, c.y};
                if (phase) {
                    a.goals[2 * n] = c.x;
                    a.goals[2 * n + 1] = c.y;
                } else {
                    a.poses[3 * n] = c.x;
                    a.poses[3 * n + 1] = c.y;
                    a.poses[3 * n + 2] = c.th;
                }
                if (a.tries) a.tries[2 * n + phase] = found == INT_MAX ? -1 : found + 1;
            }
            __syncthreads();       // placed[i] and the stores stand before robot i + 1 (and the goal phase) reads them
        }
    }
}

}  // namespace

void launch_scatter(const EnvView& e, const ScatterParams& p, const float* boxes, float* poses, float* goals, int32_t* tries,
                    hipStream_t s) {
    ScatterArgs a;
    a.R = e.R;
    a.key0 = e.key0; a.key1 = e.key1;
    a.g = e.g;
    a.cellfield = e.cellfield;
    a.boxes = boxes; a.poses = poses; a.goals = goals; a.tries = tries;
    a.p = p;
    const size_t lds = (size_t)e.R * sizeof(ScatterXY);
    if (e.R <= kWave) hipLaunchKernelGGL(scatter_kernel<64>, dim3(e.W), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(scatter_kernel<256>, dim3(e.W), dim3(256), lds, s, a);
}

}  // namespace mrca
