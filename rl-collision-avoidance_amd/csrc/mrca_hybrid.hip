// mrca_hybrid.hip -- the hybrid control wrapper (mrca_hybrid_actions): one launch, one WAVEFRONT per robot.
// The rule is mrca_hybrid_device.h's; what is decided here is who computes what.
//
// In round k lane l owns beam 64 k + l: a round reads 256 contiguous bytes of the row (and of each beam table, which every
// wave reads alike).  A lane folds its beams into its own partial minima and count; ONE butterfly over the wave merges the 64
// partial results -- minima of values without a -0.0 and a sum of integers, so which lane held which beam cannot show -- and
// lane 0 writes the command, the mode and the three clearances with ordinary vector stores.  What is the same for a robot
// (its head, its goal) is loaded once and made wave-uniform.  No atomics, no LDS, no barrier, no scratch, nothing of the env
// written.
//
// The arguments are 96 bytes: the env's fields come through its device-side view (as in the two kernels of the tick) -- all but
// the goal, a pointer of its own (MRCA_F_LOCAL_GOAL, or the caller's rows: mrca_hybrid_actions_goal) -- so that
// the nine params fit beside the six pointers below the 104 bytes at which a launch gets dearer for the host
// (include/mrca_env.h at mrca_create).
#include "mrca_hybrid.h"

namespace mrca {

namespace {

constexpr int kBlock = 256;
constexpr int kRobotsPerBlock = kBlock / kWave;

__device__ __forceinline__ HybridAcc wave_merge(HybridAcc a) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        HybridAcc b;
        b.d_min = __shfl_xor(a.d_min, o);
        b.d_front = __shfl_xor(a.d_front, o);
        b.d_block = __shfl_xor(a.d_block, o);
        b.n_block = __shfl_xor(a.n_block, o);
        a = hybrid_acc_merge(a, b);
    }
    return a;
}

// (policy and actions may be one buffer: neither is __restrict__, and lane 0 reads its robot's row before it writes it)
__global__ __launch_bounds__(kBlock) void hybrid_kernel(const EnvView* __restrict__ view_p, const HybridParams q, const int32_t N,
                                                        const float* __restrict__ goal, const uint8_t* __restrict__ mask, const float* policy, float* actions,
                                                        int32_t* __restrict__ mode, float* __restrict__ clear) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x * kRobotsPerBlock + wave;
    if (n >= N) return;                      // (wave-uniform, like every branch around the shuffles below)
    if (mask && !mask[n]) return;
    const EnvView& e = *view_p;
    const int B = e.B, F = e.F;
    const int head = __builtin_amdgcn_readfirstlane((int)e.ring_head[n]);
    if (head >= F) return;                   // (never in an env the library keeps: a head outside the ring must not become an address)

    const HybridRobot rb = hybrid_robot_begin(q, goal[2 * (size_t)n], goal[2 * (size_t)n + 1]);
    const float* row = e.scan_ring + ((size_t)n * (size_t)F + (size_t)head) * (size_t)B;
    const float* bc = e.beam_cos;
    const float* bs = e.beam_sin;
    HybridAcc acc = hybrid_acc_empty();
    for (int b = lane; b < B; b += kWave) hybrid_beam(q, rb, row[b], bc[b], bs[b], &acc);
    acc = wave_merge(acc);

    if (lane == 0) {
        const float vp = policy[2 * (size_t)n], wp = policy[2 * (size_t)n + 1];
        float v, w;
        int m;
        hybrid_result(q, rb, acc, vp, wp, &v, &w, &m);
        *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(v, w);
        if (mode) mode[n] = m;
        if (clear) {
            clear[3 * (size_t)n] = acc.d_min;
            clear[3 * (size_t)n + 1] = acc.d_front;
            clear[3 * (size_t)n + 2] = acc.d_block;
        }
    }
}

}  // namespace

void launch_hybrid(const EnvView& e, const HybridParams& p, const float* goal, const uint8_t* mask, const float* policy, float* actions, int32_t* mode,
                   float* clear, hipStream_t s) {
    hipLaunchKernelGGL(hybrid_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, e.dev, p, (int32_t)e.N,
                       goal ? goal : e.local_goal, mask,
                       policy, actions, mode, clear);
}

}  // namespace mrca
