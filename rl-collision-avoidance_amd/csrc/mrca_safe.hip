// mrca_safe.hip -- hybrid control in the paper's form (mrca_hybrid_plan, mrca_hybrid_commit).  The rule is
// mrca_safe_device.h's; what is decided here is who computes what.
//
// PLAN: one launch, one WAVEFRONT per robot, four per workgroup -- the read pattern, the butterfly and the wave-uniform robot
// index of hybrid_kernel (mrca_hybrid.hip): in round k lane l owns beam 64 k + l, a lane folds its beams into its own partial
// minima and count, one butterfly merges the 64 partial results, lane 0 writes mode, scale, pid and the clearances with
// ordinary vector stores.  It reads no command.  No atomics, no LDS, no barrier, no scratch, nothing of the env written.
// The arguments are 104 bytes (the env's fields come through its device-side view, all but the goal: MRCA_F_LOCAL_GOAL or the
// caller's rows, mrca_hybrid_plan_goal), not above the 104 beyond which a launch gets
// dearer for the host (include/mrca_env.h at mrca_create).
//
// COMMIT: one thread per robot, a handful of loads, a select and one 8-byte store.
#include "mrca_safe.h"

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

__global__ __launch_bounds__(kBlock) void hybrid_plan_kernel(const EnvView* __restrict__ view_p, const HybridParams q, const SafeParams sp,
                                                             const int32_t N, const float* __restrict__ goal,
                                                             const uint8_t* __restrict__ mask, int32_t* __restrict__ mode, float* __restrict__ scale,
                                                             float* __restrict__ pid, float* __restrict__ clear) {
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
        int m;
        float s, pv, pw;
        safe_plan_result(q, sp, rb, acc, &m, &s, &pv, &pw);
        mode[n] = m;
        scale[n] = s;
        *reinterpret_cast<float2*>(pid + 2 * (size_t)n) = make_float2(pv, pw);
        if (clear) {
            clear[3 * (size_t)n] = acc.d_min;
            clear[3 * (size_t)n + 1] = acc.d_front;
            clear[3 * (size_t)n + 2] = acc.d_block;
        }
    }
}

// (policy and actions may be one buffer: neither is __restrict__, and a thread reads its robot's row before it writes it)
__global__ __launch_bounds__(kBlock) void hybrid_commit_kernel(const int32_t N, const SafeParams sp, const uint8_t* __restrict__ mask,
                                                               const int32_t* __restrict__ mode, const float* __restrict__ pid,
                                                               const float* policy, float* actions) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    if (mask && !mask[n]) return;
    const float vp = policy[2 * (size_t)n], wp = policy[2 * (size_t)n + 1];
    const float2 p = *reinterpret_cast<const float2*>(pid + 2 * (size_t)n);
    float v, w;
    safe_commit(sp, mode[n], vp, wp, p.x, p.y, &v, &w);
    *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(v, w);
}

}  // namespace

void launch_hybrid_plan(const EnvView& e, const HybridParams& p, const SafeParams& sp, const float* goal, const uint8_t* mask, int32_t* mode, float* scale,
                        float* pid, float* clear, hipStream_t s) {
    hipLaunchKernelGGL(hybrid_plan_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, e.dev, p, sp,
                       (int32_t)e.N, goal ? goal : e.local_goal, mask, mode, scale, pid, clear);
}

void launch_hybrid_commit(int32_t n_robots, const SafeParams& sp, const uint8_t* mask, const int32_t* mode, const float* pid,
                          const float* policy, float* actions, hipStream_t s) {
    hipLaunchKernelGGL(hybrid_commit_kernel, dim3((n_robots + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n_robots, sp, mask, mode, pid,
                       policy, actions);
}

}  // namespace mrca
