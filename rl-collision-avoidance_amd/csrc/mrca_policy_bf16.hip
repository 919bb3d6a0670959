// mrca_policy_bf16.hip -- the lidar front end of both towers (the function of lidar_features_kernel, mrca_policy.hip) on
// bf16 MFMAs: the opt-in bf16 rollout inference (mrca_lidar_features_bf16, include/mrca_env.h).  fp32 stays the default.
//
// Rounding points (the numerical contract; tests/test_policy_bf16_layout.py and tests/test_gpu_policy_bf16.py check it):
//   1. raw ranges become x / 6 - 0.5 in fp32 exactly as norm_scan (mrca_policy.hip) forms them; the observation is rounded
//      to bf16 (round to nearest even)
//   2. w1, w2 are rounded to bf16 (RNE); b1, b2 stay fp32 and are added to the fp32 accumulators
//   3. h1 = relu(conv1 + b1) is rounded to bf16 (RNE) -- conv2's operand, it never leaves the CU
//   4. feat = relu(conv2 + b2) is rounded to bf16 (RNE) and stored
// Every rounding is a plain (__bf16) cast: v_cvt_pk_bf16_f32, RNE, NaN kept.  The products of two bf16 are exact in the
// fp32 accumulators of v_mfma_f32_32x32x16_bf16; only the order of their summation is the hardware's.
//
// Bound: per robot 6 KB of scans in and 16 KB of features out (2 x 4096 bf16) -- 92 MB at 4096 robots, ~11.5 us at HBM
// rate -- against 16 + 24 = 40 MFMAs of 32 cycles per (robot, tower), ~4.3 us of matrix work per SIMD (conv1 takes two MFMAs
// per tile, not one: its K of 15 is laid out as 5 taps x 4 channels so that every operand is one aligned LDS read).  So the kernel is
// written for HBM, not for the matrix pipe (the fp32 kernel's one wave per SIMD and its software pipeline are not needed):
//   * one wave owns one (robot, tower) at a time and its LDS image is 16 448 B (mrca_policy_bf16_layout.h: the scan lives
//     inside the h1 image, the output transposition too), so 2 waves per SIMD are resident and hide each other's latency;
//   * persistent waves keep the tower's bf16 weights in registers; the next robot's scan is requested as soon as the
//     current one is staged;
//   * the output leaves as 16-byte stores per lane (4 channels x 256 contiguous bytes per wave instruction), transposed
//     through LDS: conv2 runs as C[positions][channels] so a lane holds runs of 4 positions of ONE channel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrca_env.h"
#include "mrca_hostutil.h"
#include "mrca_policy_bf16_layout.h"

namespace mrca_policy_bf16 {

using namespace mrca_pbf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int kWavesPerSimd = 2;        // resident by LDS (9 waves per CU fit) and by registers (<= 256 per lane)

#define MRCA_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// as in mrca_policy.hip: relu as one integer max (a negative NaN becomes 0; the layers never produce one from finite inputs)
__device__ __forceinline__ float relu(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

// x / 6 - 0.5 exactly as mrca_policy.hip's norm_scan (and the env's norm_obs) form it
__device__ __forceinline__ float norm_scan(float x) {
    const float inv6 = 1.0f / 6.0f;
    const float q = x * inv6;
    const float r = __builtin_fmaf(-q, 6.0f, x);
    return __builtin_fmaf(r, inv6, q) - 0.5f;
}

// the rows of robot n's three frames behind `obs` (rows of 512 floats), oldest first: a ring with head[n] the newest slot,
// or deque order (head == NULL)
__device__ __forceinline__ void frame_rows(const uint8_t* __restrict__ head, int n, int (&r)[3]) {
    const int hd = head ? head[n] : 2;
    const int s0 = hd == 2 ? 0 : hd + 1, s1 = s0 == 2 ? 0 : s0 + 1;
    r[0] = 3 * n + s0;
    r[1] = 3 * n + s1;
    r[2] = 3 * n + hd;
}
// sx[2 f + h] = x[f][4 m .. 4 m + 3] with m = 64 h + lane
__device__ __forceinline__ void request_scan(float4 (&sx)[6], const float* __restrict__ obs, const uint8_t* __restrict__ head,
                                             int n, int lane) {
    int r[3];
    frame_rows(head, n, r);
    const float4* src = reinterpret_cast<const float4*>(obs);
#pragma unroll
    for (int q = 0; q < 6; ++q) sx[q] = src[(size_t)r[q >> 1] * (kBeams / 4) + (q & 1) * 64 + lane];
}

template <bool RAW>
__device__ __forceinline__ float obs_value(float v) {
    return RAW ? norm_scan(fabsf(v)) : v;      // |x|: as mrca_policy.hip (ring rows of ABI 4-5 carried a flag in the sign bit)
}

template <bool RAW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) void lidar_features_bf16_kernel(
    const float* __restrict__ obs, const uint8_t* __restrict__ head, int n_robots, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, uint16_t* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // one wave per workgroup: kWaveBytes
    const int lane = threadIdx.x;
    const int gwave = blockIdx.x, nwaves = gridDim.x;          // nwaves is even: a wave keeps its tower
    const int tower = gwave & 1;
    const int col = lane & 31, hl = lane >> 5;

    // --- the tower's weights as bf16 fragments (rounding point 2), staged coalesced through LDS as fp32 rows of odd pitch
    bf16x8 wa1[2], wb2[6];
    {
        float* wl = reinterpret_cast<float*>(lds);
        const float4* w2v = reinterpret_cast<const float4*>(w2 + tower * 3072);
        const float4* w1v = reinterpret_cast<const float4*>(w1 + tower * 480);
        float4 t2[12], t1[2];
#pragma unroll
        for (int q = 0; q < 12; ++q) t2[q] = w2v[q * 64 + lane];
        t1[0] = w1v[lane];
        t1[1] = w1v[lane < 56 ? 64 + lane : 64];
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const int f = q * 64 + lane;                      // float4 index: row f / 24, columns 4 (f % 24) ...
            float* d = wl + (f / 24) * kW2LPitch + 4 * (f % 24);
            d[0] = t2[q].x;
            d[1] = t2[q].y;
            d[2] = t2[q].z;
            d[3] = t2[q].w;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q == 0 || lane < 56) {
                const float v[4] = {t1[q].x, t1[q].y, t1[q].z, t1[q].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * (q * 64 + lane) + j;    // element: row e / 15, column e % 15
                    wl[kW1L + (e / 15) * kW1LPitch + e % 15] = v[j];
                }
            }
        }
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ci = conv1_ci(mf, hl, j);
                wa1[mf][j] = (__bf16)(ci < 0 ? 0.0f : wl[kW1L + col * kW1LPitch + ci * 5 + conv1_tap(mf, hl, j)]);
            }
#pragma unroll
        for (int s = 0; s < 6; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) wb2[s][j] = (__bf16)wl[col * kW2LPitch + conv2_ci(s, hl, j) * 3 + conv2_tap(s)];
    }
    float bias1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias1[r] = b1[tower * 32 + rowmap(r, hl)];
    const float bias2 = b2[tower * 32 + col];

    // conv2's paddings h1[.][-1] (H row 0) and h1[.][255] (H row 256): nothing else writes them
    if (lane < 8) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(lds + (lane < 4 ? 0 : (kHRows - 1) * kHRowBytes) + 16 * (lane & 3)) = z;
    }

    const int stride = nwaves >> 1;
    int n = gwave >> 1;
    if (n >= n_robots) return;       // wave-uniform; the kernel has no barrier
    float4 sx[6];
    request_scan(sx, obs, head, n, lane);

    for (; n < n_robots; n += stride) {
        // --- the scan -> X (rounding point 1); X[0] = x[.][-1] = 0.  (X overlaps the previous robot's H rows, all read.)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = 64 * h + lane;
            const float a[4] = {sx[h].x, sx[h].y, sx[h].z, sx[h].w};
            const float b[4] = {sx[2 + h].x, sx[2 + h].y, sx[2 + h].z, sx[2 + h].w};
            const float c[4] = {sx[4 + h].x, sx[4 + h].y, sx[4 + h].z, sx[4 + h].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bf16x4 v;
                v[0] = (__bf16)obs_value<RAW>(a[e]);
                v[1] = (__bf16)obs_value<RAW>(b[e]);
                v[2] = (__bf16)obs_value<RAW>(c[e]);
                v[3] = (__bf16)0.0f;
                *reinterpret_cast<bf16x4*>(lds + x_stage_off(4 * m + e)) = v;
            }
        }
        if (lane == 0) {
            const bf16x4 z = {(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
            *reinterpret_cast<bf16x4*>(lds + x_stage_off(-1)) = z;
        }
        if (n + stride < n_robots) request_scan(sx, obs, head, n + stride, lane);

        // --- conv1: 8 tiles of 32 positions (the last one's position 255 is computed and dropped), two MFMAs each
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int p = 32 * t + col;
            const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(lds + conv1_b_off(0, p, hl));
            const bf16x4 x4 = *reinterpret_cast<const bf16x4*>(lds + conv1_b_off(1, p, 0));
            bf16x8 x1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x1[j] = hl ? (__bf16)0.0f : x4[j];
                x1[4 + j] = (__bf16)0.0f;
            }
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bias1[r];
            acc = MRCA_MFMA_BF16(wa1[0], x0, acc);
            acc = MRCA_MFMA_BF16(wa1[1], x1, acc);
            if (p < kL1) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {        // rounding point 3
                    bf16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (__bf16)relu(acc[4 * g + e]);
                    *reinterpret_cast<bf16x4*>(lds + h1_store_off(p, g, hl)) = v;
                }
            }
        }

        // --- conv2: 4 tiles of 32 positions, 6 k-steps each; C[position][channel]
        f32x16 acc2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int l = 32 * t + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[t][r] = bias2;
#pragma unroll
            for (int s = 0; s < 6; ++s)
                acc2[t] = MRCA_MFMA_BF16(*reinterpret_cast<const bf16x8*>(lds + conv2_a_off(s, l, hl)), wb2[s], acc2[t]);
        }

        // --- out (rounding point 4): runs of 4 positions into O (H is read), rows of 8 positions out as 16-byte stores
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (__bf16)relu(acc2[t][4 * g + e]);
                *reinterpret_cast<bf16x4*>(lds + out_store_off(col, t, g, hl)) = v;
            }
        uint16_t* out = feat + ((size_t)tower * n_robots + n) * (kCh * kL2);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            *reinterpret_cast<u32x4*>(out + out_feat_elem(q, lane)) = *reinterpret_cast<const u32x4*>(lds + out_load_off(q, lane));
    }
}

struct DeviceInfo {
    int cus = 0;
};
static DeviceInfo g_dev[64];

}  // namespace mrca_policy_bf16

extern "C" int mrca_lidar_features_bf16(const float* obs_dev, const uint8_t* obs_head_dev, int32_t raw_scans, int32_t n_robots,
                                        int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev,
                                        const float* w2_dev, const float* b2_dev, uint16_t* feat_dev, void* stream) {
    using namespace mrca_policy_bf16;
    if (!obs_dev || !w1_dev || !b1_dev || !w2_dev || !b2_dev || !feat_dev)
        return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16: NULL pointer");
    if (frames != kFrames || beams != kBeams || n_robots < 1)
        return mrca::set_error(MRCA_ERR_UNSUPPORTED,
                               "mrca_lidar_features_bf16: frames %d beams %d robots %d (needs 3 x 512, >= 1)", frames, beams,
                               n_robots);
    // 16-byte loads of the scans and weights, 16-byte stores of the features
    if ((reinterpret_cast<uintptr_t>(obs_dev) | reinterpret_cast<uintptr_t>(w1_dev) | reinterpret_cast<uintptr_t>(w2_dev) |
         reinterpret_cast<uintptr_t>(feat_dev)) & 15)
        return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16: obs, w1, w2 and feat must be 16-byte aligned");
    mrca::DeviceGuard guard(mrca::device_of(obs_dev));
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16: hipGetDevice failed");
    DeviceInfo& d = g_dev[dev];
    if (d.cus == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        d.cus = cus;
    }
    // persistent one-wave workgroups, (actor, critic) pairs: 4 SIMDs x kWavesPerSimd per CU, no more than there is work for
    int pairs = d.cus * 4 * kWavesPerSimd / 2;
    if (pairs > n_robots) pairs = n_robots;
    const size_t lds = kWaveBytes;
    if (raw_scans)
        hipLaunchKernelGGL(lidar_features_bf16_kernel<true>, dim3(2 * pairs), dim3(64), lds, static_cast<hipStream_t>(stream),
                           obs_dev, obs_head_dev, n_robots, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    else
        hipLaunchKernelGGL(lidar_features_bf16_kernel<false>, dim3(2 * pairs), dim3(64), lds, static_cast<hipStream_t>(stream),
                           obs_dev, obs_head_dev, n_robots, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16 launch: %s", hipGetErrorString(e));
    return MRCA_OK;
}
