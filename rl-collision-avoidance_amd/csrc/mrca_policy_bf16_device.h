// mrca_policy_bf16_device.h -- the device code of the bf16 lidar front end, shared by its three users: the rollout's
// kernel (mrca_policy_bf16.hip), the update's row-table form (mrca_policy_bf16_rows.hip) and the backward kernel's conv1
// recompute (mrca_policy_bf16_bwd.hip), so that all three form the observation, the weights and h1 with the SAME
// instructions.  The rounding points are stated in mrca_policy_bf16.hip, the LDS image in mrca_policy_bf16_layout.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrca_policy_bf16_layout.h"

namespace mrca_policy_bf16 {

using namespace mrca_pbf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

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
// ... or, through a row table (rows i32[n][3], deque order): the frame store of the rollout buffer read in place
__device__ __forceinline__ void table_rows(const int32_t* __restrict__ rows, int n, int (&r)[3]) {
    r[0] = rows[3 * n];
    r[1] = rows[3 * n + 1];
    r[2] = rows[3 * n + 2];
}
// sx[2 f + h] = x[f][4 m .. 4 m + 3] with m = 64 h + lane
__device__ __forceinline__ void request_rows(float4 (&sx)[6], const float* __restrict__ obs, const int (&r)[3], int lane) {
    const float4* src = reinterpret_cast<const float4*>(obs);
#pragma unroll
    for (int q = 0; q < 6; ++q) sx[q] = src[(size_t)r[q >> 1] * (kBeams / 4) + (q & 1) * 64 + lane];
}
__device__ __forceinline__ void request_scan(float4 (&sx)[6], const float* __restrict__ obs, const uint8_t* __restrict__ head,
                                             int n, int lane) {
    int r[3];
    frame_rows(head, n, r);
    request_rows(sx, obs, r, lane);
}
// rows == NULL: `obs` is [n][3][512] in deque order
__device__ __forceinline__ void request_scan_rows(float4 (&sx)[6], const float* __restrict__ obs, const int32_t* __restrict__ rows,
                                                  int n, int lane) {
    int r[3];
    if (rows) table_rows(rows, n, r);
    else frame_rows(nullptr, n, r);
    request_rows(sx, obs, r, lane);
}

template <bool RAW>
__device__ __forceinline__ float obs_value(float v) {
    return RAW ? norm_scan(fabsf(v)) : v;      // |x|: as mrca_policy.hip (ring rows of ABI 4-5 carried a flag in the sign bit)
}

// the safe policy's scan (mrca_lidar_features_bf16_scaled) exactly as mrca_policy.hip's scale_range: a return at r is seen at
// r s, a beam that returned nothing (6) stays "nothing"; one separately rounded fp32 multiply IN FRONT of rounding point 1
__device__ __forceinline__ float scale_range(float x, float s) { return x < 6.0f ? x * s : x; }
template <bool RAW, bool SCALED>
__device__ __forceinline__ float obs_value_scaled(float v, float s) {
    static_assert(RAW || !SCALED, "only raw ranges can be rescaled");
    return SCALED ? norm_scan(scale_range(fabsf(v), s)) : obs_value<RAW>(v);
}

// The tower's weights as bf16 fragments (rounding point 2), staged coalesced through LDS as fp32 rows of odd pitch: the image
// holds W2L / W1L (mrca_policy_bf16_layout.h) when this returns.  wa1: conv1's A fragments; wb2: conv2's B fragments of the
// forward (w2[col][ci][tap], k = ci).
__device__ __forceinline__ void stage_weights(unsigned char* lds, const float* __restrict__ w1, const float* __restrict__ w2,
                                              int tower, int lane) {
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
}
__device__ __forceinline__ void conv1_weight_fragments(const unsigned char* lds, int col, int hl, bf16x8 (&wa1)[2]) {
    const float* wl = reinterpret_cast<const float*>(lds);
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = conv1_ci(mf, hl, j);
            wa1[mf][j] = (__bf16)(ci < 0 ? 0.0f : wl[kW1L + col * kW1LPitch + ci * 5 + conv1_tap(mf, hl, j)]);
        }
}

// conv2's paddings h1[.][-1] (H row 0) and h1[.][255] (H row 256): nothing else writes them
__device__ __forceinline__ void zero_h_paddings(unsigned char* lds, int lane) {
    if (lane < 8) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(lds + (lane < 4 ? 0 : (kHRows - 1) * kHRowBytes) + 16 * (lane & 3)) = z;
    }
}

// the scan -> X (rounding point 1); X[0] = x[.][-1] = 0.  (X overlaps the previous robot's H rows, all read.)
// SCALED: every range of the three frames times `sc`, the robot's factor (else `sc` is not read)
template <bool RAW, bool SCALED = false>
__device__ __forceinline__ void stage_scan(unsigned char* lds, const float4 (&sx)[6], int lane, float sc = 1.0f) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = 64 * h + lane;
        const float a[4] = {sx[h].x, sx[h].y, sx[h].z, sx[h].w};
        const float b[4] = {sx[2 + h].x, sx[2 + h].y, sx[2 + h].z, sx[2 + h].w};
        const float c[4] = {sx[4 + h].x, sx[4 + h].y, sx[4 + h].z, sx[4 + h].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bf16x4 v;
            v[0] = (__bf16)obs_value_scaled<RAW, SCALED>(a[e], sc);
            v[1] = (__bf16)obs_value_scaled<RAW, SCALED>(b[e], sc);
            v[2] = (__bf16)obs_value_scaled<RAW, SCALED>(c[e], sc);
            v[3] = (__bf16)0.0f;
            *reinterpret_cast<bf16x4*>(lds + x_stage_off(4 * m + e)) = v;
        }
    }
    if (lane == 0) {
        const bf16x4 z = {(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
        *reinterpret_cast<bf16x4*>(lds + x_stage_off(-1)) = z;
    }
}

// conv1: 8 tiles of 32 positions (the last one's position 255 is computed and dropped), two MFMAs each; h1 -> H
// (rounding point 3)
__device__ __forceinline__ void conv1_to_h(unsigned char* lds, const bf16x8 (&wa1)[2], const float (&bias1)[16], int col, int hl) {
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
            for (int g = 0; g < 4; ++g) {
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (__bf16)relu(acc[4 * g + e]);
                *reinterpret_cast<bf16x4*>(lds + h1_store_off(p, g, hl)) = v;
            }
        }
    }
}

// One persistent wave of the forward: wave `gwave` of `nwaves` (even: a wave keeps its tower) walks the robots
// gwave / 2, gwave / 2 + nwaves / 2, ...  TABLE: the scans come through a row table (`rows`; `head` unused), else from
// a ring / deque tensor (`head`; `rows` unused).  SCALED (RAW ring form): robot n's ranges times scale[n]; the factor of the
// next robot is fetched WITH its frame rows, when its scan is requested.
template <bool RAW, bool TABLE, bool SCALED = false>
__device__ __forceinline__ void front_end_wave(unsigned char* lds, const float* __restrict__ obs, const uint8_t* __restrict__ head,
                                               const int32_t* __restrict__ rows, int n_robots, const float* __restrict__ w1,
                                               const float* __restrict__ b1, const float* __restrict__ w2,
                                               const float* __restrict__ b2, uint16_t* __restrict__ feat, int gwave, int nwaves,
                                               const float* __restrict__ scale = nullptr) {
    const int lane = threadIdx.x;
    const int tower = gwave & 1;
    const int col = lane & 31, hl = lane >> 5;

    bf16x8 wa1[2], wb2[6];
    stage_weights(lds, w1, w2, tower, lane);
    conv1_weight_fragments(lds, col, hl, wa1);
    {
        const float* wl = reinterpret_cast<const float*>(lds);
#pragma unroll
        for (int s = 0; s < 6; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) wb2[s][j] = (__bf16)wl[col * kW2LPitch + conv2_ci(s, hl, j) * 3 + conv2_tap(s)];
    }
    float bias1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias1[r] = b1[tower * 32 + rowmap(r, hl)];
    const float bias2 = b2[tower * 32 + col];

    zero_h_paddings(lds, lane);

    const int stride = nwaves >> 1;
    int n = gwave >> 1;
    if (n >= n_robots) return;       // wave-uniform; the kernel has no barrier
    float4 sx[6];
    if (TABLE) request_scan_rows(sx, obs, rows, n, lane);
    else request_scan(sx, obs, head, n, lane);
    float sc = 1.0f;                 // the factor of the robot whose scan sits in sx
    if (SCALED) sc = scale[n];

    for (; n < n_robots; n += stride) {
        stage_scan<RAW, SCALED>(lds, sx, lane, sc);
        if (n + stride < n_robots) {
            if (SCALED) sc = scale[n + stride];      // (this robot's scan is staged: sc is free; issued beside the head's load)
            if (TABLE) request_scan_rows(sx, obs, rows, n + stride, lane);
            else request_scan(sx, obs, head, n + stride, lane);
        }

        conv1_to_h(lds, wa1, bias1, col, hl);

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
// the CU count of the current device, asked once per device; < 0: hipGetDevice failed
static inline int device_cus(DeviceInfo (&table)[64]) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    DeviceInfo& d = table[dev];
    if (d.cus == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        d.cus = cus;
    }
    return d.cus;
}

}  // namespace mrca_policy_bf16
