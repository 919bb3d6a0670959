// mrca_policy_bf16_bwd.hip -- backward pass of the bf16 lidar front end: the function of mrca_policy_bwd.hip on
// v_mfma_f32_32x32x16_bf16, for the opt-in fused bf16 PPO update (mrca_lidar_features_bf16_backward, include/mrca_env.h).
// fp32 stays the default; this is not the reference's precision.
//
// Per (sample, tower), with x, w1, w2 the bf16-rounded observation and weights of the forward (mrca_policy_bf16.hip):
//   g2[c][l]      = gfeat[c][l] * (feat[c][l] > 0)                                    exact (both bf16)          l < 128
//   h1[ci][p]     = bf16(relu(conv1(x) + b1))  recomputed with the forward's own code (mrca_policy_bf16_device.h)  p < 255
//   dw2[c][ci][k] = sum_{n,l} g2[c][l] * h1[ci][2l + k - 1]      db2[c] = sum_{n,l} g2[c][l]      fp32 sums of exact products
//   dh1[ci][p]    = sum_{c,k : 2l + k - 1 = p} w2[c][ci][k] * g2[c][l]    fp32;   g1 = bf16(dh1 * (h1 > 0))    (rounding point)
//   dw1[c][ci][k] = sum_{n,p} g1[c][p] * x[ci][2p + k - 1]       db1[c] = sum_{n,p} g1[c][p]      fp32 sums of exact products
// The roundings are straight-through; all of them are plain (__bf16) casts (RNE).
//
// One wave owns one (sample, tower) at a time, persistent over the minibatch.  MFMAs per item (C = A x B, 32x32x16):
//   conv1 recompute  16   C[ch][pos]  = W1 x X1                  (conv1_to_h: h1 -> H, position-major, as the forward)
//   conv2 wgrad      24   DW2_k[c][ci] += G2[c][l] x H1_k[l][ci]  K = positions.  A = the lane's own 16 bytes of the gradient row
//                         as loaded from HBM (channel c = lane, 8 consecutive l); B = h1[ci][2l + k - 1] for 8 consecutive l
//                         out of the position-major H: two ds_read_b64_tr_b16 (rows = positions, columns = channels)
//   conv2 dgrad      24   D[pos][ci]  = G2^T x W2_k              K = 32 channels.  Even positions p = 2l: tap 1 (2 MFMAs per
//                         tile of 32); odd positions p = 2l + 1: tap 2 on g2[.][l] and tap 0 on g2[.][l + 1] into ONE
//                         accumulator (4 MFMAs).  A = 16 bytes of GT, the position-major image of g2; B = w2 in registers
//   conv1 wgrad      16   DW1'[(ci,k)][c] += X1[(ci,k)][pos] x G1[pos][c]   K = positions.  dgrad's accumulator tile has the
//                         positions in registers and the channel on the lane: masked by h1 > 0 (one transposed read of H
//                         per 4 positions) and converted pairwise it IS the B operand -- g1 never leaves the registers.
//                         A = two 8-byte reads of XP, the scan de-interleaved by (2p + k - 1) mod 4; row 15 of X1 is ones:
//                         that row of DW1' is db1
//   total            80   (the fp32 kernel: 576)
// HBM per item: 6 KB of scan + 8 KB feat + 8 KB gfeat; 16 384 samples x 2 towers: 720 MB, ~90 us at 8 TB/s, against ~34 us
// of matrix time -- HBM-bound, so the kernel keeps no software pipeline: it counts on several resident waves per CU.
// LDS per wave: H (16 448 B, holds the scan X too) + GT (8 256 B) + XP (5 376 B) = 30 080 B: 5 waves per CU, so one SIMD
// holds 2: kWavesPerSimd = 2, at most 256 registers per lane.
// Per-wave fp32 partial sums go to a scratch buffer; lidar_features_bf16_bwd_finalize adds them in a fixed order in
// float64 (no float atomics): results are run-to-run bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrca_env.h"
#include "mrca_hostutil.h"
#include "mrca_policy_bf16_device.h"

namespace mrca_policy_bf16 {

constexpr int kBwdWavesPerSimd = 2;
constexpr int kBwdWavesPerCu = 5;                       // by LDS: 160 KB / kBwdWaveBytes
constexpr int kGTRowBytes = 64;                         // GT[l][c] = g2[c][l], l <= 128 (row 128 = 0: "l + 1" of l = 127)
constexpr int kGTOff = kWaveBytes;
constexpr int kGTRows = kL2 + 1;
constexpr int kXPOff = kGTOff + kGTRows * kGTRowBytes;  // XP[o + 1][ci][M] = x[ci][4 M + o], o = -1 .. 5, M < 128
constexpr int kXPPhases = 7;
constexpr int kBwdWaveBytes = kXPOff + kXPPhases * kFrames * 128 * 2;
static_assert(kGTOff % 16 == 0 && kXPOff % 16 == 0, "16-byte operand rows");
static_assert(kBwdWavesPerCu * kBwdWaveBytes <= 160 * 1024, "kBwdWavesPerCu waves fit the CU's LDS");

// per-wave partial record (floats)
constexpr int kPartDw2 = 0, kPartDw1 = 3072, kPartDb1 = 3072 + 480, kPartDb2 = kPartDb1 + 32, kPartFloats = kPartDb2 + 32;

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// ds_read_b64_tr_b16: per group of 16 lanes a block of 4 rows x 16 columns of 16-bit elements; lane 4 q + p of the group
// supplies the address of row q, columns 4 p .. 4 p + 3 (8-byte aligned) and lane i receives column i, row q in element q.
// EXEC must be all ones: every call below sits in wave-uniform control flow.
__device__ __forceinline__ bf16x4 lds_read_tr(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
}
// the lane's address into the position-major H for a block whose row q is H row `row0 + 2 q` and whose 16 columns are the
// channels of the lane's group: the lane receives h1 of channel (lane & 31) at the block's four positions
__device__ __forceinline__ int h_tr_off(int row0, int lane) {
    const int q = (lane >> 2) & 3, p = lane & 3, gc = (lane >> 4) & 1;
    return (row0 + 2 * q) * kHRowBytes + 2 * (16 * gc + 4 * p);
}
// a per-lane LDS base the compiler takes as it is: every access below is "base + compile-time constant", the constant an
// instruction's offset field.  (Left to itself the compiler forms each address with its own OR of lane bits and keeps one
// loop-invariant register per address: ~60 of them, past the 256 of two waves per SIMD.)
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ int xp_off(int o, int ci, int M) { return kXPOff + 2 * ((((o + 1) * kFrames) + ci) * 128 + M); }

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kBwdWavesPerSimd))) void lidar_features_bf16_bwd_kernel(
    const float* __restrict__ obs, const int32_t* __restrict__ rows, int n_robots, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const uint16_t* __restrict__ feat,
    const uint16_t* __restrict__ gfeat_act, const uint16_t* __restrict__ gfeat_crt, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // one wave per workgroup: kBwdWaveBytes
    const int lane = threadIdx.x;
    const int gwave = blockIdx.x, nwaves = gridDim.x;          // nwaves is even: a wave keeps its tower
    const int tower = gwave & 1;
    const int col = lane & 31, hl = lane >> 5;

    // --- the tower's weights as bf16 fragments: conv1's A (the forward's), and w2 as dgrad's B: wd[tap][s][j] =
    // w2[c = 16 s + 8 hl + j][ci = col][tap]
    bf16x8 wa1[2], wd[3][2];
    stage_weights(lds, w1, w2, tower, lane);
    conv1_weight_fragments(lds, col, hl, wa1);
    {
        const float* wl = reinterpret_cast<const float*>(lds);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) wd[k][s][j] = (__bf16)wl[(16 * s + 8 * hl + j) * kW2LPitch + col * 3 + k];
    }
    zero_h_paddings(lds, lane);
    // GT row 128 and the scan's paddings in XP: x[.][-1] (phase -1, M = 0), x[.][512], x[.][513] (phases 4 and 5, M = 127)
    if (lane < 32) *reinterpret_cast<__bf16*>(lds + kGTOff + kL2 * kGTRowBytes + 2 * lane) = (__bf16)0.0f;
    if (lane < 3) {
        *reinterpret_cast<__bf16*>(lds + xp_off(-1, lane, 0)) = (__bf16)0.0f;
        *reinterpret_cast<__bf16*>(lds + xp_off(4, lane, 127)) = (__bf16)0.0f;
        *reinterpret_cast<__bf16*>(lds + xp_off(5, lane, 127)) = (__bf16)0.0f;
    }

    f32x16 dw2[3], dw1;
#pragma unroll
    for (int r = 0; r < 16; ++r) dw2[0][r] = dw2[1][r] = dw2[2][r] = dw1[r] = 0.0f;
    float db2 = 0.0f;

    // conv1 wgrad's A row of this lane: (ci, k) = (rr / 5, rr % 5), rr = 15: ones (lanes 16..31 repeat rows 0..15: their
    // result rows are not read)
    const int rr = col & 15;
    const int a_ci = rr < 15 ? rr / 5 : 0, a_k = rr < 15 ? rr % 5 : 0;
    const __bf16 one = (__bf16)1.0f;

    const int gt_store = opaque(kGTOff + 8 * hl * kGTRowBytes + 2 * col);     // GT[8 hl][col]
    const int gt_load = opaque(kGTOff + col * kGTRowBytes + 16 * hl);         // GT[col][8 hl ..]
    const int xp_store = opaque(kXPOff + 2 * lane);                           // XP[-1][0][lane]
    const int xp_load = opaque(xp_off(a_k - 1, a_ci, 4 * hl));                // XP[a_k - 1][a_ci][4 hl ..]
    const int h_wgrad = opaque(h_tr_off(16 * hl, lane));                      // H rows 2 (8 hl) + 2 q
    const int h_mask = opaque(h_tr_off(8 * hl, lane));                        // H rows 2 (4 hl) + 2 q
    const uint16_t* gfeat = tower ? gfeat_crt : gfeat_act;
    const int stride = nwaves >> 1;
    int n = gwave >> 1;
    float4 sx[6];
    if (n < n_robots) request_scan_rows(sx, obs, rows, n, lane);

    for (; n < n_robots; n += stride) {              // wave-uniform; the kernel has no barrier
        // --- the scan -> X (for conv1) and -> XP (for conv1's wgrad); the next item's is requested as soon as this one is staged
        stage_scan<false>(lds, sx, lane);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = 64 * h + lane;
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                const float v[4] = {sx[2 * f + h].x, sx[2 * f + h].y, sx[2 * f + h].z, sx[2 * f + h].w};
                bf16x4 q;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    q[e] = (__bf16)v[e];
                    *reinterpret_cast<__bf16*>(lds + xp_store + (xp_off(e, f, 64 * h) - kXPOff)) = q[e];
                }
                if (m > 0) {
                    *reinterpret_cast<__bf16*>(lds + xp_store + (xp_off(4, f, 64 * h) - kXPOff - 2)) = q[0];
                    *reinterpret_cast<__bf16*>(lds + xp_store + (xp_off(5, f, 64 * h) - kXPOff - 2)) = q[1];
                }
                if (m < 127) *reinterpret_cast<__bf16*>(lds + xp_store + (xp_off(-1, f, 64 * h) - kXPOff + 2)) = q[3];
            }
        }

        if (n + stride < n_robots) request_scan_rows(sx, obs, rows, n + stride, lane);
        // (the sched_barriers keep the next phase's LDS reads from being hoisted into this one: the kernel sits at 242 of the 256
        // registers of two waves per SIMD)
        __builtin_amdgcn_sched_barrier(0);
        // --- conv1 recompute: h1 -> H (b1 is read per item: 16 registers that live through conv1 only)
        {
            float bias1[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) bias1[r] = b1[tower * 32 + rowmap(r, hl)];
            conv1_to_h(lds, wa1, bias1, col, hl);
        }

        __builtin_amdgcn_sched_barrier(0);
        // --- g2 = gfeat * (feat > 0): conv2 wgrad's A fragments; db2; GT
        // (the item's gradient and feature rows: channel col, positions 16 s + 8 hl .. + 7)
        bf16x8 ga[8];
        const u32x4* gp = reinterpret_cast<const u32x4*>(gfeat + (size_t)n * (kCh * kL2) + col * kL2 + 8 * hl);
        const u32x4* fp = reinterpret_cast<const u32x4*>(feat + ((size_t)tower * n_robots + n) * (kCh * kL2) + col * kL2 + 8 * hl);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const bf16x8 g = __builtin_bit_cast(bf16x8, gp[2 * s]);
            const bf16x8 f = __builtin_bit_cast(bf16x8, fp[2 * s]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ga[s][j] = (float)f[j] > 0.0f ? g[j] : (__bf16)0.0f;
                db2 += (float)ga[s][j];
                *reinterpret_cast<__bf16*>(lds + gt_store + (16 * s + j) * kGTRowBytes) = ga[s][j];
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);

        // --- conv2 wgrad: B element 4 u + q of k-step s, tap k = h1[ci = col][2 l + k - 1] = H row 2 l + k, l = 16 s + 8 hl + 4 u + q
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const bf16x4 lo = lds_read_tr(lds + h_wgrad + (2 * (16 * s) + k) * kHRowBytes);
                const bf16x4 hi = lds_read_tr(lds + h_wgrad + (2 * (16 * s + 4) + k) * kHRowBytes);
                const bf16x8 hb = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                dw2[k] = MRCA_MFMA_BF16(ga[s], hb, dw2[k]);
            }

        __builtin_amdgcn_sched_barrier(0);
        // --- conv2 dgrad, the ReLU mask, conv1 wgrad: 4 tiles of 32 conv2 positions l = 32 T + m, even then odd conv1 positions
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                const unsigned char* gt = lds + gt_load + 32 * T * kGTRowBytes;
                f32x16 d;
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r] = 0.0f;
                if (par == 0) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) d = MRCA_MFMA_BF16(*reinterpret_cast<const bf16x8*>(gt + 32 * s), wd[1][s], d);
                } else {
#pragma unroll
                    for (int s = 0; s < 2; ++s) d = MRCA_MFMA_BF16(*reinterpret_cast<const bf16x8*>(gt + 32 * s), wd[2][s], d);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        d = MRCA_MFMA_BF16(*reinterpret_cast<const bf16x8*>(gt + kGTRowBytes + 32 * s), wd[0][s], d);
                }
                // register 4 g + q of d: position p = 2 (32 T + 8 g + 4 hl + q) + par of channel col; h1 of it: H row p + 1
                bf16x8 gb[2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bf16x4 hv = lds_read_tr(lds + h_mask + (2 * (32 * T + 8 * g) + par + 1) * kHRowBytes);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        gb[g >> 1][4 * (g & 1) + q] = (float)hv[q] > 0.0f ? (__bf16)d[4 * g + q] : (__bf16)0.0f;
                }
                // element j of k-step s: position index m = 16 s + 8 (j >> 2) + 4 hl + (j & 3); x[ci][2 p + k - 1] = XP[2 par + k - 1][ci][32 T + m]
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const unsigned char* xa = lds + xp_load + (xp_off(2 * par, 0, 32 * T + 16 * s) - xp_off(0, 0, 0));
                    const bf16x4 x0 = *reinterpret_cast<const bf16x4*>(xa);
                    const bf16x4 x1 = *reinterpret_cast<const bf16x4*>(xa + 16);
                    bf16x8 xf = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
                    if (rr == 15) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) xf[j] = one;
                    }
                    dw1 = MRCA_MFMA_BF16(xf, gb[s], dw1);
                }
            }
        asm volatile("" ::: "memory");
    }

    // --- the wave's partial sums (zeros for a wave without items: the finalize adds every wave's record)
    float* P = partial + (size_t)gwave * kPartFloats;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) P[kPartDw2 + rowmap(r, hl) * 96 + col * 3 + k] = dw2[k][r];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = rowmap(r, hl);                 // row (ci, k) of DW1', 15: db1; rows 16 .. 31 repeat them
        if (i < 15) P[kPartDw1 + col * 15 + i] = dw1[r];
        if (i == 15) P[kPartDb1 + col] = dw1[r];
    }
    const float other = __shfl_xor(db2, 32);
    if (hl == 0) P[kPartDb2 + col] = db2 + other;
}

// out[t][k] = sum over the waves of tower t (gwave & 1 == t) in a FIXED order, as lidar_features_bwd_finalize
// (mrca_policy_bwd.hip) forms it: a block owns 64 consecutive outputs of one tower; its 16 wavefronts each add every 16th
// wave's partial, then the 16 sums are added in index order -- in float64, the partials of a weight gradient cancel heavily.
constexpr int kFinGroups = 16;
__global__ __launch_bounds__(64 * kFinGroups) void lidar_features_bf16_bwd_finalize(
    const float* __restrict__ partial, int nwaves, float* __restrict__ dw1, float* __restrict__ db1,
    float* __restrict__ dw2, float* __restrict__ db2) {
    __shared__ double part[kFinGroups][64];
    const int j = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int chunks = (kPartFloats + 63) / 64;
    const int t = blockIdx.x / chunks, k = (blockIdx.x % chunks) * 64 + j;
    double s = 0.0;
    if (k < kPartFloats)
        for (int w = t + 2 * grp; w < nwaves; w += 2 * kFinGroups) s += (double)partial[(size_t)w * kPartFloats + k];
    part[grp][j] = s;
    __syncthreads();
    if (grp != 0 || k >= kPartFloats) return;
    double acc = 0.0;
#pragma unroll
    for (int gidx = 0; gidx < kFinGroups; ++gidx) acc += part[gidx][j];
    const float tot = (float)acc;
    if (k < kPartDw1) dw2[t * 3072 + k] = tot;
    else if (k < kPartDb1) dw1[t * 480 + (k - kPartDw1)] = tot;
    else if (k < kPartDb2) db1[t * 32 + (k - kPartDb1)] = tot;
    else db2[t * 32 + (k - kPartDb2)] = tot;
}

static DeviceInfo g_bwd_dev[64];

static inline int bwd_max_waves(int cus) { return (cus * kBwdWavesPerCu) & ~1; }

}  // namespace mrca_policy_bf16

extern "C" int mrca_lidar_features_bf16_backward_scratch(size_t* bytes_out) {
    using namespace mrca_policy_bf16;
    if (!bytes_out) return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_backward_scratch: bytes_out is NULL");
    const int cus = device_cus(g_bwd_dev);
    if (cus < 0) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16_backward_scratch: hipGetDevice failed");
    *bytes_out = (size_t)bwd_max_waves(cus) * kPartFloats * sizeof(float);
    return MRCA_OK;
}

static int lidar_features_bf16_backward_impl(const char* who, const float* obs_dev, const int32_t* rows_dev, int32_t n_robots,
                                             int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev,
                                             const float* w2_dev, const uint16_t* feat_dev, const uint16_t* gfeat_act_dev,
                                             const uint16_t* gfeat_crt_dev, float* dw1_dev, float* db1_dev, float* dw2_dev,
                                             float* db2_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    using namespace mrca_policy_bf16;
    if (!obs_dev || !w1_dev || !b1_dev || !w2_dev || !feat_dev || !gfeat_act_dev || !gfeat_crt_dev || !dw1_dev || !db1_dev || !dw2_dev ||
        !db2_dev || !scratch_dev)
        return mrca::set_error(MRCA_ERR_INVALID, "%s: NULL pointer", who);
    if (frames != kFrames || beams != kBeams || n_robots < 1)
        return mrca::set_error(MRCA_ERR_UNSUPPORTED, "%s: frames %d beams %d samples %d (needs 3 x 512, >= 1)", who, frames, beams, n_robots);
    // 16-byte loads of the scans, weights, features and their gradients; 4-byte accesses of the rest
    if ((reinterpret_cast<uintptr_t>(obs_dev) | reinterpret_cast<uintptr_t>(w1_dev) | reinterpret_cast<uintptr_t>(w2_dev) |
         reinterpret_cast<uintptr_t>(feat_dev) | reinterpret_cast<uintptr_t>(gfeat_act_dev) | reinterpret_cast<uintptr_t>(gfeat_crt_dev)) & 15)
        return mrca::set_error(MRCA_ERR_INVALID, "%s: obs, w1, w2, feat and the two gfeat must be 16-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(rows_dev) | reinterpret_cast<uintptr_t>(b1_dev) | reinterpret_cast<uintptr_t>(dw1_dev) |
         reinterpret_cast<uintptr_t>(db1_dev) | reinterpret_cast<uintptr_t>(dw2_dev) | reinterpret_cast<uintptr_t>(db2_dev) |
         reinterpret_cast<uintptr_t>(scratch_dev)) & 3)
        return mrca::set_error(MRCA_ERR_INVALID, "%s: rows, b1, the gradients and the scratch must be 4-byte aligned", who);
    mrca::DeviceGuard guard(mrca::device_of(obs_dev));     // launch where the buffers live
    const int cus = device_cus(g_bwd_dev);
    if (cus < 0) return mrca::set_error(MRCA_ERR_HIP, "%s: hipGetDevice failed", who);
    int nwaves = bwd_max_waves(cus);         // persistent one-wave workgroups, (actor, critic) pairs, no more than there is work for
    if (nwaves > 2 * n_robots) nwaves = 2 * n_robots;
    if (scratch_bytes < (size_t)nwaves * kPartFloats * sizeof(float))
        return mrca::set_error(MRCA_ERR_INVALID, "%s: scratch of %zu B < %zu B", who, scratch_bytes, (size_t)nwaves * kPartFloats * sizeof(float));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(lidar_features_bf16_bwd_kernel, dim3(nwaves), dim3(64), (size_t)kBwdWaveBytes, st, obs_dev, rows_dev, n_robots,
                       w1_dev, b1_dev, w2_dev, feat_dev, gfeat_act_dev, gfeat_crt_dev, static_cast<float*>(scratch_dev));
    hipLaunchKernelGGL(lidar_features_bf16_bwd_finalize, dim3(2 * ((kPartFloats + 63) / 64)), dim3(64 * kFinGroups), 0, st,
                       static_cast<const float*>(scratch_dev), nwaves, dw1_dev, db1_dev, dw2_dev, db2_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mrca::set_error(MRCA_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return MRCA_OK;
}

extern "C" int mrca_lidar_features_bf16_backward(const float* obs_dev, int32_t n_robots, int32_t frames, int32_t beams,
                                                 const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                                 const uint16_t* feat_dev, const uint16_t* gfeat_act_dev,
                                                 const uint16_t* gfeat_crt_dev, float* dw1_dev, float* db1_dev, float* dw2_dev,
                                                 float* db2_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    return lidar_features_bf16_backward_impl("mrca_lidar_features_bf16_backward", obs_dev, nullptr, n_robots, frames, beams, w1_dev,
                                             b1_dev, w2_dev, feat_dev, gfeat_act_dev, gfeat_crt_dev, dw1_dev, db1_dev, dw2_dev, db2_dev,
                                             scratch_dev, scratch_bytes, stream);
}

extern "C" int mrca_lidar_features_bf16_backward_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples,
                                                      int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev,
                                                      const float* w2_dev, const uint16_t* feat_dev, const uint16_t* gfeat_act_dev,
                                                      const uint16_t* gfeat_crt_dev, float* dw1_dev, float* db1_dev, float* dw2_dev,
                                                      float* db2_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    if (!rows_dev) return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_backward_rows: rows_dev is NULL");
    return lidar_features_bf16_backward_impl("mrca_lidar_features_bf16_backward_rows", frames_dev, rows_dev, n_samples, frames, beams,
                                             w1_dev, b1_dev, w2_dev, feat_dev, gfeat_act_dev, gfeat_crt_dev, dw1_dev, db1_dev, dw2_dev,
                                             db2_dev, scratch_dev, scratch_bytes, stream);
}
