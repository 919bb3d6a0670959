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
#include "mrca_policy_bf16_device.h"

namespace mrca_policy_bf16 {

constexpr int kWavesPerSimd = 2;        // resident by LDS (9 waves per CU fit) and by registers (<= 256 per lane)

// the wave's work is front_end_wave (mrca_policy_bf16_device.h), shared with the row-table form of the update
template <bool RAW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) void lidar_features_bf16_kernel(
    const float* __restrict__ obs, const uint8_t* __restrict__ head, int n_robots, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, uint16_t* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // one wave per workgroup: kWaveBytes
    front_end_wave<RAW, false>(lds, obs, head, nullptr, n_robots, w1, b1, w2, b2, feat, blockIdx.x, gridDim.x);
}

// the safe policy's form (mrca_lidar_features_bf16_scaled): raw ring, robot n's ranges times scale[n] before rounding point 1
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) void lidar_features_bf16_scaled_kernel(
    const float* __restrict__ obs, const uint8_t* __restrict__ head, const float* __restrict__ scale, int n_robots,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    uint16_t* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    front_end_wave<true, false, true>(lds, obs, head, nullptr, n_robots, w1, b1, w2, b2, feat, blockIdx.x, gridDim.x, scale);
}

static DeviceInfo g_dev[64];

}  // namespace mrca_policy_bf16

// scale_dev != NULL: the scaled kernel (raw ring form; mrca_lidar_features_bf16_scaled has checked that)
static int lidar_features_bf16_impl(const float* obs_dev, const uint8_t* obs_head_dev, const float* scale_dev, int32_t raw_scans,
                                    int32_t n_robots, int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev,
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
    const int cus = device_cus(g_dev);
    if (cus < 0) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16: hipGetDevice failed");
    // persistent one-wave workgroups, (actor, critic) pairs: 4 SIMDs x kWavesPerSimd per CU, no more than there is work for
    int pairs = cus * 4 * kWavesPerSimd / 2;
    if (pairs > n_robots) pairs = n_robots;
    const size_t lds = kWaveBytes;
    if (scale_dev)
        hipLaunchKernelGGL(lidar_features_bf16_scaled_kernel, dim3(2 * pairs), dim3(64), lds, static_cast<hipStream_t>(stream),
                           obs_dev, obs_head_dev, scale_dev, n_robots, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    else if (raw_scans)
        hipLaunchKernelGGL(lidar_features_bf16_kernel<true>, dim3(2 * pairs), dim3(64), lds, static_cast<hipStream_t>(stream),
                           obs_dev, obs_head_dev, n_robots, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    else
        hipLaunchKernelGGL(lidar_features_bf16_kernel<false>, dim3(2 * pairs), dim3(64), lds, static_cast<hipStream_t>(stream),
                           obs_dev, obs_head_dev, n_robots, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16 launch: %s", hipGetErrorString(e));
    return MRCA_OK;
}

extern "C" int mrca_lidar_features_bf16(const float* obs_dev, const uint8_t* obs_head_dev, int32_t raw_scans, int32_t n_robots,
                                        int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev,
                                        const float* w2_dev, const float* b2_dev, uint16_t* feat_dev, void* stream) {
    return lidar_features_bf16_impl(obs_dev, obs_head_dev, nullptr, raw_scans, n_robots, frames, beams, w1_dev, b1_dev, w2_dev, b2_dev,
                                    feat_dev, stream);
}

extern "C" int mrca_lidar_features_bf16_scaled(const float* obs_dev, const uint8_t* obs_head_dev, const float* scale_dev,
                                               int32_t n_robots, int32_t frames, int32_t beams, const float* w1_dev,
                                               const float* b1_dev, const float* w2_dev, const float* b2_dev, uint16_t* feat_dev,
                                               void* stream) {
    if (!obs_head_dev)
        return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_scaled: obs_head_dev is NULL (raw ring form only)");
    if (!scale_dev) return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_scaled: scale_dev is NULL");
    if (reinterpret_cast<uintptr_t>(scale_dev) % 4)
        return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_scaled: scale_dev must be 4-byte aligned");
    return lidar_features_bf16_impl(obs_dev, obs_head_dev, scale_dev, 1, n_robots, frames, beams, w1_dev, b1_dev, w2_dev, b2_dev,
                                    feat_dev, stream);
}
