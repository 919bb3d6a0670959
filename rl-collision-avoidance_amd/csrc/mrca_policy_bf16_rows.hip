// mrca_policy_bf16_rows.hip -- the bf16 lidar front end reading its scans through a row table: the forward of the opt-in
// fused bf16 PPO update (mrca_lidar_features_bf16_rows, include/mrca_env.h).  The minibatch's stacks are read in place out of
// the rollout buffer's one-frame-per-tick store (frames f32[*][512], normalised; rows i32[n][3], oldest first), as
// mrca_lidar_features_rows does for the fp32 update.  The wave's work is front_end_wave of mrca_policy_bf16_device.h -- the
// code of the rollout's kernel (mrca_policy_bf16.hip), so the update re-evaluates the policy with the rollout's rounding
// points and instructions; only the three row indices of a sample come from the table.  HBM per sample: 6 KB in, 16 KB out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrca_env.h"
#include "mrca_hostutil.h"
#include "mrca_policy_bf16_device.h"

namespace mrca_policy_bf16 {

constexpr int kRowsWavesPerSimd = 2;    // as the rollout's kernel: 9 waves per CU by LDS, <= 256 registers per lane

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kRowsWavesPerSimd))) void lidar_features_bf16_rows_kernel(
    const float* __restrict__ frames, const int32_t* __restrict__ rows, int n_samples, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, uint16_t* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // one wave per workgroup: kWaveBytes
    front_end_wave<false, true>(lds, frames, nullptr, rows, n_samples, w1, b1, w2, b2, feat, blockIdx.x, gridDim.x);
}

static DeviceInfo g_rows_dev[64];

}  // namespace mrca_policy_bf16

extern "C" int mrca_lidar_features_bf16_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples, int32_t frames,
                                             int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                             const float* b2_dev, uint16_t* feat_dev, void* stream) {
    using namespace mrca_policy_bf16;
    if (!frames_dev || !rows_dev || !w1_dev || !b1_dev || !w2_dev || !b2_dev || !feat_dev)
        return mrca::set_error(MRCA_ERR_INVALID, "mrca_lidar_features_bf16_rows: NULL pointer");
    if (frames != kFrames || beams != kBeams || n_samples < 1)
        return mrca::set_error(MRCA_ERR_UNSUPPORTED,
                               "mrca_lidar_features_bf16_rows: frames %d beams %d samples %d (needs 3 x 512, >= 1)", frames, beams,
                               n_samples);
    // 16-byte loads of the frames and weights, 16-byte stores of the features, 4-byte loads of the table
    if (((reinterpret_cast<uintptr_t>(frames_dev) | reinterpret_cast<uintptr_t>(w1_dev) | reinterpret_cast<uintptr_t>(w2_dev) |
          reinterpret_cast<uintptr_t>(feat_dev)) & 15) || (reinterpret_cast<uintptr_t>(rows_dev) & 3))
        return mrca::set_error(MRCA_ERR_INVALID,
                               "mrca_lidar_features_bf16_rows: frames, w1, w2 and feat must be 16-byte aligned, rows 4-byte");
    mrca::DeviceGuard guard(mrca::device_of(frames_dev));
    const int cus = device_cus(g_rows_dev);
    if (cus < 0) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16_rows: hipGetDevice failed");
    int pairs = cus * 4 * kRowsWavesPerSimd / 2;
    if (pairs > n_samples) pairs = n_samples;
    hipLaunchKernelGGL(lidar_features_bf16_rows_kernel, dim3(2 * pairs), dim3(64), (size_t)kWaveBytes, static_cast<hipStream_t>(stream),
                       frames_dev, rows_dev, n_samples, w1_dev, b1_dev, w2_dev, b2_dev, feat_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mrca::set_error(MRCA_ERR_HIP, "mrca_lidar_features_bf16_rows launch: %s", hipGetErrorString(e));
    return MRCA_OK;
}
