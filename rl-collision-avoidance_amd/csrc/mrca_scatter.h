// mrca_scatter.h -- launch interface of the scenario sampler (mrca_scatter.hip) for the C ABI (mrca_abi_controllers.hip: mrca_scatter).
#pragma once
#include "mrca_kernels.h"
#include "mrca_scatter_device.h"

namespace mrca {

// The rule of mrca_scatter_device.h for every world of e: boxes f32[R,8] -> poses f32[N,3], goals f32[N,2], tries i32[N,2]
// (nullptr: not wanted).  ONE launch on `s`, a workgroup per world (64 lanes for R <= 64, 256 above) with R * 8 bytes of LDS:
// R <= kScatterMaxRobots, which the ABI has checked like the params.  Reads e's geometry, cellfield and key; writes the three
// buffers and nothing of the env.
void launch_scatter(const EnvView& e, const ScatterParams& p, const float* boxes, float* poses, float* goals, int32_t* tries,
                    hipStream_t s);

}  // namespace mrca
