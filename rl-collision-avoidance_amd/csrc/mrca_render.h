// mrca_render.h -- launch interface of the top-down renderer (mrca_render.hip) for the C ABI (mrca_abi_controllers.hip: mrca_render).
#pragma once
#include "mrca_kernels.h"
#include "mrca_render_device.h"

namespace mrca {

// The views travel to the kernels as kernel arguments (2 kB for 128 of them): nothing is copied to the device ahead of the
// launches, so the call neither synchronises nor keeps a staging buffer whose reuse two streams could race on.  A call with
// more views goes out as one set of launches per 128.
constexpr int kRenderViewsPerLaunch = 128;

// ids[V,H,W] := the ID image of every view (cleared first); trail[V,H,W] (or nullptr) takes max(trail, index + 1) at every
// robot's centre; rgb[V,H,W,3] (or nullptr) := the resolved picture.  Reads e's fields as they stand on `s`, writes none.
// Arguments are the ABI's, already validated (rgb 4-byte aligned).
void launch_render(const EnvView& e, const RenderView* views, int num_views, int W, int H, uint32_t layers, uint32_t* ids,
                   uint32_t* trail, uint8_t* rgb, hipStream_t s);

}  // namespace mrca
