// mrca_noise.h -- launch interface of the lidar noise model (mrca_noise.hip) for the C ABI (mrca_abi_controllers.hip: mrca_scan_noise).
#pragma once
#include "mrca_kernels.h"
#include "mrca_noise_device.h"

namespace mrca {

// The rule of mrca_noise_device.h applied IN PLACE to the newest scan row of every robot whose mask byte is not 0 (mask nullptr:
// all): the row in slot ring_head[n] of scan_ring and its hit words -- for a robot whose fresh flag is set, all F slots (the
// cast has just filled them with one row).  views: bits of MRCA_VIEW_*, the eager views (lazy_obs = 0) rewritten with it:
// scan[n], and the newest frame of obs[n] (all F frames for a fresh robot).  ONE launch on `s`, the params travel as kernel
// arguments.  Reads e's ring_head, fresh, t, episode and key; writes the ring, the hit bits and those views, nothing else.
// Arguments are the ABI's, already validated.
void launch_scan_noise(const EnvView& e, const ScanNoiseParams& p, const uint8_t* mask, int views, hipStream_t s);

}  // namespace mrca
