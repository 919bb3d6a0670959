// mrca_orca.h -- launch interface of the ORCA baseline controller (mrca_orca.hip) for the C ABI (mrca_abi.hip: mrca_orca_actions).
#pragma once
#include "mrca_kernels.h"
#include "mrca_orca_device.h"

namespace mrca {

// actions[n] := the (v, omega) the rule of mrca_orca_device.h gives robot n, vel[n] (or nullptr) := the holonomic velocity it
// chose, for every robot whose mask byte is not 0 (mask nullptr: all); other rows are not touched.  ONE launch on `s`, the
// params travel as kernel arguments.  Reads e's fields as they stand on `s`, writes none.  Worlds of 1..kOrcaMaxRobots (64)
// robots: a world's robots are the lanes of a wavefront.  Arguments are the ABI's, already validated.
void launch_orca(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s);

}  // namespace mrca
