// mrca_orca.h -- launch interface of the ORCA baseline controller (mrca_orca.hip) for the C ABI (mrca_abi_controllers.hip: mrca_orca_actions).
#pragma once
#include "mrca_kernels.h"
#include "mrca_nhorca_device.h"

namespace mrca {

// actions[n] := the (v, omega) the rule of mrca_orca_device.h gives robot n, vel[n] (or nullptr) := the holonomic velocity it
// chose, for every robot whose mask byte is not 0 (mask nullptr: all); other rows are not touched.  ONE launch on `s`, the
// params travel as kernel arguments.  Reads e's fields as they stand on `s`, writes none.  Worlds of 1..kOrcaMaxRobots (64)
// robots: a world's robots are the lanes of a wavefront.  Arguments are the ABI's, already validated.
void launch_orca(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s);

// The same for worlds of MORE than kOrcaMaxRobots robots (mrca_orca_actions_any): a robot's candidates come from the env's
// lidar hash (e.bw_lstart / bw_lsorted), which must describe the poses as they stand on `s`, and orca_rings(p.neighbor_dist)
// must not be 0.  ONE launch, one wavefront per robot; reads e (the hash included), writes none of it.
void launch_orca_big(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s);

// The NH-ORCA baseline (mrca_nhorca_actions, the rule of mrca_nhorca_device.h): actions and vel as above (vel: the tracked solve's
// velocity), mode[n] (or nullptr) := enum NhOrcaMode.  `big`: launch_orca_big's way to the neighbours and its conditions; otherwise
// launch_orca's.  ONE launch; p.o.max_neighbors <= kNhMaxNeighbors.
void launch_nhorca(const EnvView& e, const NhOrcaParams& p, bool big, const uint8_t* mask, float* actions, float* vel, int32_t* mode,
                   hipStream_t s);

}  // namespace mrca
