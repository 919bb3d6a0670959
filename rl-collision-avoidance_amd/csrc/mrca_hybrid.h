// mrca_hybrid.h -- launch interface of the hybrid control wrapper (mrca_hybrid.hip) for the C ABI (mrca_abi_controllers.hip: mrca_hybrid_actions).
#pragma once
#include "mrca_kernels.h"
#include "mrca_hybrid_device.h"

namespace mrca {

// actions[n] := the (v, omega) the rule of mrca_hybrid_device.h makes of policy[n] for robot n, mode[n] (or nullptr) := which
// of the three drives it (kHybridNormal / Simple / Emergent, kHybridAtGoal), clear[n] (or nullptr) := (d_min, d_front, d_block),
// for every robot whose mask byte is not 0 (mask nullptr: all); other rows are not touched.  actions may be policy itself.
// ONE launch on `s`, the params travel as kernel arguments and the env's fields through its device-side view (e.dev).  Reads
// e's local_goal, scan_ring, ring_head and beam tables as they stand on `s`, writes nothing of e.  Worlds of any size: a robot
// needs nothing of another.  Arguments are the ABI's, already validated.
// goal: f32[N,2] rows in the robots' frames that stand where e's local_goal would (mrca_hybrid_actions_goal), nullptr = e's local_goal.
void launch_hybrid(const EnvView& e, const HybridParams& p, const float* goal, const uint8_t* mask, const float* policy, float* actions, int32_t* mode,
                   float* clear, hipStream_t s);

}  // namespace mrca
