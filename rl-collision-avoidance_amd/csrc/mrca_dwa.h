// mrca_dwa.h -- launch interface of the DWA baseline controller (mrca_dwa.hip) for the C ABI (mrca_abi_controllers.hip: mrca_dwa_actions).
#pragma once
#include "mrca_kernels.h"
#include "mrca_dwa_device.h"

namespace mrca {

// actions[n] := the (v, omega) the rule of mrca_dwa_device.h gives robot n, choice[n] (or nullptr) := the candidate it chose
// (kDwaChoiceBlocked / kDwaChoiceAtGoal: none), score[n] (or nullptr) := that candidate's score, for every robot whose mask
// byte is not 0 (mask nullptr: all); other rows are not touched.  ONE launch on `s`, the params travel as kernel arguments.
// Reads e's local_goal, speed, scan_ring, ring_head and beam tables as they stand on `s`, writes nothing of e.  Worlds of any
// size: a robot needs nothing of another.  Arguments are the ABI's, already validated.
// goal: f32[N,2] rows in the robots' frames that stand where e's local_goal would (mrca_dwa_actions_goal), nullptr = e's local_goal.
void launch_dwa(const EnvView& e, const DwaParams& p, const float* goal, const uint8_t* mask, float* actions, int32_t* choice, float* score,
                hipStream_t s);

}  // namespace mrca
