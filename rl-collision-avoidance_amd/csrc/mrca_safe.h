// mrca_safe.h -- launch interface of hybrid control in the paper's form (mrca_safe.hip) for the C ABI (mrca_abi_controllers.hip:
// mrca_hybrid_plan, mrca_hybrid_commit).
#pragma once
#include "mrca_kernels.h"
#include "mrca_safe_device.h"

namespace mrca {

// mode[n], scale[n], pid[n] and clear[n] (or nullptr) := what safe_plan_robot (mrca_safe_device.h) makes of robot n's newest scan
// row and local goal, for every robot whose mask byte is not 0 (mask nullptr: all); other rows are not touched.  ONE launch on
// `s`; reads e's local_goal, scan_ring, ring_head and beam tables as they stand on `s`, writes nothing of e.  Arguments are the
// ABI's, already validated.  goal: f32[N,2] rows that stand where e's local_goal would (mrca_hybrid_plan_goal), nullptr = e's local_goal.
void launch_hybrid_plan(const EnvView& e, const HybridParams& p, const SafeParams& sp, const float* goal, const uint8_t* mask, int32_t* mode, float* scale,
                        float* pid, float* clear, hipStream_t s);

// actions[n] := safe_commit of policy[n] under mode[n] and pid[n], for every robot whose mask byte is not 0; actions may be
// policy itself.  ONE launch on `s`, one thread per robot; needs no env.
void launch_hybrid_commit(int32_t n_robots, const SafeParams& sp, const uint8_t* mask, const int32_t* mode, const float* pid,
                          const float* policy, float* actions, hipStream_t s);

}  // namespace mrca
