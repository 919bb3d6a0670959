// mrca_planner.h -- launch interface of the global planner (mrca_planner.hip) for the C ABI (mrca_abi_controllers.hip: mrca_goal_fields,
// mrca_subgoals, mrca_subgoals_los).
#pragma once
#include "mrca_kernels.h"
#include "mrca_planner_device.h"

namespace mrca {

// field[g][j][i] := plan_field_init of planning cell (i, j) for goal point goals[g]: 0 at its seed, kPlanWall where blocked,
// kPlanInf elsewhere.  Reads e's cellfield and geometry.
void launch_goal_field_init(const EnvView& e, const PlannerParams& p, const float* goals, int G, uint32_t* field, hipStream_t s);
// One round: every (goal, tile) relaxes its tile from the field as it stands and stores the cells that fell; *counter += 1 per
// workgroup in which anything fell or whose sweeps ran out.  No workgroup waits for another.
void launch_goal_field_round(const EnvView& e, const PlannerParams& p, int G, uint32_t* field, uint32_t* counter, hipStream_t s);
// kPlanWall -> kPlanInf: the field as the ABI describes it
void launch_goal_field_finish(const EnvView& e, const PlannerParams& p, int G, uint32_t* field, hipStream_t s);

// The per-tick call: ONE launch on `s`, the params travel as kernel arguments and the env's fields through its device-side view
// (e.dev).  Reads e's pose, head records, goal and geometry and the caller's field / goals / slot as they stand on `s`, writes
// nothing of e.  lanes: 8 (a direction per lane, the product) or 1 (a robot per thread: plan_robot as it stands).  Arguments are
// the ABI's, already validated.
void launch_subgoals(const EnvView& e, const PlannerParams& p, const uint32_t* field, const float* goals, int G, const int32_t* slot,
                     const uint8_t* mask, float* local, float* subgoal, float* dist, int32_t* status, int lanes, hipStream_t s);

// The per-tick call with line of sight (the rule: mrca_planner_device.h, LINE OF SIGHT): launch_subgoals' arguments, the reach
// and ahead (i32[N,2] = (m, m_vis), or nullptr).  ONE launch.  lanes: a robot's group, 8 or 64 (the same outputs).
constexpr int kLosWaveRobots = 8192;      // up to here the library gives a robot a wavefront (mrca_abi_controllers.hip)
void launch_subgoals_los(const EnvView& e, const PlannerParams& p, const LosParams& lp, const uint32_t* field, const float* goals, int G,
                         const int32_t* slot, const uint8_t* mask, float* local, float* subgoal, float* dist, int32_t* status,
                         int32_t* ahead, int lanes, hipStream_t s);

}  // namespace mrca
