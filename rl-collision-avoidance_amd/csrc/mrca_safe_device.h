// mrca_safe_device.h -- hybrid control in the PAPER'S form (mrca_hybrid_plan, mrca_hybrid_commit), the rule
// stated once for the gfx950 kernels of mrca_safe.hip and for a plain host build (tests/test_safe_host.py drives the same
// functions through g++).  It stands on the functions of mrca_hybrid_device.h as they are: the same beams, the same minima, the
// same classification.
//
// Fan, Long, Liu, Pan (IJRR 2020, Sec. 5): where an obstacle is dangerously close the SAFE POLICY drives -- the network run on
// a scan in which obstacles look nearer, its speed capped.  The mode of mrca_hybrid_device.h does not depend on the incoming
// command (it is decided from the newest scan row and the local goal), so it is known BEFORE the forward runs, and a tick is
//
//   PLAN    mode[n] as mrca_hybrid_actions would report it;  scale[n] = scan_scale in mode 2, else 1;
//           pid[n] = the PID command in mode 1, (0, 0) in the other modes
//   FORWARD one forward for everybody, robot n's ranges multiplied by scale[n] while they are staged
//           (mrca_lidar_features_scaled / _bf16_scaled:  x' = x < 6 ? x scale : x  in front of x / 6 - 0.5)
//   COMMIT  mode 0: the policy's (vp, wp) bit for bit;  modes 1 and -2: pid;  mode 2: (vp > v_cap ? v_cap : vp, wp);
//           any other mode value: (vp, wp) bit for bit
//
// OUR READING OF THE PAPER'S "SCALED SCAN".  A beam that returned nothing (exactly 6, the lidar's range) stays "nothing": only
// returns come nearer, a return at r is seen at r s.  And the WHOLE stack of three frames is scaled by the CURRENT tick's factor,
// so that the frames stay mutually consistent: a robot that enters the safe mode does not see everything jump towards it
// between two frames.
//
// Mode 2's clearance scaling s(d_front) of mrca_hybrid_actions is deliberately NOT applied in the commit: the scaled scan is the
// paper's mechanism, and stacking ours on top of it would measure neither.  omega is kept, so the robot may still turn away at
// full rate; a NaN vp stays a NaN (the comparison is false).
//
// Every step is a comparison, a copy or one separately rounded fp32 multiply: tests/safe_ref.py restates it in NumPy float32
// and gives the same bits.
#pragma once
#include "mrca_hybrid_device.h"

namespace mrca {

// same layout as mrca_safe_policy_params (include/mrca_env.h)
struct SafeParams {
    float scan_scale, v_cap;
};

// the range the safe policy sees in place of x = |raw range| under the factor s (restated by the two front ends, which do not
// see the env's headers: mrca_policy.hip, mrca_policy_bf16_device.h: scale_range)
MRCA_HD float safe_scan_range(float x, float s) { return x < kHybridRangeMax ? x * s : x; }

// PLAN: what the beams added up to -> mode, the scan factor and the PID command.  The classification is hybrid_result's, asked
// with a zero command (no mode depends on the command; mode 1 and -2 do not read it).
MRCA_HD void safe_plan_result(const HybridParams& q, const SafeParams& sp, const HybridRobot& rb, const HybridAcc& acc, int* mode,
                              float* scale, float* pid_v, float* pid_w) {
    float v, w;
    int m;
    hybrid_result(q, rb, acc, 0.0f, 0.0f, &v, &w, &m);
    *mode = m;
    *scale = m == kHybridEmergent ? sp.scan_scale : 1.0f;
    *pid_v = m == kHybridSimple ? v : 0.0f;
    *pid_w = m == kHybridSimple ? w : 0.0f;
}

// COMMIT: the command that drives the robot from the forward's (vp, wp), the plan's mode and PID command
MRCA_HD void safe_commit(const SafeParams& sp, int mode, float vp, float wp, float pid_v, float pid_w, float* v, float* w) {
    if (mode == kHybridSimple || mode == kHybridAtGoal) {
        *v = pid_v;
        *w = pid_w;
    } else if (mode == kHybridEmergent) {
        *v = vp > sp.v_cap ? sp.v_cap : vp;
        *w = wp;
    } else {
        *v = vp;
        *w = wp;
    }
}

// ---- the plan as a plain loop.  The kernel runs the same pieces with a beam per lane and one wave reduction.
// goal = the robot's MRCA_F_LOCAL_GOAL, ranges = its newest scan row -> mode, scale, pid (v, omega), clear = (d_min, d_front, d_block)
MRCA_HD void safe_plan_robot(const HybridParams& q, const SafeParams& sp, const float* goal, const float* ranges, int beams,
                             const float* beam_cos, const float* beam_sin, int* mode, float* scale, float* pid, float* clear) {
    const HybridRobot rb = hybrid_robot_begin(q, goal[0], goal[1]);
    HybridAcc acc = hybrid_acc_empty();
    for (int b = 0; b < beams; ++b) hybrid_beam(q, rb, ranges[b], beam_cos[b], beam_sin[b], &acc);
    safe_plan_result(q, sp, rb, acc, mode, scale, &pid[0], &pid[1]);
    clear[0] = acc.d_min;
    clear[1] = acc.d_front;
    clear[2] = acc.d_block;
}

}  // namespace mrca
