// mrca_hybrid_device.h -- the rule of the hybrid control wrapper (mrca_hybrid_actions), stated once for the
// gfx950 kernel of mrca_hybrid.hip and for a plain host build (tests/test_hybrid_host.py drives the same functions through g++).
//
// The idea is the hybrid control of Fan, Long, Liu, Pan, "Distributed multi-robot collision avoidance via deep reinforcement
// learning for navigation in complex scenarios" (IJRR 2020, Sec. 5): a learned policy drives only where it is needed.  Where
// nothing stands between a robot and its goal a PID law drives it there ("simple"), where an obstacle is dangerously close the
// policy is made careful ("emergent"), and everywhere else the policy's command goes through ("normal").
//
// WHERE THIS DIFFERS FROM THE PAPER.  The paper's safe policy runs the NETWORK AGAIN on a scan scaled down so that obstacles
// look nearer, and clips its output.  This rule sits BEHIND the policy and scales the command it has already given: v is
// multiplied by s in [0, safe_scale], omega is kept, so the robot can still turn away at full rate.  The mode goes out with the
// command; the literal form -- the network on the rescaled scan, in the same forward -- is mrca_safe_device.h's.  And the paper's
// "the goal is nearer than every obstacle" is here a CORRIDOR test: no return stands within `corridor` metres of the straight
// segment from the robot towards its goal, `look` metres long at most.
//
// It is SENSOR-LEVEL: per robot it reads the newest row of the scan ring, the goal in the robot's frame (MRCA_F_LOCAL_GOAL) and
// the incoming command.  It does NOT read MRCA_F_HIT_BITS, poses or anything of another robot; behind mrca_scan_noise it sees
// the noisy row.  Everything happens in the robot's own frame (x ahead, y to the left), where the beam directions
// (beam_cos / beam_sin) already are.  With goal (gx, gy), command (vp, wp), ranges r_b (r = r_b + 0: a -0.0 counts as 0):
//
//   gl = sqrt(gx gx + gy gy);   gl <= kGoalRadius: the command is (0, 0), mode -2 (as the DWA baseline)
//   u = g / gl,   reach = min(gl, look)
//   a beam is a RETURN iff r < 6;  its point p = r (c_b, s_b),  t = p . u,  l = p x u = px uy - py ux;
//   it BLOCKS iff t >= 0 && t <= reach && |l| < corridor                        (at the goal no beam blocks)
//   d_min = least r of all beams,  d_front = least r of the beams with c_b >= front_cos (6: none),
//   n_block = blocking beams,  d_block = least r among them (6: none)
//   mode 2, emergent, iff d_min < risk_dist:   (vp s, wp),  s = clamp((d_front - stop_dist) / (risk_dist - stop_dist), 0, safe_scale)
//   mode 1, simple, iff not emergent and n_block == 0:   orca_command(v_pid u, heading (s, c) = (0, 1), max_speed, k_omega)
//   mode 0, normal, otherwise:   (vp, wp) bit for bit, a NaN or a -0.0 included
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 + - * / sqrt or a comparison, in a fixed order
// (-ffp-contract=off, correctly rounded division and square root); no transcendental, no atan2.  A NumPy float32 restatement
// (tests/hybrid_ref.py) gives the same bits.
//
// What is written so that the ORDER of evaluation cannot show: the three clearances are minima written `d < m ? d : m` over
// values none of which is a -0.0, and n_block is a count -- the kernel deals the beams to the lanes of a wavefront and reduces,
// the host functions below walk them in a loop.
#pragma once
#include "mrca_orca_device.h"

namespace mrca {

// same layout as mrca_hybrid_params (include/mrca_env.h)
struct HybridParams {
    float risk_dist, stop_dist, safe_scale, corridor, look, front_cos, v_pid, k_omega, max_speed;
};

constexpr float kHybridRangeMax = 6.0f;   // the lidar's range: a beam that returns this saw nothing
constexpr int kHybridNormal = 0;          // the incoming command as it is
constexpr int kHybridSimple = 1;          // the way to the goal is free: the PID law
constexpr int kHybridEmergent = 2;        // something is dangerously close: the incoming command's v scaled down
constexpr int kHybridAtGoal = -2;         // within kGoalRadius of the goal: (0, 0)

// what is the same for every beam of a robot
struct HybridRobot {
    float ux, uy, reach;
    bool at_goal;
};
MRCA_HD HybridRobot hybrid_robot_begin(const HybridParams& q, float gx, float gy) {
    HybridRobot r;
    const float gl = sqrtf(gx * gx + gy * gy);
    r.at_goal = gl <= kGoalRadius;
    r.ux = 0.0f;
    r.uy = 0.0f;
    r.reach = 0.0f;
    if (!r.at_goal) {
        r.ux = gx / gl;
        r.uy = gy / gl;
        r.reach = gl < q.look ? gl : q.look;
    }
    return r;
}

// what a robot's beams add up to; any two of these merge into one, in any order
struct HybridAcc {
    float d_min, d_front, d_block;
    int n_block;
};
MRCA_HD HybridAcc hybrid_acc_empty() { return HybridAcc{kInf, kHybridRangeMax, kHybridRangeMax, 0}; }
MRCA_HD float hybrid_min(float d, float m) { return d < m ? d : m; }
MRCA_HD HybridAcc hybrid_acc_merge(const HybridAcc& a, const HybridAcc& b) {
    return HybridAcc{hybrid_min(a.d_min, b.d_min), hybrid_min(a.d_front, b.d_front), hybrid_min(a.d_block, b.d_block), a.n_block + b.n_block};
}

// one beam of range `range` in direction (bc, bs), folded into acc
MRCA_HD void hybrid_beam(const HybridParams& q, const HybridRobot& rb, float range, float bc, float bs, HybridAcc* acc) {
    const float r = range + 0.0f;
    acc->d_min = hybrid_min(r, acc->d_min);
    if (bc >= q.front_cos) acc->d_front = hybrid_min(r, acc->d_front);
    if (r < kHybridRangeMax && !rb.at_goal) {
        const float px = r * bc, py = r * bs;
        const float t = px * rb.ux + py * rb.uy;
        const float l = px * rb.uy - py * rb.ux;
        if (t >= 0.0f && t <= rb.reach && fabsf(l) < q.corridor) {
            acc->n_block += 1;
            acc->d_block = hybrid_min(r, acc->d_block);
        }
    }
}

// x into [lo, hi] (lo <= hi); a NaN becomes lo
MRCA_HD float hybrid_clamp(float x, float lo, float hi) { return !(x > lo) ? lo : (x < hi ? x : hi); }

// the command and the mode from what the beams added up to; (vp, wp) the incoming command
MRCA_HD void hybrid_result(const HybridParams& q, const HybridRobot& rb, const HybridAcc& acc, float vp, float wp, float* v, float* w,
                           int* mode) {
    if (rb.at_goal) {
        *v = 0.0f;
        *w = 0.0f;
        *mode = kHybridAtGoal;
    } else if (acc.d_min < q.risk_dist) {
        const float s = hybrid_clamp((acc.d_front - q.stop_dist) / (q.risk_dist - q.stop_dist), 0.0f, q.safe_scale);
        *v = vp * s;
        *w = wp;
        *mode = kHybridEmergent;
    } else if (acc.n_block == 0) {
        orca_command(q.v_pid * rb.ux, q.v_pid * rb.uy, 0.0f, 1.0f, q.max_speed, q.k_omega, v, w);
        *mode = kHybridSimple;
    } else {
        *v = vp;
        *w = wp;
        *mode = kHybridNormal;
    }
}

// ---- the rule as a plain loop.  The kernel runs the same pieces with a beam per lane and one wave reduction.

// The whole rule for one robot: goal = its MRCA_F_LOCAL_GOAL, policy = the incoming (v, omega), ranges = its newest scan row.
// -> cmd (v, omega), mode, clear = (d_min, d_front, d_block).  cmd may be policy itself.
MRCA_HD void hybrid_robot(const HybridParams& q, const float* goal, const float* policy, const float* ranges, int beams, const float* beam_cos,
                          const float* beam_sin, float* cmd, int* mode, float* clear) {
    const HybridRobot rb = hybrid_robot_begin(q, goal[0], goal[1]);
    HybridAcc acc = hybrid_acc_empty();
    for (int b = 0; b < beams; ++b) hybrid_beam(q, rb, ranges[b], beam_cos[b], beam_sin[b], &acc);
    const float vp = policy[0], wp = policy[1];
    hybrid_result(q, rb, acc, vp, wp, &cmd[0], &cmd[1], mode);
    clear[0] = acc.d_min;
    clear[1] = acc.d_front;
    clear[2] = acc.d_block;
}

}  // namespace mrca
