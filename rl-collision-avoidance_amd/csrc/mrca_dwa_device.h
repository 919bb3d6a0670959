// mrca_dwa_device.h -- the rule of the DWA baseline controller (mrca_dwa_actions), stated once for the gfx950
// kernel of mrca_dwa.hip and for a plain host build (tests/test_dwa_host.py drives the same functions through g++).
//
// The algorithm is the dynamic window approach of Fox, Burgard, Thrun, "The dynamic window approach to collision avoidance"
// (1997): sample the (v, omega) commands the robot can reach within one tick, roll each out as an arc over a short horizon,
// drop the ones that come closer to an obstacle than the robot's radius, and take the one that scores best on progress to the
// goal, heading, clearance and speed.
//
// It is SENSOR-LEVEL: what it reads is what the policy reads -- the newest lidar scan, the goal in the robot's frame
// (MRCA_F_LOCAL_GOAL) and the robot's own commanded speed (MRCA_F_SPEED).  It does NOT read MRCA_F_HIT_BITS, the poses,
// MRCA_F_SPEED_GT or anything of another robot: a return from a robot is an obstacle like a return from a wall, and every
// obstacle is taken as standing still.  Everything happens in the robot's own frame (x ahead, y to the left), where the scan's
// beam directions (beam_cos / beam_sin) already are.
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 + - * / sqrt or a comparison, in a fixed order
// (-ffp-contract=off, correctly rounded division and square root); the only transcendental is sincos_det and there is no
// atan2.  A NumPy float32 restatement (tests/dwa_ref.py) gives the same bits.
//
// What is written so that the ORDER of evaluation cannot show: a candidate's clearance is a minimum over obstacle points
// (NaN never enters it: `d < m ? d : m`), and the choice is the maximum of a key (score, ~candidate) that is a total order --
// the kernel deals the candidates to the lanes of a wavefront, the host functions below walk them in a loop.
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_dwa_params (include/mrca_env.h)
struct DwaParams {
    float radius, horizon, obst_dist, clear_cap, max_speed, max_omega, acc_v, acc_w, w_goal, w_heading, w_clear, w_speed;
    int32_t steps, nv, nw;
};

constexpr int kDwaSectors = 64;           // obstacle points: the nearest return of each sixty-fourth of the scan, one per lane
constexpr int kDwaMaxSteps = 64;
constexpr int kDwaMaxNv = 16;
constexpr int kDwaMaxNw = 64;
constexpr float kDwaRangeMax = 6.0f;      // the lidar's range: a beam that returns this saw nothing
constexpr int kDwaChoiceBlocked = -1;     // no admissible candidate: stop and turn towards the goal's side
constexpr int kDwaChoiceAtGoal = -2;      // within kGoalRadius of the goal: (0, 0)

// ---- obstacle points

// a return counts below this range
MRCA_HD float dwa_range_cut(float obst_dist) { return obst_dist < kDwaRangeMax ? obst_dist : kDwaRangeMax; }

// the nearest counting return of beams [first, first + per) in ascending order with a strict comparison: the lowest beam
// among equals (-0.0 < 0.0 is false, so a range of -0.0 is a 0 here too).  -> the beam, -1: the sector gives no point
MRCA_HD int dwa_sector_min(const float* ranges, int first, int per, float cut, float* best_range) {
    float br = kInf;
    int bb = -1;
    for (int k = 0; k < per; ++k) {
        const float r = ranges[first + k];
        if (r < cut && r < br) {
            br = r;
            bb = first + k;
        }
    }
    *best_range = br;
    return bb;
}

// the point of a return in the robot's frame; the + 0 makes a range of -0.0 a 0
MRCA_HD void dwa_point(float range, float bc, float bs, float* x, float* y) {
    const float r = range + 0.0f;
    *x = r * bc;
    *y = r * bs;
}

// ---- the window

// x into [lo, hi] (lo <= hi); a NaN becomes lo
MRCA_HD float dwa_clamp(float x, float lo, float hi) { return !(x > lo) ? lo : (x < hi ? x : hi); }

// [vlo, vhi] x [wlo, whi]: what one tick of the acceleration limits leaves of [0, max_speed] x [-max_omega, max_omega]
// around the current command (v0, w0); a command outside that rectangle gives the nearest part of it
MRCA_HD void dwa_window(const DwaParams& q, float v0, float w0, float* vlo, float* vhi, float* wlo, float* whi) {
    const float av = q.acc_v * kDt, aw = q.acc_w * kDt;
    *vhi = dwa_clamp(v0 + av, 0.0f, q.max_speed);
    *vlo = dwa_clamp(v0 - av, 0.0f, *vhi);
    *whi = dwa_clamp(w0 + aw, -q.max_omega, q.max_omega);
    *wlo = dwa_clamp(w0 - aw, -q.max_omega, *whi);
}

// sample i of n, evenly over [lo, hi] with both ends included; n = 1 takes hi.  The lower half is counted from lo and the
// upper half from hi, so a window that is symmetric about 0 gives samples that are: sample n-1-i is exactly minus sample i.
MRCA_HD float dwa_sample(float lo, float hi, int i, int n) {
    if (n == 1) return hi;
    const float span = hi - lo;
    const float den = (float)(n - 1);
    if (2 * i < n - 1) return lo + span * ((float)i / den);
    return hi - span * ((float)(n - 1 - i) / den);
}

// ---- one candidate

// One sub-step of the rollout.  This RESTATES latch_and_integrate's integrator (mrca_device.h: explicit Euler, the position
// advanced with the heading at the start of the step, then the heading wrapped and its sine / cosine taken through
// sincos_det) with a step length of dt: that function's step is fixed at kDt and comes with the command latch.
struct DwaState {
    float x, y, th, s, c;
};
MRCA_HD DwaState dwa_start() { return DwaState{0.0f, 0.0f, 0.0f, 0.0f, 1.0f}; }
MRCA_HD void dwa_advance(DwaState* st, float v, float w, float dt) {
    const float d = v * dt;
    st->x = st->x + d * st->c;
    st->y = st->y + d * st->s;
    st->th = wrap_angle(st->th + w * dt);
    sincos_det(st->th, &st->s, &st->c);
}

// squared distance of a rollout position from one obstacle point, folded into the minimum so far
MRCA_HD float dwa_min_d2(float m, float x, float y, float ox, float oy) {
    const float dx = x - ox, dy = y - oy;
    const float d = dx * dx + dy * dy;
    return d < m ? d : m;
}

// clearance from the least squared distance over all sub-steps and points; with no point at all it is clear_cap
MRCA_HD float dwa_clearance(const DwaParams& q, bool any_point, float min_d2) {
    return any_point ? sqrtf(min_d2) - q.radius : q.clear_cap;
}

// the score of a candidate that ended at `e` with clearance `clear`; (gx, gy) the goal, gl = |g|.  The + 0 at the end makes
// a score of -0.0 a 0: equal scores then have equal bits.
MRCA_HD float dwa_score(const DwaParams& q, const DwaState& e, float v, float clear, float gx, float gy, float gl) {
    const float ex = gx - e.x, ey = gy - e.y;
    const float el = sqrtf(ex * ex + ey * ey);
    const float progress = (gl - el) / (q.max_speed * q.horizon);
    const float align = el == 0.0f ? 1.0f : (e.c * ex + e.s * ey) / el;
    const float cl = clear < q.clear_cap ? clear : q.clear_cap;
    return (((q.w_goal * progress + q.w_heading * align) + q.w_clear * (cl / q.clear_cap)) + q.w_speed * (v / q.max_speed)) + 0.0f;
}

// admissible: the robot's disc stays off every obstacle point (and the score is a number)
MRCA_HD bool dwa_admissible(float clear, float score) { return clear >= 0.0f && score == score; }

// ---- the choice.  key = (order-preserving bits of the score) << 32 | ~c: greater score first, the lower candidate among
// equal scores, in ONE unsigned comparison.  0 is no key (an inadmissible candidate): ~c of c < 2^31 is never 0.
MRCA_HD uint32_t dwa_ordered_bits(float score) {
    uint32_t b;
    __builtin_memcpy(&b, &score, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
MRCA_HD float dwa_ordered_score(uint32_t o) {
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float s;
    __builtin_memcpy(&s, &b, 4);
    return s;
}
MRCA_HD unsigned long long dwa_key(bool admissible, float score, int c) {
    return admissible ? ((unsigned long long)dwa_ordered_bits(score) << 32) | (uint32_t)~c : 0ull;
}

// what is the same for every candidate of a robot
struct DwaRobot {
    float gx, gy, gl;
    float vlo, vhi, wlo, whi;
    float dt;
    bool at_goal;
};
MRCA_HD DwaRobot dwa_robot_begin(const DwaParams& q, float gx, float gy, float v0, float w0) {
    DwaRobot r;
    r.gx = gx;
    r.gy = gy;
    r.gl = sqrtf(gx * gx + gy * gy);
    r.at_goal = r.gl <= kGoalRadius;
    dwa_window(q, v0, w0, &r.vlo, &r.vhi, &r.wlo, &r.whi);
    r.dt = q.horizon / (float)q.steps;
    return r;
}
MRCA_HD void dwa_candidate_command(const DwaParams& q, const DwaRobot& r, int c, float* v, float* w) {
    *v = dwa_sample(r.vlo, r.vhi, c / q.nw, q.nv);
    *w = dwa_sample(r.wlo, r.whi, c % q.nw, q.nw);
}

// candidate c against the obstacle points (px, py)[0 .. n_slots), n_slots a multiple of 4; a slot without a point holds (+inf, 0), which is further
// than anything, and any_point says whether one slot has a point.  The minimum over the points does not depend on their order
// or on how many empty slots stand among them: the host passes the kDwaSectors sectors as they are, the kernel the points
// packed to the front.  -> its key; clear / score (or nullptr) out
MRCA_HD unsigned long long dwa_candidate(const DwaParams& q, const DwaRobot& r, int c, const float* px, const float* py, int n_slots,
                                         bool any_point, float* clear_out, float* score_out) {
    float v, w;
    dwa_candidate_command(q, r, c, &v, &w);
    DwaState st = dwa_start();
    float m = kInf;
    for (int k = 0; k < q.steps; ++k) {
        dwa_advance(&st, v, w, r.dt);
        if (any_point)                       // (without a point the minimum is not looked at: dwa_clearance)
            for (int s = 0; s < n_slots; s += 4) {       // (four at a time: one 16-byte read per coordinate on the device)
                m = dwa_min_d2(m, st.x, st.y, px[s], py[s]);
                m = dwa_min_d2(m, st.x, st.y, px[s + 1], py[s + 1]);
                m = dwa_min_d2(m, st.x, st.y, px[s + 2], py[s + 2]);
                m = dwa_min_d2(m, st.x, st.y, px[s + 3], py[s + 3]);
            }
    }
    const float clear = dwa_clearance(q, any_point, m);
    const float score = dwa_score(q, st, v, clear, r.gx, r.gy, r.gl);
    if (clear_out) *clear_out = clear;
    if (score_out) *score_out = score;
    return dwa_key(dwa_admissible(clear, score), score, c);
}

// the command, the choice and the score that go with the greatest key (0: nobody was admissible)
MRCA_HD void dwa_result(const DwaParams& q, const DwaRobot& r, unsigned long long best, float* cmd, int* choice, float* score) {
    if (r.at_goal) {
        cmd[0] = 0.0f;
        cmd[1] = 0.0f;
        *choice = kDwaChoiceAtGoal;
        *score = 0.0f;
    } else if (best == 0ull) {
        cmd[0] = 0.0f;
        cmd[1] = r.gy >= 0.0f ? q.max_omega : -q.max_omega;
        *choice = kDwaChoiceBlocked;
        *score = 0.0f;
    } else {
        const int c = (int)~(uint32_t)best;
        dwa_candidate_command(q, r, c, &cmd[0], &cmd[1]);
        *choice = c;
        *score = dwa_ordered_score((uint32_t)(best >> 32));
    }
}

// ---- the rule as plain loops.  The kernel runs the same pieces with a sector per lane and the candidates dealt to the lanes.

// the obstacle points of one scan row: px / py [kDwaSectors] (a sector without a point: (+inf, 0)), beam[s] its beam or -1
// -> how many sectors gave a point
MRCA_HD int dwa_points(const float* ranges, int beams, const float* beam_cos, const float* beam_sin, float obst_dist, float* px,
                       float* py, int* beam) {
    const int per = beams / kDwaSectors;
    const float cut = dwa_range_cut(obst_dist);
    int n = 0;
    for (int s = 0; s < kDwaSectors; ++s) {
        float r;
        const int b = dwa_sector_min(ranges, s * per, per, cut, &r);
        px[s] = kInf;
        py[s] = 0.0f;
        if (b >= 0) {
            dwa_point(r, beam_cos[b], beam_sin[b], &px[s], &py[s]);
            ++n;
        }
        if (beam) beam[s] = b;
    }
    return n;
}

// The whole rule for one robot: goal = its MRCA_F_LOCAL_GOAL, speed = its MRCA_F_SPEED, ranges = its newest scan row.
// -> cmd (v, omega), choice, score; diagnostics (or nullptr): pts[kDwaSectors][2], beam[kDwaSectors], and per candidate
// c < nv * nw: adm[c], clear[c], scores[c]
MRCA_HD void dwa_robot(const DwaParams& q, const float* goal, const float* speed, const float* ranges, int beams, const float* beam_cos,
                       const float* beam_sin, float* cmd, int* choice, float* score, float* pts, int* beam, uint8_t* adm, float* clear,
                       float* scores) {
    float px[kDwaSectors], py[kDwaSectors];
    const int n = dwa_points(ranges, beams, beam_cos, beam_sin, q.obst_dist, px, py, beam);
    if (pts)
        for (int s = 0; s < kDwaSectors; ++s) {
            pts[2 * s] = px[s];
            pts[2 * s + 1] = py[s];
        }
    const DwaRobot r = dwa_robot_begin(q, goal[0], goal[1], speed[0], speed[1]);
    unsigned long long best = 0ull;
    if (!r.at_goal || adm) {
        for (int c = 0; c < q.nv * q.nw; ++c) {
            float cl, sc;
            const unsigned long long key = dwa_candidate(q, r, c, px, py, kDwaSectors, n > 0, &cl, &sc);
            best = key > best ? key : best;
            if (adm) {
                adm[c] = key != 0ull;
                clear[c] = cl;
                scores[c] = sc;
            }
        }
    }
    dwa_result(q, r, best, cmd, choice, score);
}

}  // namespace mrca
