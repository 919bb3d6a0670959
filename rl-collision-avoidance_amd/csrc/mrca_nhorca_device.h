// mrca_nhorca_device.h -- the rule of the NH-ORCA baseline controller (mrca_nhorca_actions), stated once for the
// gfx950 kernel of mrca_orca.hip (orca_kernel<BIG, true>) and for a plain host build (tests/test_nhorca_host.py).
//
// Alonso-Mora, Breitenmoser, Rufli, Beardsley, Siegwart, "Optimal reciprocal collision avoidance for multiple non-holonomic
// robots": ORCA may choose only holonomic velocities that the unicycle can track within a bound eps, and every disc grows by
// eps.  A unicycle tracks the velocity of speed u at angle th from its heading by turning at omega = th / T with the forward
// speed u (th/2) / tan(th/2); over [0, T] its distance from the point that moves at that velocity peaks at t = T and is
// T u |sin(th/2)|.  So inside the cone |th| <= th_max = min(T w_max, pi/2) and the disc |v| <= eps / (T sin(th_max/2)) the
// error is at most eps: a convex set, which enters the linear program of mrca_orca_device.h as two lines and a radius.
//
// Everything of ORCA is that header's, unchanged: orca_constraint, orca_solve, the sectors, the neighbour selection, the
// preferred velocity.  Like there, every step is a separately rounded fp32 + - * / sqrt or a comparison in a fixed order; the
// angles go through sincos_det and atan2_approx (mrca_device.h), no libm.  tests/nhorca_ref.py gives the same bits.
#pragma once
#include "mrca_orca_device.h"

namespace mrca {

// same layout as mrca_nhorca_params (include/mrca_env.h): ORCA's eleven fields (k_omega is not used), then the two of the tracking
struct NhOrcaParams {
    OrcaParams o;
    float track_error;      // eps [m]
    float track_time;       // T [s]
};

constexpr int kNhHeadingLines = 2;                                        // they come first and are hard, like the static lines
constexpr int kNhMaxNeighbors = kOrcaMaxNeighbors - kNhHeadingLines;      // 2 + 16 + 46 = 64 constraints: one per lane
constexpr float kNhOmegaMax = 1.0f;                                       // the env's turn-rate bound [rad/s]
constexpr float kNhStraight = 1e-3f;                                      // |th| below this: the arc is the chord

enum NhOrcaMode { kNhTrack = 0, kNhTurn = 1, kNhStillMode = 2, kNhEvade = 3 };

// what the params give once, the same for every robot
struct NhOrcaDerived {
    float sm, cm;           // sin, cos of th_max
    float u_cap;            // the tracked solve's speed bound
    float radius;           // Rr = radius + eps
};

MRCA_HD NhOrcaDerived nhorca_derive(const NhOrcaParams& q) {
    NhOrcaDerived d;
    const float tw = q.track_time * kNhOmegaMax;
    const float th_max = tw < 0.5f * kPi ? tw : 0.5f * kPi;
    sincos_det(th_max, &d.sm, &d.cm);
    float sh, ch;
    sincos_det(0.5f * th_max, &sh, &ch);
    const float cap = q.track_error / (q.track_time * sh);
    d.u_cap = q.o.max_speed < cap ? q.o.max_speed : cap;
    d.radius = q.o.radius + q.track_error;
    return d;
}

// the two heading lines of a robot whose heading is (c, s): through the origin, left edge first; det(d, p - v) <= 0 keeps v
// inside the cone
MRCA_HD void nhorca_heading_lines(float s, float c, float sm, float cm, OrcaLine* left, OrcaLine* right) {
    left->px = 0.0f;
    left->py = 0.0f;
    left->dx = -(c * cm - s * sm);
    left->dy = -(s * cm + c * sm);
    right->px = 0.0f;
    right->py = 0.0f;
    right->dx = c * cm + s * sm;
    right->dy = s * cm - c * sm;
}

// (x, y), of length n, lies inside the cone around the heading (c, s)
MRCA_HD bool nhorca_inside(float x, float y, float n, float s, float c, float cm) { return c * x + s * y >= cm * n; }

MRCA_HD float nhorca_side(float x, float y, float s, float c) { return c * y - s * x >= 0.0f ? 1.0f : -1.0f; }

// Between the two solves: S1 = the free solve's velocity, o = the preferred velocity.  -> true: the tracked solve aims at o,
// false: at (0, 0); *turn: the way to turn in place should the tracked solve stand still
MRCA_HD bool nhorca_aim(float s1x, float s1y, float ox, float oy, float s, float c, float cm, float* turn) {
    const float n1 = sqrtf(dot2(s1x, s1y, s1x, s1y));
    *turn = 0.0f;
    if (n1 >= kOrcaStill) {
        if (nhorca_inside(s1x, s1y, n1, s, c, cm)) return true;
        *turn = nhorca_side(s1x, s1y, s, c);
        return false;
    }
    const float no = sqrtf(dot2(ox, oy, ox, oy));
    if (no > 0.0f && !nhorca_inside(ox, oy, no, s, c, cm)) *turn = nhorca_side(ox, oy, s, c);
    return false;
}

// The tracked solve's velocity S2 -> (v, omega) and the mode.  The half angle comes through tan(th/2) = lat / (u + fwd).
MRCA_HD int nhorca_command(float s2x, float s2y, float s, float c, bool track, float turn, float max_speed, float T, float* v,
                           float* w) {
    const float u = sqrtf(dot2(s2x, s2y, s2x, s2y));
    if (u < kOrcaStill) {
        *v = 0.0f;
        *w = turn;
        return turn != 0.0f ? kNhTurn : kNhStillMode;
    }
    const float fwd = c * s2x + s * s2y;
    const float lat = c * s2y - s * s2x;
    const float th = atan2_approx(lat, fwd);
    const float om = th / T;
    *w = om < -kNhOmegaMax ? -kNhOmegaMax : (om > kNhOmegaMax ? kNhOmegaMax : om);
    const float arc = fabsf(th) < kNhStraight ? u : ((u * (0.5f * th)) * (u + fwd)) / lat;
    *v = arc > 0.0f ? (arc > max_speed ? max_speed : arc) : 0.0f;      // (written so that a NaN is 0)
    return track ? kNhTrack : kNhEvade;
}

// Both solves over lines[0 .. n) = the two heading lines, then n_static static lines, then the robot lines.
// -> the mode; (v, omega) in cmd, S2 in vel.  s1 (or nullptr): the free solve's velocity; diag (or nullptr): the tracked solve's
MRCA_HD int nhorca_solve(const NhOrcaParams& q, const NhOrcaDerived& d, const OrcaLine* lines, int n, int n_static, float s, float c,
                         float ox, float oy, float* cmd, float* vel, float* s1, int* diag) {
    float s1x, s1y;
    orca_solve(lines + kNhHeadingLines, n - kNhHeadingLines, n_static, q.o.max_speed, ox, oy, &s1x, &s1y, nullptr);
    float turn;
    const bool track = nhorca_aim(s1x, s1y, ox, oy, s, c, d.cm, &turn);
    orca_solve(lines, n, kNhHeadingLines + n_static, d.u_cap, track ? ox : 0.0f, track ? oy : 0.0f, &vel[0], &vel[1], diag);
    if (s1) {
        s1[0] = s1x;
        s1[1] = s1y;
    }
    return nhorca_command(vel[0], vel[1], s, c, track, turn, q.o.max_speed, q.track_time, &cmd[0], &cmd[1]);
}

// The rule for robot `local` of one world GIVEN its kept neighbours (orca_robot_with's arguments).
// -> the mode; lines_out / counts (or nullptr): all constraints (the heading lines are lines_out[0] and [1]), [n, n_static]:
// n counts the heading lines, n_static does not
MRCA_HD int nhorca_robot_with(const NhOrcaParams& q, const int* nb, int kept, int local, uint32_t gid, uint32_t k0, uint32_t k1,
                              const float* pose, const float* sincos, const float* speed_gt, const float* goal, const float* ranges,
                              const unsigned long long* hits, int beams, const float* beam_cos, const float* beam_sin, float* cmd,
                              float* vel, float* s1, OrcaLine* lines_out, int* counts, int* diag) {
    OrcaLine lines[kOrcaMaxLines];
    const NhOrcaDerived d = nhorca_derive(q);
    const float s = sincos[2 * local], c = sincos[2 * local + 1];
    float ox, oy;
    orca_pref_velocity(q.o, gid, k0, k1, pose[3 * local], pose[3 * local + 1], goal[0], goal[1], &ox, &oy);
    nhorca_heading_lines(s, c, d.sm, d.cm, &lines[0], &lines[1]);
    int n_static;
    const int n = kNhHeadingLines + orca_lines(q.o, d.radius, nb, kept, local, pose, sincos, speed_gt, ranges, hits, beams, beam_cos,
                                               beam_sin, lines + kNhHeadingLines, &n_static);
    const int mode = nhorca_solve(q, d, lines, n, n_static, s, c, ox, oy, cmd, vel, s1, diag);
    if (lines_out)
        for (int k = 0; k < n; ++k) lines_out[k] = lines[k];
    if (counts) {
        counts[0] = n;
        counts[1] = n_static;
    }
    return mode;
}

// The whole rule for robot `local` of one world: its neighbours among the world's R robots, then nhorca_robot_with.
MRCA_HD int nhorca_robot(const NhOrcaParams& q, int R, int local, uint32_t gid, uint32_t k0, uint32_t k1, const float* pose,
                         const float* sincos, const float* speed_gt, const float* goal, const float* ranges,
                         const unsigned long long* hits, int beams, const float* beam_cos, const float* beam_sin, float* cmd, float* vel,
                         float* s1, OrcaLine* lines_out, int* counts, int* diag) {
    int nb[kOrcaMaxNeighbors];
    const int kept = orca_neighbours_strided(pose, 3, R, local, q.o.neighbor_dist, q.o.max_neighbors, nb);
    return nhorca_robot_with(q, nb, kept, local, gid, k0, k1, pose, sincos, speed_gt, goal, ranges, hits, beams, beam_cos, beam_sin, cmd,
                             vel, s1, lines_out, counts, diag);
}

}  // namespace mrca
