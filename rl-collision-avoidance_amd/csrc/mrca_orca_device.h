// mrca_orca_device.h -- the rule of the ORCA baseline controller (mrca_orca_actions), stated once for the
// gfx950 kernel of mrca_orca.hip and for a plain host build (tests/test_orca_host.py drives the same functions through g++).
//
// The algorithm is van den Berg, Guy, Lin, Manocha, "Reciprocal n-body collision avoidance": every neighbour and every static
// lidar return gives a half plane of permitted velocities, and the new velocity is the one closest to the preferred velocity
// that satisfies them (a 2-D linear program, with a 3-D one that relaxes the robot constraints evenly where they conflict).
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 + - * / sqrt or a comparison, in a fixed order
// (-ffp-contract=off, correctly rounded division and square root); the one angle that is needed goes through sincos_det and
// there is no atan2.  A NumPy float32 restatement (tests/orca_ref.py) gives the same bits.
//
// What is written so that the ORDER of evaluation cannot show: the ends of LP1's interval are a maximum and a minimum over
// the earlier lines (a +0 is added to each, so that the sign of a zero does not depend on which zero came first), and its two
// ways to fail are an "any".  The kernel forms them across a wavefront, the host functions below in a loop.
//
// Wherever |w| is a divisor, |w| = 0 takes unitW = (1, 0).
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_orca_params (include/mrca_env.h)
struct OrcaParams {
    float radius, neighbor_dist, time_horizon, time_horizon_obst, obst_dist, v_pref, max_speed, responsibility, k_omega, jitter;
    int32_t max_neighbors;
};

constexpr int kOrcaSectors = 16;          // static constraints: the nearest wall return of each sixteenth of the scan
constexpr int kOrcaMaxNeighbors = 48;     // 16 + 48 = 64 constraints: one per lane of a wavefront
constexpr int kOrcaMaxLines = kOrcaSectors + kOrcaMaxNeighbors;
constexpr int kOrcaMaxRobots = 64;        // robots per world whose robots are the lanes of ONE wavefront (more: the lidar hash)
constexpr float kOrcaEps = 1e-5f;
constexpr float kOrcaStill = 1e-4f;       // a chosen velocity slower than this is the command (0, 0)
constexpr uint32_t kStreamOrca = 2u;      // Philox stream of the per-robot jitter angle (0 / 1: kStreamPose / kStreamGoal)

// A constraint: the directed line through (px, py) along (dx, dy), |d| = 1; v satisfies it when det(d, p - v) <= 0.
struct OrcaLine {
    float px, py, dx, dy;
};

enum OrcaBranch { kOrcaCircle = 0, kOrcaLegLeft = 1, kOrcaLegRight = 2, kOrcaOverlap = 3 };

MRCA_HD float det2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }
MRCA_HD float dot2(float ax, float ay, float bx, float by) { return ax * bx + ay * by; }

// > 0: velocity (vx, vy) violates the line, by that much
MRCA_HD float orca_violation(const OrcaLine& l, float vx, float vy) { return det2(l.dx, l.dy, l.px - vx, l.py - vy); }

// ---- one constraint.  relPos = p_j - p, relVel = V - V_j, (vx, vy) = V, R the combined radius, inv_t = 1 / horizon.
// -> which branch was taken (enum OrcaBranch)
MRCA_HD int orca_constraint(float rpx, float rpy, float rvx, float rvy, float vx, float vy, float R, float inv_t, float resp,
                            OrcaLine* out) {
    const float dist2 = dot2(rpx, rpy, rpx, rpy);
    const float R2 = R * R;
    float ux, uy, dx, dy;
    int branch;
    bool circle = dist2 <= R2;      // the discs already overlap: the cut-off circle of ONE TICK
    float it = inv_t;
    float wx = 0.0f, wy = 0.0f, w2 = 0.0f;
    if (circle) {
        it = 1.0f / kDt;
        branch = kOrcaOverlap;
        wx = rvx - it * rpx;
        wy = rvy - it * rpy;
        w2 = dot2(wx, wy, wx, wy);
    } else {
        wx = rvx - it * rpx;
        wy = rvy - it * rpy;
        w2 = dot2(wx, wy, wx, wy);
        const float d1 = dot2(wx, wy, rpx, rpy);
        circle = d1 < 0.0f && d1 * d1 > R2 * w2;
        branch = kOrcaCircle;
    }
    if (circle) {
        const float wl = sqrtf(w2);
        const float nx = wl == 0.0f ? 1.0f : wx / wl;
        const float ny = wl == 0.0f ? 0.0f : wy / wl;
        dx = ny;
        dy = -nx;
        const float m = R * it - wl;
        ux = m * nx;
        uy = m * ny;
    } else {
        const float leg = sqrtf(dist2 - R2);
        if (det2(rpx, rpy, wx, wy) > 0.0f) {
            dx = (rpx * leg - rpy * R) / dist2;
            dy = (rpx * R + rpy * leg) / dist2;
            branch = kOrcaLegLeft;
        } else {
            dx = -((rpx * leg + rpy * R) / dist2);
            dy = -((-rpx * R + rpy * leg) / dist2);
            branch = kOrcaLegRight;
        }
        const float d2 = dot2(rvx, rvy, dx, dy);
        ux = d2 * dx - rvx;
        uy = d2 * dy - rvy;
    }
    out->px = vx + resp * ux;
    out->py = vy + resp * uy;
    out->dx = dx;
    out->dy = dy;
    return branch;
}

// ---- LP1 on line k inside the disc |v| <= max_speed, in three pieces.
// begin: the interval the disc leaves of the line; false: the line misses the disc
MRCA_HD bool orca_lp1_begin(const OrcaLine& k, float max_speed, float* tl, float* tr) {
    const float d = dot2(k.px, k.py, k.dx, k.dy);
    const float disc = (d * d + max_speed * max_speed) - dot2(k.px, k.py, k.px, k.py);
    if (disc < 0.0f) return false;
    const float sq = sqrtf(disc);
    *tl = -d - sq;
    *tr = -d + sq;
    return true;
}

// clip by ONE earlier line j: lowers *tr or raises *tl; false: k is parallel to j and lies outside it (LP1 fails)
MRCA_HD bool orca_lp1_clip(const OrcaLine& k, const OrcaLine& j, float* tl, float* tr) {
    const float den = det2(k.dx, k.dy, j.dx, j.dy);
    const float num = det2(j.dx, j.dy, k.px - j.px, k.py - j.py);
    if (fabsf(den) <= kOrcaEps) return !(num < 0.0f);
    const float t = num / den;
    if (den >= 0.0f) *tr = t < *tr ? t : *tr;
    else *tl = t > *tl ? t : *tl;
    return true;
}

// end: the point of the interval that is furthest along opt (dir_opt) or closest to it; false: the interval is empty
MRCA_HD bool orca_lp1_end(const OrcaLine& k, float tl, float tr, float ox, float oy, bool dir_opt, float* rx, float* ry) {
    tl = tl + 0.0f;
    tr = tr + 0.0f;
    if (tl > tr) return false;
    float t;
    if (dir_opt) {
        t = dot2(ox, oy, k.dx, k.dy) > 0.0f ? tr : tl;
    } else {
        t = dot2(k.dx, k.dy, ox - k.px, oy - k.py);
        t = t < tl ? tl : (t > tr ? tr : t);
    }
    *rx = k.px + t * k.dx;
    *ry = k.py + t * k.dy;
    return true;
}

// LP2's starting point
MRCA_HD void orca_lp2_start(float ox, float oy, float max_speed, bool dir_opt, float* rx, float* ry) {
    if (dir_opt) {
        *rx = ox * max_speed;
        *ry = oy * max_speed;
        return;
    }
    const float o2 = dot2(ox, oy, ox, oy);
    if (o2 > max_speed * max_speed) {
        const float ol = sqrtf(o2);
        *rx = (ox * max_speed) / ol;
        *ry = (oy * max_speed) / ol;
    } else {
        *rx = ox;
        *ry = oy;
    }
}

// LP3: robot line j seen from robot line i (j before i); false: parallel and pointing the same way -- no line
MRCA_HD bool orca_project(const OrcaLine& i, const OrcaLine& j, OrcaLine* out) {
    const float D = det2(i.dx, i.dy, j.dx, j.dy);
    if (fabsf(D) <= kOrcaEps) {
        if (dot2(i.dx, i.dy, j.dx, j.dy) > 0.0f) return false;
        out->px = (i.px + j.px) / 2.0f;
        out->py = (i.py + j.py) / 2.0f;
    } else {
        const float t = det2(j.dx, j.dy, i.px - j.px, i.py - j.py) / D;
        out->px = i.px + t * i.dx;
        out->py = i.py + t * i.dy;
    }
    const float ex = j.dx - i.dx, ey = j.dy - i.dy;
    const float el = sqrtf(dot2(ex, ey, ex, ey));
    out->dx = ex / el;
    out->dy = ey / el;
    return true;
}

// ---- the pieces around the solve

// (range, beam) order of the sector minimum: the nearest beam, the lowest one among equals
MRCA_HD bool orca_beam_before(float ra, int ba, float rb, int bb) { return ra < rb || (ra == rb && ba < bb); }

// a beam counts when it returned from the floorplan (hit bit clear) closer than obst_dist
MRCA_HD bool orca_beam_counts(float range, bool hit_robot, float obst_dist) { return !hit_robot && range < obst_dist; }

// the static point of a return, relative to the robot's centre, with the direction formed as the ray cast forms it
MRCA_HD void orca_static_rel(float range, float s, float c, float bc, float bs, float* x, float* y) {
    *x = range * (c * bc - s * bs);
    *y = range * (s * bc + c * bs);
}

// (dist2, index) order of the neighbour selection: total, so equal distances have one answer
MRCA_HD bool orca_key_before(float da, int ja, float db, int jb) { return da < db || (da == db && ja < jb); }

// preferred velocity of robot `gid` (its index in the env) standing at p with goal g; key: the env's seed
MRCA_HD void orca_pref_velocity(const OrcaParams& q, uint32_t gid, uint32_t k0, uint32_t k1, float px, float py, float gx, float gy,
                                float* ox, float* oy) {
    const float dx = gx - px, dy = gy - py;
    const float dist = sqrtf(dot2(dx, dy, dx, dy));
    if (dist <= kGoalRadius) {
        *ox = 0.0f;
        *oy = 0.0f;
        return;
    }
    float x = (q.v_pref * dx) / dist, y = (q.v_pref * dy) / dist;
    if (q.jitter != 0.0f) {
        const U4 r = philox4x32_10(gid, 0u, 0u, kStreamOrca, k0, k1);
        const float a = q.jitter * (2.0f * u01(r.x) - 1.0f);
        float sa, ca;
        sincos_det(a, &sa, &ca);
        const float rx = ca * x - sa * y, ry = sa * x + ca * y;
        x = rx;
        y = ry;
    }
    *ox = x;
    *oy = y;
}

// holonomic velocity -> (v, omega) of a forward-only differential drive; (s, c) the robot's heading
MRCA_HD void orca_command(float vx, float vy, float s, float c, float max_speed, float k_omega, float* v, float* w) {
    const float sp = sqrtf(dot2(vx, vy, vx, vy));
    if (sp < kOrcaStill) {
        *v = 0.0f;
        *w = 0.0f;
        return;
    }
    const float fwd = c * vx + s * vy;
    const float lat = c * vy - s * vx;
    *v = fwd > 0.0f ? (fwd > max_speed ? max_speed : fwd) : 0.0f;
    const float turn = k_omega * (fwd > 0.0f ? lat / sp : (lat >= 0.0f ? 1.0f : -1.0f));
    *w = turn < -1.0f ? -1.0f : (turn > 1.0f ? 1.0f : turn);
}

// ---- the solve as plain loops over an array of lines in contract order (static ones first, then robots nearest first).
// The kernel runs the same pieces with the loop over the earlier lines spread across a wavefront.

MRCA_HD bool orca_lp1(const OrcaLine* lines, int k, float max_speed, float ox, float oy, bool dir_opt, float* rx, float* ry,
                      int* parallel_fail) {
    float tl, tr;
    if (!orca_lp1_begin(lines[k], max_speed, &tl, &tr)) return false;
    bool ok = true;
    for (int j = 0; j < k; ++j)
        if (!orca_lp1_clip(lines[k], lines[j], &tl, &tr)) ok = false;
    if (!ok) {
        if (parallel_fail) *parallel_fail += 1;
        return false;
    }
    return orca_lp1_end(lines[k], tl, tr, ox, oy, dir_opt, rx, ry);
}

// -> n when every line holds, else the first line that could not be satisfied (the result is then the one before it)
MRCA_HD int orca_lp2(const OrcaLine* lines, int n, float max_speed, float ox, float oy, bool dir_opt, float* rx, float* ry,
                     int* parallel_fail) {
    orca_lp2_start(ox, oy, max_speed, dir_opt, rx, ry);
    for (int k = 0; k < n; ++k) {
        if (orca_violation(lines[k], *rx, *ry) > 0.0f) {
            const float tx = *rx, ty = *ry;
            if (!orca_lp1(lines, k, max_speed, ox, oy, dir_opt, rx, ry, parallel_fail)) {
                *rx = tx;
                *ry = ty;
                return k;
            }
        }
    }
    return n;
}

MRCA_HD void orca_lp3(const OrcaLine* lines, int n, int n_static, int begin, float max_speed, float* rx, float* ry) {
    float distance = 0.0f;
    OrcaLine proj[kOrcaMaxLines];
    for (int i = begin; i < n; ++i) {
        if (orca_violation(lines[i], *rx, *ry) > distance) {
            int m = 0;
            for (int j = 0; j < n_static; ++j) proj[m++] = lines[j];
            for (int j = n_static; j < i; ++j)
                if (orca_project(lines[i], lines[j], &proj[m])) ++m;
            const float tx = *rx, ty = *ry;
            if (orca_lp2(proj, m, max_speed, -lines[i].dy, lines[i].dx, true, rx, ry, nullptr) < m) {
                *rx = tx;
                *ry = ty;
            }
            distance = orca_violation(lines[i], *rx, *ry);
        }
    }
}

// diag (or nullptr): [0] 1 when LP2 fell short, [1] 1 when LP3 changed the result, [2] LP1 failures by the parallel-line rule
MRCA_HD void orca_solve(const OrcaLine* lines, int n, int n_static, float max_speed, float ox, float oy, float* rx, float* ry,
                        int* diag) {
    int pf = 0;
    const int k = orca_lp2(lines, n, max_speed, ox, oy, false, rx, ry, &pf);
    const float bx = *rx, by = *ry;
    if (k < n) orca_lp3(lines, n, n_static, k, max_speed, rx, ry);
    if (diag) {
        diag[0] = k < n;
        diag[1] = k < n && (bx != *rx || by != *ry);
        diag[2] = pf;
    }
}

// sector minima of one scan row: best_range[s] / best_beam[s] (beam -1: the sector gives no constraint)
MRCA_HD void orca_sectors(const float* ranges, const unsigned long long* hits, int beams, float obst_dist, float* best_range,
                          int* best_beam) {
    const int per = beams / kOrcaSectors;
    for (int s = 0; s < kOrcaSectors; ++s) {
        float r = kInf;
        int bb = -1;
        for (int b = s * per; b < (s + 1) * per; ++b) {
            const bool hit = (hits[b >> 6] >> (b & 63)) & 1ull;
            if (orca_beam_counts(ranges[b], hit, obst_dist) && (bb < 0 || orca_beam_before(ranges[b], b, r, bb))) {
                r = ranges[b];
                bb = b;
            }
        }
        best_range[s] = r;
        best_beam[s] = bb;
    }
}

// ---- the neighbour selection.  The key of a candidate is (dist2, index) in the order of orca_key_before, packed into one
// unsigned 64-bit number: dist2 >= 0, and the bits of a non-negative float order as an unsigned integer, so
// (bits(dist2) << 32) | index compares like the pair in ONE comparison and a tie goes to the lower index by itself.
// dist2 = dot2(dx, dy, dx, dy) is a sum of two squares: each square is >= +0 and (+0) + (+0) = +0, so -0.0 (whose bits would
// sort above every positive number) cannot arise; a NaN never passes `dist2 < nd2` and so never gets a key.
constexpr unsigned long long kOrcaNoKey = ~0ull;     // sorts behind every key (its dist2 half is a NaN pattern)

MRCA_HD unsigned long long orca_key(float d2, int j) {
    uint32_t b;
    __builtin_memcpy(&b, &d2, 4);
    return ((unsigned long long)b << 32) | (uint32_t)j;
}
MRCA_HD int orca_key_index(unsigned long long key) { return (int)(uint32_t)key; }

// dist2 of robot j from (px, py): every operation rounded on its own
MRCA_HD float orca_dist2(float px, float py, float xj, float yj) {
    const float dx = xj - px, dy = yj - py;
    return dot2(dx, dy, dx, dy);
}

// Worlds of more than kOrcaMaxRobots robots find their candidates through the lidar hash (mrca_device.h: kLidarCell = 6.5 m
// cells): the (2g + 1)^2 cells around the robot's own.  -> g for a neighbor_dist, 0: too large for three rings.
// Why g * 6.5 - 0.2: two robots whose computed dist2 is below nd^2 are at most nd (1 + 2^-22) apart along x, so their cell
// quotients x / 6.5 differ by at most nd / 6.5 -- as real numbers.  hash_cell_coord computes x * fl(1 / 6.5): the rounded
// reciprocal and the rounded product are each off by at most half an ulp of the quotient.  At |x| = 2.5e5 m (the circle of
// 500 000 robots) the quotient is 38 462, its ulp 2^-8 cell = 0.025 m, so each computed quotient is off by at most 0.025 m
// and their difference by at most 0.05 m (about 0.03 m for one ulp, as the 6.3 / 6.5 pair of the ray cast allows for).
// nd <= g * 6.5 - 0.2 keeps the computed quotients within g of each other with 0.15 m to spare, and two numbers at most g
// apart have floors at most g apart: every neighbour lies in one of the (2g + 1)^2 cells.
constexpr int kOrcaMaxRings = 3;
MRCA_HD int orca_rings(float neighbor_dist) {
    return neighbor_dist <= 6.3f ? 1 : (neighbor_dist <= 12.8f ? 2 : (neighbor_dist <= 19.3f ? 3 : 0));
}

// the kept neighbours of robot `local` among R robots whose (x, y) are pts[stride * j], pts[stride * j + 1], nearest first
// -> their count.  Any R: nothing is stored per robot, a candidate's rank is counted against all others.
MRCA_HD int orca_neighbours_strided(const float* pts, int stride, int R, int local, float neighbor_dist, int max_neighbors, int* out) {
    const float nd2 = neighbor_dist * neighbor_dist;
    const float px = pts[stride * local], py = pts[stride * local + 1];
    int n = 0;
    for (int j = 0; j < R; ++j) {
        const float dj = orca_dist2(px, py, pts[stride * j], pts[stride * j + 1]);
        if (j == local || !(dj < nd2)) continue;
        int rank = 0;
        for (int c = 0; c < R && rank < max_neighbors; ++c) {
            const float dc = orca_dist2(px, py, pts[stride * c], pts[stride * c + 1]);
            if (c != local && dc < nd2 && orca_key_before(dc, c, dj, j)) ++rank;
        }
        if (rank < max_neighbors) {
            out[rank] = j;
            ++n;
        }
    }
    return n;
}

// the kept neighbours of robot `local` among the R robots of its world (pose_xy[R][2]), nearest first -> their count
MRCA_HD int orca_neighbours(const float* pose_xy, int R, int local, float neighbor_dist, int max_neighbors, int* out) {
    return orca_neighbours_strided(pose_xy, 2, R, local, neighbor_dist, max_neighbors, out);
}

// The same list from the lidar hash of an env (lstart[lmask + 2], lsorted[N]: the counting sort of the env's robots by
// hash_bucket(x, y, kLidarCell, world, lmask), in ANY order inside a bucket): robot `n` (index in the env, pose[N][3]) of
// `world`, whose robots are [world * R, (world + 1) * R).  -> the count; out: indices inside the world, nearest first.
// It walks the (2g + 1)^2 cells around n's own, g = orca_rings(neighbor_dist) (which must not be 0).  Buckets alias: several
// cells and several worlds may share one, and one bucket may serve two of the cells asked for -- a robot counts only in the
// cell and the world it really is in (the ray cast's rule, mrca_raycast_body.h), so nobody is listed twice and nobody is lost.
// The keys are totally ordered, so the order in which the candidates are met cannot show.  The kernel (mrca_orca.hip) does the
// same with a wavefront; this is the statement it is held to.
MRCA_HD int orca_neighbours_hashed(const int32_t* lstart, const int32_t* lsorted, int lmask, const float* pose, int world, int R, int n,
                                   float neighbor_dist, int max_neighbors, int* out) {
    const int g = orca_rings(neighbor_dist);
    const float nd2 = neighbor_dist * neighbor_dist;
    const float px = pose[3 * (size_t)n], py = pose[3 * (size_t)n + 1];
    const int icx = hash_cell_coord(px, kLidarCell), icy = hash_cell_coord(py, kLidarCell);
    unsigned long long best[kOrcaMaxNeighbors];
    int kept = 0;
    for (int qy = icy - g; qy <= icy + g; ++qy)
        for (int qx = icx - g; qx <= icx + g; ++qx) {
            const uint32_t h = hash_cell(qx, qy, world) & (uint32_t)lmask;
            for (int k = lstart[h]; k < lstart[h + 1]; ++k) {
                const int j = lsorted[k];
                if (j == n || j / R != world) continue;
                const float xj = pose[3 * (size_t)j], yj = pose[3 * (size_t)j + 1];
                if (hash_cell_coord(xj, kLidarCell) != qx || hash_cell_coord(yj, kLidarCell) != qy) continue;
                const float d2 = orca_dist2(px, py, xj, yj);
                if (!(d2 < nd2)) continue;
                const unsigned long long key = orca_key(d2, j);
                int at = kept;                        // insertion into the sorted best-so-far
                while (at > 0 && key < best[at - 1]) --at;
                if (at >= max_neighbors) continue;
                const int last = kept < max_neighbors ? kept : max_neighbors - 1;
                for (int m = last; m > at; --m) best[m] = best[m - 1];
                best[at] = key;
                if (kept < max_neighbors) ++kept;
            }
        }
    for (int k = 0; k < kept; ++k) out[k] = orca_key_index(best[k]) - world * R;
    return kept;
}

// The constraints of robot `local` of one world in contract order (the static lines of its newest scan row, then its kept
// neighbours nb[0 .. kept), nearest first), every disc of radius `radius`.  -> their count; *n_static_out: the static ones
MRCA_HD int orca_lines(const OrcaParams& q, float radius, const int* nb, int kept, int local, const float* pose, const float* sincos,
                       const float* speed_gt, const float* ranges, const unsigned long long* hits, int beams, const float* beam_cos,
                       const float* beam_sin, OrcaLine* lines, int* n_static_out) {
    const float px = pose[3 * local], py = pose[3 * local + 1];
    const float s = sincos[2 * local], c = sincos[2 * local + 1];
    const float sp = speed_gt[2 * local];
    const float vx = sp * c, vy = sp * s;
    int n = 0;
    float br[kOrcaSectors];
    int bb[kOrcaSectors];
    orca_sectors(ranges, hits, beams, q.obst_dist, br, bb);
    const float inv_to = 1.0f / q.time_horizon_obst;
    for (int k = 0; k < kOrcaSectors; ++k) {
        if (bb[k] < 0) continue;
        float rx, ry;
        orca_static_rel(br[k], s, c, beam_cos[bb[k]], beam_sin[bb[k]], &rx, &ry);
        orca_constraint(rx, ry, vx, vy, vx, vy, radius, inv_to, 1.0f, &lines[n++]);
    }
    *n_static_out = n;
    const float inv_t = 1.0f / q.time_horizon;
    for (int k = 0; k < kept; ++k) {
        const int j = nb[k];
        const float sj = speed_gt[2 * j];
        const float vjx = sj * sincos[2 * j + 1], vjy = sj * sincos[2 * j];
        orca_constraint(pose[3 * j] - px, pose[3 * j + 1] - py, vx - vjx, vy - vjy, vx, vy, 2.0f * radius, inv_t, q.responsibility,
                        &lines[n++]);
    }
    return n;
}

// The rule for robot `local` of one world GIVEN its kept neighbours nb[0 .. kept) (indices inside the world, nearest first).
// pose[R][3], sincos[R][2] = the head records' (sin, cos), speed_gt[R][2], goal = this robot's, ranges / hits = its newest scan
// row and hit words, gid = its index in the env.
// -> (v, omega) in cmd, the holonomic velocity in vel; lines_out / counts (or nullptr): the constraints, [n, n_static]
MRCA_HD void orca_robot_with(const OrcaParams& q, const int* nb, int kept, int local, uint32_t gid, uint32_t k0, uint32_t k1,
                             const float* pose, const float* sincos, const float* speed_gt, const float* goal, const float* ranges,
                             const unsigned long long* hits, int beams, const float* beam_cos, const float* beam_sin, float* cmd,
                             float* vel, OrcaLine* lines_out, int* counts, int* diag) {
    OrcaLine lines[kOrcaMaxLines];
    const float s = sincos[2 * local], c = sincos[2 * local + 1];
    float ox, oy;
    orca_pref_velocity(q, gid, k0, k1, pose[3 * local], pose[3 * local + 1], goal[0], goal[1], &ox, &oy);
    int n_static;
    const int n = orca_lines(q, q.radius, nb, kept, local, pose, sincos, speed_gt, ranges, hits, beams, beam_cos, beam_sin, lines,
                             &n_static);
    float rx, ry;
    orca_solve(lines, n, n_static, q.max_speed, ox, oy, &rx, &ry, diag);
    vel[0] = rx;
    vel[1] = ry;
    orca_command(rx, ry, s, c, q.max_speed, q.k_omega, &cmd[0], &cmd[1]);
    if (lines_out)
        for (int k = 0; k < n; ++k) lines_out[k] = lines[k];
    if (counts) {
        counts[0] = n;
        counts[1] = n_static;
    }
}

// The whole rule for robot `local` of one world: its neighbours among the world's R robots, then orca_robot_with.
MRCA_HD void orca_robot(const OrcaParams& q, int R, int local, uint32_t gid, uint32_t k0, uint32_t k1, const float* pose,
                        const float* sincos, const float* speed_gt, const float* goal, const float* ranges,
                        const unsigned long long* hits, int beams, const float* beam_cos, const float* beam_sin, float* cmd,
                        float* vel, OrcaLine* lines_out, int* counts, int* diag) {
    int nb[kOrcaMaxNeighbors];
    const int kept = orca_neighbours_strided(pose, 3, R, local, q.neighbor_dist, q.max_neighbors, nb);
    orca_robot_with(q, nb, kept, local, gid, k0, k1, pose, sincos, speed_gt, goal, ranges, hits, beams, beam_cos, beam_sin, cmd, vel,
                    lines_out, counts, diag);
}

}  // namespace mrca
