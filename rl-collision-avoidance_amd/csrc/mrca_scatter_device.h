// mrca_scatter_device.h -- the rule of the scenario sampler (mrca_scatter), stated once for the gfx950 kernel of
// mrca_scatter.hip and for a plain host build (tests/test_scatter_host.py drives the same functions through g++).
//
// The env's own reset samplers (pose_try / goal_try, mrca_device.h) restate the reference: they test neither the map nor the
// other robots.  This rule produces what mrca_reset(env, mask, poses_dev, goals_dev) accepts -- per world a different set of
// starts and goals that keep a stated distance from each other and from the map, the same bits for the same (seed, draw).
//
// INPUT.  The env's map geometry and EnvView::cellfield (per map cell the Chebyshev distance to the nearest occupied cell,
// saturated at 255, cells beyond the map free: the byte mrca_planner_device.h reads), the env's Philox key, R boxes
// box[i] = (sx0, sy0, sx1, sy1, gx0, gy0, gx1, gy1), one per LOCAL index, shared by all worlds, and ScatterParams.
//
// CANDIDATE k of robot n (the global index; i = n % R its local one):
//   U  = philox4x32_10(n, draw, k, word, key)          word = 3 for starts, 7 for goals
//   x  = x0 + (x1 - x0) * u01(U.x),  y = y0 + (y1 - y0) * u01(U.y)      a box with x0 == x1 pins the coordinate (to x0 + 0)
//   th = wrap_angle(kTwoPi * u01(U.z))                 starts only, pose_try's expression
// The reset sampler's streams use counter word 3 = 0 (pose) and 1 (goal), the noise model's words have the low two bits 2
// (mrca_noise_device.h): a word whose low two bits are 3 meets neither.
//
// CLEAR OF THE MAP (integers only, once the cell is known).  The point's map cell is c = floorf((x - g.x0) * g.inv_cell) per
// axis; a cell that is not a number or beyond +-2^30 is never clear.  Inside the map: v = the byte of c.  Outside: clamp c into
// the map to c' and take v = max(byte(c'), Chebyshev cell distance from c to c').  For an off-map cell and any in-map cell o the
// per-axis distance splits at c' (|c - o| = |c - c'| + |c' - o| on an axis where c is outside, c = c' on the other), so
// Chebyshev(c, o) >= max(Chebyshev(c', o), Chebyshev(c, c')): v is a LOWER bound of the true distance -- the test can refuse
// a valid point and never accepts an invalid one.  Clear iff v > clear_cells.  clear_cells = 0 still refuses occupied cells; in
// an open world (all bytes 255) everything is clear.
//
// APART from a point already placed: !(dx * dx + dy * dy < sep * sep), squares only.  IN THE BAND around the robot's own start:
// d2 >= goal_min * goal_min && d2 <= goal_max * goal_max with the same d2.
//
// SEQUENTIAL DEFINITION (the specification).  In each world, for i = 0 .. R-1 in order, start_i is the candidate of the LEAST
// k < max_tries that is clear and apart (min_sep) from start_j for every j < i.  Then, for i = 0 .. R-1 in order, goal_i is the
// candidate of the least k < max_tries that is clear, in the band around start_i and apart (goal_sep) from goal_j for every
// j < i.  If no k qualifies the robot takes candidate max_tries - 1 as it is (the way sample_pose keeps its last draw), its
// tries entry is -1, and later robots treat it as placed; otherwise tries = k + 1.  The result hangs on (key, draw, boxes,
// params, map) and on nothing else -- not on the launch shape, not on the other worlds.
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 + - * or a comparison, in a fixed order
// (-ffp-contract=off).  A NumPy float32 restatement (tests/scatter_ref.py) gives the same bits.
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_scatter_params (include/mrca_env.h)
struct ScatterParams {
    float min_sep, goal_sep, goal_min, goal_max;
    int32_t clear_cells, max_tries;
    uint32_t draw;
};

constexpr uint32_t kStreamScatterStart = 3u, kStreamScatterGoal = 7u;   // whole counter words; low two bits 3
constexpr int kScatterMaxRobots = 4096;      // a world's placed points are float2[R] in LDS: 32 KB
constexpr int kScatterMaxTries = 65536;
constexpr int kScatterMaxClear = 254;
constexpr float kScatterMinSep = 0.6f;       // two 0.44 x 0.38 footprints cannot meet with centres 2 x 0.2907 m apart
constexpr float kScatterCellLimit = 1073741824.0f;   // 2^30: beyond it a cell index is no integer worth having

struct ScatterXY {
    float x, y;
};
struct ScatterCandidate {
    float x, y, th;
};

// candidate k of robot gid in the box (x0, y0, x1, y1) on stream `word`
MRCA_HD ScatterCandidate scatter_candidate(const float* box, uint32_t gid, uint32_t draw, uint32_t k, uint32_t word, uint32_t k0,
                                           uint32_t k1) {
    const U4 r = philox4x32_10(gid, draw, k, word, k0, k1);
    ScatterCandidate c;
    c.x = box[0] + (box[2] - box[0]) * u01(r.x);
    c.y = box[1] + (box[3] - box[1]) * u01(r.y);
    c.th = wrap_angle(kTwoPi * u01(r.z));
    return c;
}

// the clearance value v of a point (0 for a cell that is no number)
MRCA_HD int scatter_clearance(const uint8_t* cellfield, const GridGeom& g, float x, float y) {
    const float fx = floorf((x - g.x0) * g.inv_cell);
    const float fy = floorf((y - g.y0) * g.inv_cell);
    if (!(fx >= -kScatterCellLimit && fx <= kScatterCellLimit && fy >= -kScatterCellLimit && fy <= kScatterCellLimit)) return 0;
    const int cx = (int)fx, cy = (int)fy;
    const int qx = cx < 0 ? 0 : (cx > g.width - 1 ? g.width - 1 : cx);
    const int qy = cy < 0 ? 0 : (cy > g.height - 1 ? g.height - 1 : cy);
    const int ox = cx > qx ? cx - qx : qx - cx, oy = cy > qy ? cy - qy : qy - cy;
    const int off = ox > oy ? ox : oy;
    const int byte = (int)cellfield[(size_t)qy * (size_t)g.width + (size_t)qx];
    return byte > off ? byte : off;
}

MRCA_HD bool scatter_clear(const uint8_t* cellfield, const GridGeom& g, int clear_cells, float x, float y) {
    return scatter_clearance(cellfield, g, x, y) > clear_cells;
}

MRCA_HD float scatter_dist2(float x, float y, float px, float py) {
    const float dx = x - px, dy = y - py;
    return dx * dx + dy * dy;
}

MRCA_HD bool scatter_apart(float x, float y, const ScatterXY& p, float sep2) { return !(scatter_dist2(x, y, p.x, p.y) < sep2); }

MRCA_HD bool scatter_in_band(float x, float y, float sx, float sy, float lo2, float hi2) {
    const float d2 = scatter_dist2(x, y, sx, sy);
    return d2 >= lo2 && d2 <= hi2;
}

// ---- the rule as a plain loop over ONE world.  The kernel runs the same pieces with a candidate per lane and a ballot per round.

// world w of R robots: poses [R,3], goals [R,2] and tries [R,2] (or nullptr) are that world's rows; placed is scratch [R]
MRCA_HD void scatter_world(const ScatterParams& p, const GridGeom& g, const uint8_t* cellfield, uint32_t k0, uint32_t k1, int R,
                           int w, const float* boxes, float* poses, float* goals, int32_t* tries, ScatterXY* placed) {
    const float min2 = p.min_sep * p.min_sep, sep2 = p.goal_sep * p.goal_sep;
    const float lo2 = p.goal_min * p.goal_min, hi2 = p.goal_max * p.goal_max;
    for (int phase = 0; phase < 2; ++phase)
        for (int i = 0; i < R; ++i) {
            const uint32_t gid = (uint32_t)w * (uint32_t)R + (uint32_t)i;
            const float* box = boxes + 8 * i + 4 * phase;
            ScatterCandidate c{};
            int found = -1;
            for (int k = 0; k < p.max_tries && found < 0; ++k) {
                c = scatter_candidate(box, gid, p.draw, (uint32_t)k, phase ? kStreamScatterGoal : kStreamScatterStart, k0, k1);
                bool ok = scatter_clear(cellfield, g, p.clear_cells, c.x, c.y);
                if (phase) ok = ok && scatter_in_band(c.x, c.y, poses[3 * i], poses[3 * i + 1], lo2, hi2);
                for (int j = 0; j < i && ok; ++j) ok = scatter_apart(c.x, c.y, placed[j], phase ? sep2 : min2);
                if (ok) found = k;
            }
            // (no k qualified: c is candidate max_tries - 1, the last one tried)
            placed[i] = ScatterXY{c.x, c.y};
            if (phase) {
                goals[2 * i] = c.x;
                goals[2 * i + 1] = c.y;
            } else {
                poses[3 * i] = c.x;
                poses[3 * i + 1] = c.y;
                poses[3 * i + 2] = c.th;
            }
            if (tries) tries[2 * i + phase] = found < 0 ? -1 : found + 1;
        }
}

}  // namespace mrca
