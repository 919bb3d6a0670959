// mrca_planner_device.h -- the rule of the global planner (mrca_goal_fields, mrca_subgoals), stated once for the
// gfx950 kernels of mrca_planner.hip and for a plain host build (tests/test_planner_host.py drives the same functions through g++).
//
// The idea is the two-level navigation of Fan, Long, Liu, Pan (IJRR 2020, long-range navigation): a global planner hands the
// learned local policy a SUBGOAL a little way down the shortest path, in place of the goal itself.  Here: per goal point a FIELD
// of integer path lengths over a coarsened copy of the env's map, planned once per goal set, and per robot and tick a short WALK
// down that field.
//
// PLANNING GRID.  The env's map coarsened by `stride` s (1..8): planning cell (i, j) covers the map cells
// [s i, s i + s) x [s j, s j + s); PW = ceil(map_w / s), PH = ceil(map_h / s).  The map cell of a point is the env's own rule,
// floorf((x - g.x0) * g.inv_cell); the planning cell is that divided by s.  A point whose map cell lies outside the map
// (or is not a number) is OFF GRID.
//
// BLOCKED.  A planning cell is blocked iff an occupied map cell lies within Chebyshev distance `inflate` (0..64 map cells) of one
// of its map cells; map cells beyond the map are free.  EnvView::cellfield is that Chebyshev distance per map cell, exact up to
// its saturation at 255 and with the same "beyond the map is free": a map cell is near an obstacle iff its byte is <= inflate.
//
// FIELD.  u32 [PH][PW] per goal point p.  D = 0 at p's planning cell, the SEED, blocked or not -- and the seed counts as an
// unblocked cell for everything below (a goal inside the inflation can still be walked into, and past).  A goal off grid has no
// seed.  kPlanInf for every other blocked cell and for every cell no path reaches; every other cell holds the length of the
// shortest 8-connected path to the seed through unblocked cells, a straight step 5, a diagonal step 7, a diagonal step allowed
// only if both cells it squeezes between are unblocked and in the grid.  That is the least solution of
// D(c) = min over allowed steps of D(n) + w -- unique, so ANY order of relaxation, with values of any age, ends in the same words.
// Lengths fit: a path visits a cell once, 7 * 2^28 cells < 2^32.
// The chamfer 5/7 metric OVER-ESTIMATES the Euclidean length of a path by up to 8 % (a step at 26.6 degrees costs 5 + 7 = 12
// for sqrt(5) * 5 = 11.18) and under-estimates a pure diagonal by 1 % (7 for 7.07).  mrca_subgoals does NO line-of-sight
// smoothing: its subgoal is a cell centre `lookahead` steps down the 8-connected path.  mrca_subgoals_los (LINE OF SIGHT, below)
// looks further down the same path and takes the farthest cell the robot's cell sees.
//
// While mrca_goal_fields relaxes, blocked cells hold kPlanWall, which no candidate reads as a length; its last launch turns them
// into kPlanInf.  In the finished field a cell beside a finite unblocked cell is blocked iff it holds kPlanInf (it would
// otherwise be one straight step away), so the walk needs the field alone.
//
// WALK.  For a robot in planning cell c with `lookahead` L (1..256): up to L times, among the allowed steps out of c take the one
// of least D(n) + w(c, n), on ties the lowest direction index in the order E, NE, N, NW, W, SW, S, SE (N is +y); take it only if
// D(n) < D(c).  From a kPlanInf cell (blocked or cut off) every in-grid neighbour with finite D is a candidate, diagonal or not:
// the escape step of a robot standing inside the inflation.  Stop early at D = 0.
//
// RESULT per robot: status 1, the walk reached the seed: the subgoal is the slot's goal point, bit for bit.  status 0: the centre
// of the cell reached, x = g.x0 + ((float)i + 0.5f) * (g.cell * (float)s).  status -1: no slot.  status -2: the robot is off
// grid or no candidate exists at the first step (a field without seed is all kPlanInf: no candidate).  For -1 and -2 the subgoal
// is the robot's own goal, bit for bit.  local = the subgoal in the robot's frame by the expression, and from the sine and cosine,
// the ray cast uses for MRCA_F_LOCAL_GOAL (mrca_raycast_body.h).  dist = (float)D(c_start) * ((g.cell * (float)s) / 5.0f), +inf
// for kPlanInf, off grid and no slot.
//
// LINE OF SIGHT (mrca_subgoals_los).  Integers only.  With `reach` (1..256) beside L: walk as above for up to
// max(L, reach) steps and keep the cells c_0 .. c_W (W steps taken).  A cell is OPEN iff it is in the planning grid and its word
// is not kPlanInf.  visible(c_0, c_m) is the integer supercover line between the two cell centres (McNeill's form): dx = |di|,
// dy = |dj|, err = dx - dy, then dx and dy doubled; err > 0: step in x, err -= dy; err < 0: step in y, err += dx; err == 0: the
// line passes exactly through a lattice corner -- both side cells (i + sx, j) and (i, j + sy) must be open (the walk's
// no-corner-cut rule), then step diagonally, err += dx - dy.  Every cell entered must be open, the last one included; c_0 itself
// is not tested (a robot inside the inflation still sees).  m_vis = the LARGEST m in 1..W with visible(c_0, c_m), 0 if none
// (visibility along a path is not monotone: the largest, not the last before the first failure); m = max(m_vis, min(L, W)), so
// the subgoal is never nearer than the plain walk's.  The four outputs are plan_result's for a walk that ended in c_m; a fifth,
// ahead = (m, m_vis), is (0, 0) for status -1 / -2 and for W = 0.  Two consequences: reach <= L gives mrca_subgoals' four
// outputs bit for bit (W <= L, so m = W); and where D(c_0) is finite and W >= 1, m_vis >= 1 (c_1 is an allowed step: open, and
// if diagonal between two open cells).
//
// Like mrca_device.h: integers, or separately rounded IEEE fp32 steps in a fixed order (-ffp-contract=off).  A NumPy / heapq
// restatement (tests/planner_ref.py, tests/planner_los_ref.py) gives the same words and bits.
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_planner_params (include/mrca_env.h)
struct PlannerParams {
    int32_t stride, inflate, lookahead, max_rounds;
};
// same layout as mrca_los_params
struct LosParams {
    int32_t reach;
};

constexpr uint32_t kPlanInf = 0xFFFFFFFFu;    // blocked, or no path
constexpr uint32_t kPlanWall = 0xFFFFFFFEu;   // blocked, while mrca_goal_fields relaxes (never in a finished field)
constexpr uint32_t kPlanStraight = 5u, kPlanDiagonal = 7u;
constexpr int kPlanTile = 64;                 // a workgroup relaxes kPlanTile x kPlanTile planning cells
constexpr int kPlanSweeps = 64;               // at most this many times per launch
constexpr int kPlanMaxStride = 8, kPlanMaxInflate = 64, kPlanMaxLookahead = 256, kPlanMaxGoals = 4096;
constexpr int kLosMaxReach = 256;             // mrca_los_params::reach, 1..kLosMaxReach
constexpr int kLosMaxPath = 256;              // the longest walk mrca_subgoals_los keeps: max(lookahead, reach)
static_assert(kLosMaxPath >= kPlanMaxLookahead && kLosMaxPath >= kLosMaxReach, "the kept path holds the longest walk");
constexpr int kPlanOnGoal = 1, kPlanOnPath = 0, kPlanNoSlot = -1, kPlanNoPath = -2;

// direction k = 0..7: E, NE, N, NW, W, SW, S, SE (two bits per direction, offset by one)
MRCA_HD int plan_dx(int k) { return (int)((0x901Au >> (2 * k)) & 3u) - 1; }
MRCA_HD int plan_dy(int k) { return (int)((0x01A9u >> (2 * k)) & 3u) - 1; }
MRCA_HD uint32_t plan_step_cost(int k) { return (k & 1) ? kPlanDiagonal : kPlanStraight; }

MRCA_HD int plan_cells(int map_cells, int s) { return (map_cells + s - 1) / s; }

// the map cell of a point -> is it on the grid?  (ix, iy) are 0 where it is not
MRCA_HD bool plan_map_cell(const GridGeom& g, float x, float y, int* ix, int* iy) {
    const float fx = floorf((x - g.x0) * g.inv_cell);
    const float fy = floorf((y - g.y0) * g.inv_cell);
    const bool on = fx >= 0.0f && fx < (float)g.width && fy >= 0.0f && fy < (float)g.height;
    *ix = on ? (int)fx : 0;
    *iy = on ? (int)fy : 0;
    return on;
}

// planning cell (i, j), inside the planning grid, of stride s
MRCA_HD bool plan_blocked(const uint8_t* cellfield, const GridGeom& g, int s, int inflate, int i, int j) {
    const int x1 = imin(s * i + s, g.width), y1 = imin(s * j + s, g.height);
    bool b = false;
    for (int y = s * j; y < y1; ++y)
        for (int x = s * i; x < x1; ++x) b = b || (int)cellfield[(size_t)y * (size_t)g.width + (size_t)x] <= inflate;
    return b;
}

// what mrca_goal_fields starts a cell from
MRCA_HD uint32_t plan_field_init(bool seed, bool blocked) { return seed ? 0u : (blocked ? kPlanWall : kPlanInf); }

// One relaxation of a cell holding `cur` from its eight neighbours n[k] (kPlanWall where the grid ends): the least of cur
// and the allowed steps.  A blocked cell stays what it is; kPlanInf and kPlanWall are no lengths.
MRCA_HD uint32_t plan_relax(uint32_t cur, const uint32_t* n) {
    if (cur == kPlanWall) return cur;
    uint32_t best = cur;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bool ok = n[k] < kPlanWall;
        if (k & 1) ok = ok && n[k - 1] != kPlanWall && n[(k + 1) & 7] != kPlanWall;
        const uint32_t cand = n[k] + plan_step_cost(k);
        best = (ok && cand < best) ? cand : best;
    }
    return best;
}

// ---- the walk

// Direction k as a candidate out of a cell holding dc: dn = D of the neighbour (kPlanInf where the grid ends), da / db = D of the
// two cells a diagonal k squeezes between (directions k - 1 and k + 1).  -> (D(n) + w) << 3 | k, or all ones: no candidate.
// The least key is the step of the rule, ties included.
MRCA_HD uint64_t plan_key(uint32_t dc, uint32_t dn, uint32_t da, uint32_t db, int k) {
    bool ok = dn != kPlanInf;
    if ((k & 1) && dc != kPlanInf) ok = ok && da != kPlanInf && db != kPlanInf;
    return ok ? ((((uint64_t)dn + (uint64_t)plan_step_cost(k)) << 3) | (uint64_t)k) : ~(uint64_t)0;
}
MRCA_HD uint64_t plan_key_min(uint64_t a, uint64_t b) { return b < a ? b : a; }

// the least key of a step -> taken?  (ci, cj, dc) move with it
MRCA_HD bool plan_take(uint64_t key, int* ci, int* cj, uint32_t* dc) {
    const int k = (int)(key & 7u);
    const uint32_t dn = (uint32_t)((key >> 3) - (uint64_t)plan_step_cost(k));
    if (!(dn < *dc)) return false;
    *ci += plan_dx(k);
    *cj += plan_dy(k);
    *dc = dn;
    return true;
}

MRCA_HD float plan_centre(float origin, float cell, int s, int i) { return origin + ((float)i + 0.5f) * (cell * (float)s); }
MRCA_HD float plan_dist(const GridGeom& g, int s, uint32_t d) { return d == kPlanInf ? kInf : (float)d * ((g.cell * (float)s) / 5.0f); }
// get_local_goal as the ray cast states it: (x, y) the robot, (sn, cs) its head record's sine and cosine
MRCA_HD void plan_local(float px, float py, float x, float y, float sn, float cs, float* lx, float* ly) {
    const float gx = px - x, gy = py - y;
    *lx = gx * cs + gy * sn;
    *ly = gy * cs - gx * sn;
}

// what the walk of a robot ends in: the four outputs from the cell reached
struct PlanResult {
    float sx, sy, lx, ly, dist;
    int status;
};
// walked: the robot had a slot and stood on the grid; (ci, cj, dc): where the walk ended; d0: D of its first cell;
// nocand: no candidate at the first step; (slot_gx, slot_gy): the slot's goal point; (gx, gy): MRCA_F_GOAL[n]
MRCA_HD PlanResult plan_result(const GridGeom& g, int s, bool has_slot, bool walked, bool nocand, int ci, int cj, uint32_t dc, uint32_t d0,
                               float slot_gx, float slot_gy, float gx, float gy, float x, float y, float sn, float cs) {
    PlanResult r;
    r.status = !has_slot ? kPlanNoSlot : (!walked || nocand) ? kPlanNoPath : dc == 0u ? kPlanOnGoal : kPlanOnPath;
    r.sx = gx;
    r.sy = gy;
    if (r.status == kPlanOnGoal) {
        r.sx = slot_gx;
        r.sy = slot_gy;
    } else if (r.status == kPlanOnPath) {
        r.sx = plan_centre(g.x0, g.cell, s, ci);
        r.sy = plan_centre(g.y0, g.cell, s, cj);
    }
    plan_local(r.sx, r.sy, x, y, sn, cs, &r.lx, &r.ly);
    r.dist = walked ? plan_dist(g, s, d0) : kInf;
    return r;
}

// ---- the rule as plain loops.  The kernels run the same pieces: a cell per thread and sweep in LDS, a direction per lane.

// the least key out of (ci, cj) holding dc, on field f [ph][pw]
MRCA_HD uint64_t plan_best_step(const uint32_t* f, int pw, int ph, int ci, int cj, uint32_t dc) {
    uint32_t d[8];
    for (int k = 0; k < 8; ++k) {
        const int ni = ci + plan_dx(k), nj = cj + plan_dy(k);
        d[k] = (ni >= 0 && nj >= 0 && ni < pw && nj < ph) ? f[(size_t)nj * (size_t)pw + (size_t)ni] : kPlanInf;
    }
    uint64_t best = ~(uint64_t)0;
    for (int k = 0; k < 8; ++k) best = plan_key_min(best, plan_key(dc, d[k], d[(k + 7) & 7], d[(k + 1) & 7], k));
    return best;
}

// The whole rule for one robot.  f: its slot's field or nullptr (no slot); slot_goal: that slot's goal point; goal =
// MRCA_F_GOAL[n]; pose (x, y); head record (sn, cs).
MRCA_HD PlanResult plan_robot(const GridGeom& g, const PlannerParams& q, const uint32_t* f, const float* slot_goal, const float* goal,
                              float x, float y, float sn, float cs) {
    const int s = q.stride, pw = plan_cells(g.width, s), ph = plan_cells(g.height, s);
    int ix, iy;
    const bool walked = plan_map_cell(g, x, y, &ix, &iy) && f != nullptr;
    int ci = ix / s, cj = iy / s;
    uint32_t dc = walked ? f[(size_t)cj * (size_t)pw + (size_t)ci] : kPlanInf;
    const uint32_t d0 = dc;
    bool nocand = false, live = walked;
    for (int step = 0; step < q.lookahead; ++step) {
        live = live && dc != 0u;
        if (!live) break;
        const uint64_t key = plan_best_step(f, pw, ph, ci, cj, dc);
        if (key == ~(uint64_t)0) {
            nocand = step == 0;
            live = false;
        } else {
            live = plan_take(key, &ci, &cj, &dc);
        }
    }
    return plan_result(g, s, f != nullptr, walked, nocand, ci, cj, dc, d0, f ? slot_goal[0] : 0.0f, f ? slot_goal[1] : 0.0f, goal[0], goal[1],
                       x, y, sn, cs);
}

// ---- line of sight

MRCA_HD bool plan_open(const uint32_t* f, int pw, int ph, int i, int j) {
    return i >= 0 && j >= 0 && i < pw && j < ph && f[(size_t)j * (size_t)pw + (size_t)i] != kPlanInf;
}

// visible(c_0 = (i0, j0), (i1, j1)): the supercover line of the rule.  At most |di| + |dj| cells are entered.
MRCA_HD bool plan_visible(const uint32_t* f, int pw, int ph, int i0, int j0, int i1, int j1) {
    int dx = i1 > i0 ? i1 - i0 : i0 - i1, dy = j1 > j0 ? j1 - j0 : j0 - j1;
    const int sx = i1 > i0 ? 1 : -1, sy = j1 > j0 ? 1 : -1;
    int left = dx + dy;                 // unit steps still to go; a diagonal step is two of them
    int err = dx - dy;
    dx *= 2;
    dy *= 2;
    int i = i0, j = j0;
    bool ok = true;
    for (int t = 0; t < 2 * kLosMaxPath && ok && left > 0; ++t) {
        if (err > 0) {
            i += sx;
            err -= dy;
            left -= 1;
        } else if (err < 0) {
            j += sy;
            err += dx;
            left -= 1;
        } else {
            ok = plan_open(f, pw, ph, i + sx, j) && plan_open(f, pw, ph, i, j + sy);
            i += sx;
            j += sy;
            err += dx - dy;
            left -= 2;
        }
        ok = ok && plan_open(f, pw, ph, i, j);
    }
    return ok;
}

// m of the rule from m_vis, L and W
MRCA_HD int plan_los_choose(int m_vis, int L, int W) { return imax(m_vis, imin(L, W)); }

struct LosResult {
    PlanResult r;
    int m, m_vis;
};

// The whole line-of-sight rule for one robot; the arguments of plan_robot and the reach.  path: 2 * kLosMaxPath ints of scratch.
MRCA_HD LosResult plan_robot_los(const GridGeom& g, const PlannerParams& q, const LosParams& lq, const uint32_t* f, const float* slot_goal,
                                 const float* goal, float x, float y, float sn, float cs, int* path) {
    const int s = q.stride, pw = plan_cells(g.width, s), ph = plan_cells(g.height, s);
    int ix, iy;
    const bool walked = plan_map_cell(g, x, y, &ix, &iy) && f != nullptr;
    const int i0 = ix / s, j0 = iy / s;
    int ci = i0, cj = j0;
    uint32_t dc = walked ? f[(size_t)cj * (size_t)pw + (size_t)ci] : kPlanInf;
    const uint32_t d0 = dc;
    bool nocand = false, live = walked;
    int W = 0;
    const int steps = imax(q.lookahead, lq.reach);
    for (int step = 0; step < steps; ++step) {
        live = live && dc != 0u;
        if (!live) break;
        const uint64_t key = plan_best_step(f, pw, ph, ci, cj, dc);
        if (key == ~(uint64_t)0) {
            nocand = step == 0;
            live = false;
        } else {
            live = plan_take(key, &ci, &cj, &dc);
            if (live) {
                path[2 * W] = ci;
                path[2 * W + 1] = cj;
                ++W;
            }
        }
    }
    int m_vis = 0;
    for (int m = W; m >= 1 && m_vis == 0; --m)
        if (plan_visible(f, pw, ph, i0, j0, path[2 * (m - 1)], path[2 * (m - 1) + 1])) m_vis = m;
    LosResult out;
    out.m = plan_los_choose(m_vis, q.lookahead, W);
    out.m_vis = m_vis;
    if (out.m >= 1) {
        ci = path[2 * (out.m - 1)];
        cj = path[2 * (out.m - 1) + 1];
        dc = f[(size_t)cj * (size_t)pw + (size_t)ci];
    }
    out.r = plan_result(g, s, f != nullptr, walked, nocand, ci, cj, dc, d0, f ? slot_goal[0] : 0.0f, f ? slot_goal[1] : 0.0f, goal[0],
                        goal[1], x, y, sn, cs);
    return out;
}

// One workgroup's share of a launch of mrca_goal_fields, as a loop: tile (ti, tj) of field f [ph][pw] relaxed at most `sweeps`
// times from a COPY of the tile and a one-cell halo (halo: the values the copy takes the halo from -- f itself, or an older
// state of it, which a workgroup may see while its neighbour lowers cells), then the cells that fell stored.  -> 1 if anything
// fell or the sweeps ran out.  scratch: (kPlanTile + 2)^2 words.
MRCA_HD int plan_tile_round(uint32_t* f, const uint32_t* halo, int pw, int ph, int ti, int tj, int sweeps, uint32_t* scratch) {
    const int P = kPlanTile + 2;
    for (int ly = 0; ly < P; ++ly)
        for (int lx = 0; lx < P; ++lx) {
            const int i = ti * kPlanTile + lx - 1, j = tj * kPlanTile + ly - 1;
            const bool in = i >= 0 && j >= 0 && i < pw && j < ph;
            const bool own = lx >= 1 && ly >= 1 && lx <= kPlanTile && ly <= kPlanTile;
            scratch[ly * P + lx] = in ? (own ? f : halo)[(size_t)j * (size_t)pw + (size_t)i] : kPlanWall;
        }
    bool changed = true;
    for (int sweep = 0; sweep < sweeps && changed; ++sweep) {
        changed = false;
        for (int ly = 1; ly <= kPlanTile; ++ly)
            for (int lx = 1; lx <= kPlanTile; ++lx) {
                uint32_t n[8];
                for (int k = 0; k < 8; ++k) n[k] = scratch[(ly + plan_dy(k)) * P + lx + plan_dx(k)];
                const uint32_t v = plan_relax(scratch[ly * P + lx], n);
                changed = changed || v != scratch[ly * P + lx];
                scratch[ly * P + lx] = v;
            }
    }
    bool fell = false;
    for (int ly = 1; ly <= kPlanTile; ++ly)
        for (int lx = 1; lx <= kPlanTile; ++lx) {
            const int i = ti * kPlanTile + lx - 1, j = tj * kPlanTile + ly - 1;
            if (i < pw && j < ph && scratch[ly * P + lx] < f[(size_t)j * (size_t)pw + (size_t)i]) {
                f[(size_t)j * (size_t)pw + (size_t)i] = scratch[ly * P + lx];
                fell = true;
            }
        }
    return (fell || changed) ? 1 : 0;
}

// The bound on the launches of mrca_goal_fields when max_rounds is 0.  Take a shortest path to any cell and cut it where it
// changes tile.  A piece of l cells is final l / kPlanSweeps (rounded up) launches after the cell before it is: a sweep makes
// the next cell of a path final once the one before it is, whatever else is stale.  A path visits a cell once, so its pieces
// have at most 4096 T cells together (T tiles), and every piece but the first begins in one of the 252 border cells of its
// tile: at most 252 T + 1 pieces.  So T (4096 / kPlanSweeps + 252) + 1 launches reach the fixed point, and one more sees that
// nothing changed.  (A bound, not an estimate: the shipped Stage-2 map takes some tens.)
MRCA_HD int64_t plan_round_bound(int pw, int ph) {
    const int64_t T = (int64_t)plan_cells(pw, kPlanTile) * (int64_t)plan_cells(ph, kPlanTile);
    return T * (int64_t)(kPlanTile * kPlanTile / kPlanSweeps + 4 * kPlanTile - 4) + 2;
}

}  // namespace mrca
