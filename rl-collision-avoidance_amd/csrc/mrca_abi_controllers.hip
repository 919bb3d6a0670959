// mrca_abi_controllers.hip -- host side of include/mrca_env.h for what acts on an env between its ticks: the renderer, the ORCA,
// NH-ORCA and DWA baselines, the lidar noise model, the scenario sampler, hybrid control and the global planner.  Every entry point has one shape -- take the
// params (the caller's or the defaults) through their table, check the pointers, then the env, then launch -- and the pieces
// of that shape are stated once, below.  What can be judged without the env is judged first, in the order it stands here: a
// caller's mistake is named whatever else is wrong.  The env itself is mrca_abi.hip's (mrca_env_state.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "mrca_orca.h"
#include "mrca_dwa.h"
#include "mrca_noise.h"
#include "mrca_hybrid.h"
#include "mrca_safe.h"
#include "mrca_planner.h"
#include "mrca_render.h"
#include "mrca_scatter.h"
#include "mrca_env_state.h"      // (last: its `fail` is a macro)

using namespace mrca::env_state;

namespace {

#define CHECK(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// A params struct's table: a row is a field, the kind of rule and its bounds; the rows are checked in the order they stand in.
enum Kind {
    kFinite,       // "is not finite"
    kAbove,        // "must be > lo"
    kAtLeast,      // "must be >= lo"
    kAtMost,       // "must be <= hi"
    kClosed,       // "outside [lo, hi]"
    kHalfOpen,     // "outside (lo, hi]"
    kIntRange,     // "<value> outside lo..hi" (an int32_t field)
    kIntAtLeast0,  // "<value> is negative" (an int32_t field)
};
struct Rule { size_t offset; const char* name; Kind kind; float lo, hi; };
#define ROW(P, field, ...) {offsetof(P, field), #field, __VA_ARGS__}

int check_int_range(const char* fn, const char* name, int32_t v, int lo, int hi) {
    if (v < lo || v > hi) return fail(MRCA_ERR_INVALID, "%s: %s %d outside %d..%d", fn, name, v, lo, hi);
    return MRCA_OK;
}

template <size_t N> int check_rules(const char* fn, const void* params, const Rule (&rules)[N]) {
    for (const Rule& r : rules) {
        float f;
        int32_t i;
        memcpy(&f, static_cast<const char*>(params) + r.offset, sizeof f);
        memcpy(&i, &f, sizeof i);
        const double lo = r.lo, hi = r.hi;
        switch (r.kind) {
        case kFinite: if (!std::isfinite(f)) return fail(MRCA_ERR_INVALID, "%s: %s is not finite", fn, r.name); break;
        case kAbove: if (!(f > r.lo)) return fail(MRCA_ERR_INVALID, "%s: %s must be > %g", fn, r.name, lo); break;
        case kAtLeast: if (!(f >= r.lo)) return fail(MRCA_ERR_INVALID, "%s: %s must be >= %g", fn, r.name, lo); break;
        case kAtMost: if (!(f <= r.hi)) return fail(MRCA_ERR_INVALID, "%s: %s must be <= %g", fn, r.name, hi); break;
        case kClosed: if (!(f >= r.lo && f <= r.hi)) return fail(MRCA_ERR_INVALID, "%s: %s outside [%g, %g]", fn, r.name, lo, hi); break;
        case kHalfOpen: if (!(f > r.lo && f <= r.hi)) return fail(MRCA_ERR_INVALID, "%s: %s outside (%g, %g]", fn, r.name, lo, hi); break;
        case kIntRange: CHECK(check_int_range(fn, r.name, i, (int)r.lo, (int)r.hi)); break;
        case kIntAtLeast0: if (i < 0) return fail(MRCA_ERR_INVALID, "%s: %s %d is negative", fn, r.name, i); break;
        }
    }
    return MRCA_OK;
}

// A pointer argument: NULL (where it has to be given), then its alignment
int check_ptr(const char* fn, const char* name, const void* ptr, int alignment, bool required) {
    if (required && !ptr) return fail(MRCA_ERR_INVALID, "%s: %s is NULL", fn, name);
    if (reinterpret_cast<uintptr_t>(ptr) % alignment) return fail(MRCA_ERR_INVALID, "%s: %s must be %d-byte aligned", fn, name, alignment);
    return MRCA_OK;
}

// The end of a call: launch() on `device` whatever the caller's current one is
template <class Launch> int launched(int device, Launch&& launch) {
    mrca::DeviceGuard guard(device);
    launch();
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

using Orca = mrca_orca_params;
static_assert(offsetof(Orca, max_neighbors) == offsetof(mrca::OrcaParams, max_neighbors), "mrca_orca_params and mrca::OrcaParams are one layout");
const Rule kOrcaRules[] = {
    ROW(Orca, radius, kFinite), ROW(Orca, neighbor_dist, kFinite), ROW(Orca, time_horizon, kFinite), ROW(Orca, time_horizon_obst, kFinite),
    ROW(Orca, obst_dist, kFinite), ROW(Orca, v_pref, kFinite), ROW(Orca, max_speed, kFinite), ROW(Orca, responsibility, kFinite),
    ROW(Orca, k_omega, kFinite), ROW(Orca, jitter, kFinite),
    ROW(Orca, radius, kAbove, 0), ROW(Orca, neighbor_dist, kAbove, 0), ROW(Orca, time_horizon, kAbove, 0), ROW(Orca, time_horizon_obst, kAbove, 0),
    ROW(Orca, max_speed, kAbove, 0), ROW(Orca, obst_dist, kClosed, 0, 6), ROW(Orca, responsibility, kClosed, 0, 1),
    ROW(Orca, max_neighbors, kIntRange, 0, mrca::kOrcaMaxNeighbors)};
int check(const char* fn, const Orca& p) { return check_rules(fn, &p, kOrcaRules); }

using NhOrca = mrca_nhorca_params;
static_assert(offsetof(NhOrca, max_neighbors) == offsetof(mrca::NhOrcaParams, o.max_neighbors) &&
                  offsetof(NhOrca, track_time) == offsetof(mrca::NhOrcaParams, track_time),
              "mrca_nhorca_params and mrca::NhOrcaParams are one layout");
// (ORCA's rules for ORCA's fields, in ORCA's order; max_neighbors has its own bound here and comes last)
const Rule kNhOrcaRules[] = {
    ROW(NhOrca, radius, kFinite), ROW(NhOrca, neighbor_dist, kFinite), ROW(NhOrca, time_horizon, kFinite), ROW(NhOrca, time_horizon_obst, kFinite),
    ROW(NhOrca, obst_dist, kFinite), ROW(NhOrca, v_pref, kFinite), ROW(NhOrca, max_speed, kFinite), ROW(NhOrca, responsibility, kFinite),
    ROW(NhOrca, k_omega, kFinite), ROW(NhOrca, jitter, kFinite), ROW(NhOrca, track_error, kFinite), ROW(NhOrca, track_time, kFinite),
    ROW(NhOrca, radius, kAbove, 0), ROW(NhOrca, neighbor_dist, kAbove, 0), ROW(NhOrca, time_horizon, kAbove, 0),
    ROW(NhOrca, time_horizon_obst, kAbove, 0), ROW(NhOrca, max_speed, kAbove, 0), ROW(NhOrca, obst_dist, kClosed, 0, 6),
    ROW(NhOrca, responsibility, kClosed, 0, 1), ROW(NhOrca, track_error, kHalfOpen, 0, 0.5f), ROW(NhOrca, track_time, kClosed, 0.1f, 1.5f),
    ROW(NhOrca, max_neighbors, kIntRange, 1, mrca::kNhMaxNeighbors)};
int check(const char* fn, const NhOrca& p) { return check_rules(fn, &p, kNhOrcaRules); }

using Dwa = mrca_dwa_params;
static_assert(offsetof(Dwa, steps) == offsetof(mrca::DwaParams, steps) && offsetof(Dwa, nw) == offsetof(mrca::DwaParams, nw),
              "mrca_dwa_params and mrca::DwaParams are one layout");
const Rule kDwaRules[] = {
    ROW(Dwa, radius, kFinite), ROW(Dwa, horizon, kFinite), ROW(Dwa, obst_dist, kFinite), ROW(Dwa, clear_cap, kFinite), ROW(Dwa, max_speed, kFinite),
    ROW(Dwa, max_omega, kFinite), ROW(Dwa, acc_v, kFinite), ROW(Dwa, acc_w, kFinite), ROW(Dwa, w_goal, kFinite), ROW(Dwa, w_heading, kFinite),
    ROW(Dwa, w_clear, kFinite), ROW(Dwa, w_speed, kFinite),
    ROW(Dwa, radius, kAbove, 0), ROW(Dwa, horizon, kAbove, 0), ROW(Dwa, clear_cap, kAbove, 0), ROW(Dwa, max_speed, kAbove, 0), ROW(Dwa, max_omega, kAbove, 0),
    ROW(Dwa, max_speed, kAtMost, 0, 1), ROW(Dwa, max_omega, kAtMost, 0, 1), ROW(Dwa, obst_dist, kClosed, 0, 6),
    ROW(Dwa, acc_v, kAtLeast, 0), ROW(Dwa, acc_w, kAtLeast, 0), ROW(Dwa, w_goal, kAtLeast, 0), ROW(Dwa, w_heading, kAtLeast, 0), ROW(Dwa, w_clear, kAtLeast, 0),
    ROW(Dwa, w_speed, kAtLeast, 0),
    ROW(Dwa, steps, kIntRange, 1, mrca::kDwaMaxSteps), ROW(Dwa, nv, kIntRange, 1, mrca::kDwaMaxNv), ROW(Dwa, nw, kIntRange, 1, mrca::kDwaMaxNw)};
int check(const char* fn, const Dwa& p) { return check_rules(fn, &p, kDwaRules); }

using Noise = mrca_scan_noise_params;
static_assert(offsetof(Noise, quantum) == offsetof(mrca::ScanNoiseParams, quantum), "mrca_scan_noise_params and mrca::ScanNoiseParams are one layout");
const Rule kNoiseRules[] = {
    ROW(Noise, sigma_const, kFinite), ROW(Noise, sigma_prop, kFinite), ROW(Noise, dropout, kFinite), ROW(Noise, quantum, kFinite),
    ROW(Noise, sigma_const, kClosed, 0, 6), ROW(Noise, sigma_prop, kClosed, 0, 1), ROW(Noise, dropout, kClosed, 0, 1), ROW(Noise, quantum, kClosed, 0, 1)};
int check(const char* fn, const Noise& p) { return check_rules(fn, &p, kNoiseRules); }

using Hybrid = mrca_hybrid_params;
static_assert(offsetof(Hybrid, max_speed) == offsetof(mrca::HybridParams, max_speed), "mrca_hybrid_params and mrca::HybridParams are one layout");
const Rule kHybridFirst[] = {
    ROW(Hybrid, risk_dist, kFinite), ROW(Hybrid, stop_dist, kFinite), ROW(Hybrid, safe_scale, kFinite), ROW(Hybrid, corridor, kFinite),
    ROW(Hybrid, look, kFinite), ROW(Hybrid, front_cos, kFinite), ROW(Hybrid, v_pid, kFinite), ROW(Hybrid, k_omega, kFinite), ROW(Hybrid, max_speed, kFinite),
    ROW(Hybrid, stop_dist, kAtLeast, 0)};
const Rule kHybridRest[] = {
    ROW(Hybrid, risk_dist, kAtMost, 0, 6), ROW(Hybrid, safe_scale, kClosed, 0, 1), ROW(Hybrid, corridor, kAbove, 0), ROW(Hybrid, look, kHalfOpen, 0, 6),
    ROW(Hybrid, front_cos, kClosed, -1, 1), ROW(Hybrid, v_pid, kAbove, 0), ROW(Hybrid, k_omega, kAtLeast, 0), ROW(Hybrid, max_speed, kHalfOpen, 0, 1)};
int check(const char* fn, const Hybrid& p) {
    CHECK(check_rules(fn, &p, kHybridFirst));
    if (!(p.stop_dist < p.risk_dist)) return fail(MRCA_ERR_INVALID, "%s: risk_dist must be > stop_dist", fn);
    return check_rules(fn, &p, kHybridRest);
}

using Safe = mrca_safe_policy_params;
static_assert(offsetof(Safe, v_cap) == offsetof(mrca::SafeParams, v_cap), "mrca_safe_policy_params and mrca::SafeParams are one layout");
const Rule kSafeRules[] = {ROW(Safe, scan_scale, kFinite), ROW(Safe, v_cap, kFinite), ROW(Safe, scan_scale, kHalfOpen, 0, 1), ROW(Safe, v_cap, kHalfOpen, 0, 1)};
int check(const char* fn, const Safe& p) { return check_rules(fn, &p, kSafeRules); }

using Planner = mrca_planner_params;
static_assert(offsetof(Planner, max_rounds) == offsetof(mrca::PlannerParams, max_rounds), "mrca_planner_params and mrca::PlannerParams are one layout");
const Rule kPlannerRules[] = {
    ROW(Planner, stride, kIntRange, 1, mrca::kPlanMaxStride), ROW(Planner, inflate, kIntRange, 0, mrca::kPlanMaxInflate),
    ROW(Planner, lookahead, kIntRange, 1, mrca::kPlanMaxLookahead), ROW(Planner, max_rounds, kIntAtLeast0)};
int check(const char* fn, const Planner& p) { return check_rules(fn, &p, kPlannerRules); }

using Los = mrca_los_params;
static_assert(offsetof(Los, reach) == offsetof(mrca::LosParams, reach), "mrca_los_params and mrca::LosParams are one layout");
// (mrca_subgoals_los keeps a planning cell as two 16-bit halves of a word: mrca_create takes no map side above 16384 cells)
const Rule kLosRules[] = {ROW(Los, reach, kIntRange, 1, mrca::kLosMaxReach)};
int check(const char* fn, const Los& p) { return check_rules(fn, &p, kLosRules); }

using Scatter = mrca_scatter_params;
static_assert(offsetof(Scatter, draw) == offsetof(mrca::ScatterParams, draw), "mrca_scatter_params and mrca::ScatterParams are one layout");
const Rule kScatterFirst[] = {
    ROW(Scatter, min_sep, kFinite), ROW(Scatter, goal_sep, kFinite), ROW(Scatter, goal_min, kFinite), ROW(Scatter, goal_max, kFinite),
    ROW(Scatter, min_sep, kAtLeast, mrca::kScatterMinSep), ROW(Scatter, goal_sep, kAtLeast, 0), ROW(Scatter, goal_min, kAtLeast, 0)};
const Rule kScatterRest[] = {
    ROW(Scatter, clear_cells, kIntRange, 0, mrca::kScatterMaxClear), ROW(Scatter, max_tries, kIntRange, 1, mrca::kScatterMaxTries)};
int check(const char* fn, const Scatter& p) {
    CHECK(check_rules(fn, &p, kScatterFirst));
    if (!(p.goal_min <= p.goal_max)) return fail(MRCA_ERR_INVALID, "%s: goal_max must be >= goal_min", fn);
    return check_rules(fn, &p, kScatterRest);
}

// The params of a call as the kernels take them: the caller's (NULL: the defaults), if their table above accepts them
template <class P, class Q> int take_params(const char* fn, const P* given, int (*defaults)(P*), Q* out) {
    static_assert(sizeof(P) == sizeof(Q) && std::is_trivially_copyable<P>::value && std::is_trivially_copyable<Q>::value,
                  "the ABI's struct and the kernels' are one layout");
    P p;
    if (given) p = *given;
    else defaults(&p);
    CHECK(check(fn, p));
    memcpy(out, &p, sizeof p);
    return MRCA_OK;
}

// What mrca_orca_actions and mrca_orca_actions_any check alike (`fn` names the caller) -> *out: the params as the kernels take them
int orca_validate(const char* fn, const mrca_env* env, const mrca_orca_params* params, const float* actions_dev, const float* vel_dev,
                  mrca::OrcaParams* out) {
    CHECK(take_params(fn, params, mrca_orca_default_params, out));
    CHECK(check_ptr(fn, "actions_dev", actions_dev, 8, true));
    CHECK(check_ptr(fn, "vel_dev", vel_dev, 4, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    return MRCA_OK;
}

}  // namespace

extern "C" {

static_assert(sizeof(mrca_render_view) == sizeof(mrca::RenderView) && offsetof(mrca_render_view, m_per_px) == offsetof(mrca::RenderView, m),
              "mrca_render_view and mrca::RenderView are one layout");

int mrca_render(mrca_env* env, const mrca_render_view* views, int32_t num_views, int32_t width, int32_t height, uint32_t layers,
                uint32_t* ids_dev, uint32_t* trail_dev, uint8_t* rgb_dev, void* stream) {
    const char* fn = "mrca_render";
    CHECK(check_int_range(fn, "num_views", num_views, 1, 256));
    CHECK(check_ptr(fn, "views", views, 1, true));
    if (width < 1 || width > 4096 || height < 1 || height > 4096)
        return fail(MRCA_ERR_INVALID, "mrca_render: image size %d x %d outside 1..4096", width, height);
    if (layers & ~(uint32_t)(MRCA_RENDER_MAP | MRCA_RENDER_GOALS | MRCA_RENDER_BODIES | MRCA_RENDER_BEAMS))
        return fail(MRCA_ERR_INVALID, "mrca_render: unknown layer bits 0x%x", layers);
    CHECK(check_ptr(fn, "ids_dev", ids_dev, 1, true));
    if (reinterpret_cast<uintptr_t>(ids_dev) % 4 || reinterpret_cast<uintptr_t>(trail_dev) % 4 || reinterpret_cast<uintptr_t>(rgb_dev) % 4)
        return fail(MRCA_ERR_INVALID, "mrca_render: ids_dev, trail_dev and rgb_dev must be 4-byte aligned");
    for (int32_t v = 0; v < num_views; ++v)
        if (!(views[v].m_per_px > 0.0f) || !std::isfinite(views[v].m_per_px) || !std::isfinite(views[v].cx) || !std::isfinite(views[v].cy))
            return fail(MRCA_ERR_INVALID, "mrca_render: view %d needs a finite centre and a finite positive m_per_px", v);
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    for (int32_t v = 0; v < num_views; ++v)
        if (views[v].world < 0 || views[v].world >= env->cfg.num_worlds)
            return fail(MRCA_ERR_INVALID, "mrca_render: view %d shows world %d of %d", v, views[v].world, env->cfg.num_worlds);
    return launched(env->cfg.device, [&] {
        mrca::launch_render(env->view, reinterpret_cast<const mrca::RenderView*>(views), num_views, width, height, layers, ids_dev, trail_dev,
                            rgb_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_orca_default_params(mrca_orca_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_orca_default_params: out is NULL");
    out->radius = 0.35f;            // the footprint's half diagonal 0.2907 m + a margin
    out->neighbor_dist = 6.0f;
    out->time_horizon = 2.0f;       // (time_horizon, k_omega): tuned on the three closed-loop gates, profiles/orca/defaults.txt
    out->time_horizon_obst = 1.5f;
    out->obst_dist = 3.0f;
    out->v_pref = 1.0f;
    out->max_speed = 1.0f;
    out->responsibility = 0.5f;
    out->k_omega = 6.0f;
    out->jitter = 0.0f;
    out->max_neighbors = 10;
    return MRCA_OK;
}

int mrca_orca_actions(mrca_env* env, const mrca_orca_params* params, const uint8_t* mask_dev, float* actions_dev, float* vel_dev,
                      void* stream) {
    mrca::OrcaParams q;
    CHECK(orca_validate("mrca_orca_actions", env, params, actions_dev, vel_dev, &q));
    if (env->cfg.robots_per_world > mrca::kOrcaMaxRobots)
        return fail(MRCA_ERR_UNSUPPORTED, "mrca_orca_actions: robots_per_world %d > %d", env->cfg.robots_per_world, mrca::kOrcaMaxRobots);
    return launched(env->cfg.device, [&] { mrca::launch_orca(env->view, q, mask_dev, actions_dev, vel_dev, static_cast<hipStream_t>(stream)); });
}

int mrca_orca_actions_any(mrca_env* env, const mrca_orca_params* params, const uint8_t* mask_dev, float* actions_dev,
                          float* vel_dev, void* stream) {
    mrca::OrcaParams q;
    CHECK(orca_validate("mrca_orca_actions_any", env, params, actions_dev, vel_dev, &q));
    const bool big = env->cfg.robots_per_world > mrca::kOrcaMaxRobots;
    if (big && mrca::orca_rings(q.neighbor_dist) == 0)
        return fail(MRCA_ERR_UNSUPPORTED, "mrca_orca_actions_any: neighbor_dist %g > 19.3 with robots_per_world %d > %d (the search "
                                          "looks at three rings of 6.5 m cells at most)",
                    (double)q.neighbor_dist, env->cfg.robots_per_world, mrca::kOrcaMaxRobots);
    if (big && !env->lidar_hash_current)
        return fail(MRCA_ERR_INVALID, "mrca_orca_actions_any: the lidar hash does not describe the current poses -- call "
                                      "mrca_observe_worlds (after mrca_move_worlds) or mrca_reset first (robots_per_world %d > %d)",
                    env->cfg.robots_per_world, mrca::kOrcaMaxRobots);
    return launched(env->cfg.device, [&] {
        if (big) mrca::launch_orca_big(env->view, q, mask_dev, actions_dev, vel_dev, static_cast<hipStream_t>(stream));
        else mrca::launch_orca(env->view, q, mask_dev, actions_dev, vel_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_nhorca_default_params(mrca_nhorca_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_nhorca_default_params: out is NULL");
    mrca_orca_params o;
    mrca_orca_default_params(&o);
    memcpy(out, &o, sizeof o);       // ORCA's eleven fields lead, in ORCA's layout; k_omega is not used
    // (track_error, track_time, jitter): chosen by the sweep over the four closed-loop gates, profiles/nhorca/defaults.txt
    out->track_error = 0.05f;
    out->track_time = 0.3f;
    out->jitter = 0.3f;
    return MRCA_OK;
}

int mrca_nhorca_actions(mrca_env* env, const mrca_nhorca_params* params, const uint8_t* mask_dev, float* actions_dev, float* vel_dev,
                        int32_t* mode_dev, void* stream) {
    const char* fn = "mrca_nhorca_actions";
    mrca::NhOrcaParams q;
    CHECK(take_params(fn, params, mrca_nhorca_default_params, &q));
    CHECK(check_ptr(fn, "actions_dev", actions_dev, 8, true));
    CHECK(check_ptr(fn, "vel_dev", vel_dev, 4, false));
    CHECK(check_ptr(fn, "mode_dev", mode_dev, 4, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    const bool big = env->cfg.robots_per_world > mrca::kOrcaMaxRobots;      // (mrca_orca_actions_any's two rules for big worlds)
    if (big && mrca::orca_rings(q.o.neighbor_dist) == 0)
        return fail(MRCA_ERR_UNSUPPORTED, "mrca_nhorca_actions: neighbor_dist %g > 19.3 with robots_per_world %d > %d (the search "
                                          "looks at three rings of 6.5 m cells at most)",
                    (double)q.o.neighbor_dist, env->cfg.robots_per_world, mrca::kOrcaMaxRobots);
    if (big && !env->lidar_hash_current)
        return fail(MRCA_ERR_INVALID, "mrca_nhorca_actions: the lidar hash does not describe the current poses -- call "
                                      "mrca_observe_worlds (after mrca_move_worlds) or mrca_reset first (robots_per_world %d > %d)",
                    env->cfg.robots_per_world, mrca::kOrcaMaxRobots);
    return launched(env->cfg.device, [&] {
        mrca::launch_nhorca(env->view, q, big, mask_dev, actions_dev, vel_dev, mode_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_dwa_default_params(mrca_dwa_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_dwa_default_params: out is NULL");
    out->radius = 0.35f;            // the footprint's half diagonal 0.2907 m + a margin (as the ORCA baseline)
    out->horizon = 2.0f;            // (horizon, steps, the weights): tuned on the closed-loop gates, profiles/dwa/defaults.txt
    out->obst_dist = 3.0f;
    out->clear_cap = 1.0f;
    out->max_speed = 1.0f;
    out->max_omega = 1.0f;
    out->acc_v = 10.0f;             // the env has no acceleration limit: one tick of these reaches the whole range
    out->acc_w = 20.0f;
    out->w_goal = 1.0f;
    out->w_heading = 0.0f;          // (any weight here makes robots that meet head-on stop and face each other)
    out->w_clear = 0.2f;
    out->w_speed = 0.3f;
    out->steps = 10;
    out->nv = 5;
    out->nw = 21;
    return MRCA_OK;
}

// mrca_dwa_actions and mrca_dwa_actions_goal (`fn` names the caller; goal_dev NULL: MRCA_F_LOCAL_GOAL)
static int dwa_actions(const char* fn, mrca_env* env, const mrca_dwa_params* params, const float* goal_dev, const uint8_t* mask_dev,
                       float* actions_dev, int32_t* choice_dev, float* score_dev, void* stream) {
    mrca::DwaParams q;
    CHECK(take_params(fn, params, mrca_dwa_default_params, &q));
    CHECK(check_ptr(fn, "actions_dev", actions_dev, 8, true));
    CHECK(check_ptr(fn, "choice_dev", choice_dev, 4, false));
    CHECK(check_ptr(fn, "score_dev", score_dev, 4, false));
    CHECK(check_ptr(fn, "goal_dev", goal_dev, 8, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    return launched(env->cfg.device, [&] {
        mrca::launch_dwa(env->view, q, goal_dev, mask_dev, actions_dev, choice_dev, score_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_dwa_actions(mrca_env* env, const mrca_dwa_params* params, const uint8_t* mask_dev, float* actions_dev, int32_t* choice_dev,
                     float* score_dev, void* stream) {
    return dwa_actions("mrca_dwa_actions", env, params, nullptr, mask_dev, actions_dev, choice_dev, score_dev, stream);
}

int mrca_dwa_actions_goal(mrca_env* env, const mrca_dwa_params* params, const uint8_t* mask_dev, float* actions_dev, int32_t* choice_dev,
                          float* score_dev, const float* goal_dev, void* stream) {
    return dwa_actions("mrca_dwa_actions_goal", env, params, goal_dev, mask_dev, actions_dev, choice_dev, score_dev, stream);
}

int mrca_scan_noise_default_params(mrca_scan_noise_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_scan_noise_default_params: out is NULL");
    // a small indoor lidar's order of magnitude (a centimetre, a percent of the range, one beam in two hundred lost), NOT the
    // reference's: Stage is configured without ranger noise
    out->sigma_const = 0.01f;
    out->sigma_prop = 0.01f;
    out->dropout = 0.005f;
    out->quantum = 0.0f;
    return MRCA_OK;
}

int mrca_scan_noise(mrca_env* env, const mrca_scan_noise_params* params, const uint8_t* mask_dev, void* stream) {
    mrca::ScanNoiseParams q;
    CHECK(take_params("mrca_scan_noise", params, mrca_scan_noise_default_params, &q));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!env->reset_seen) return fail(MRCA_ERR_INVALID, "mrca_scan_noise before the first mrca_reset: there is no scan yet");
    if (q.sigma_const == 0.0f && q.sigma_prop == 0.0f && q.dropout == 0.0f && q.quantum == 0.0f) return MRCA_OK;   // nothing to do
    return launched(env->cfg.device, [&] {
        mrca::launch_scan_noise(env->view, q, mask_dev, env->cfg.lazy_obs ? 0 : (MRCA_VIEW_SCAN | MRCA_VIEW_OBS), static_cast<hipStream_t>(stream));
    });
}

int mrca_scatter_default_params(mrca_scatter_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_scatter_default_params: out is NULL");
    out->min_sep = 1.0f;            // a robot's length and a half between two footprints
    out->goal_sep = 1.0f;           // (two goal discs of radius 0.5 m do not overlap)
    out->goal_min = 5.0f;
    out->goal_max = 1.0e4f;         // no upper bound on any map the producer's boxes fit in
    out->clear_cells = 4;           // 0.4 m on 0.1 m cells: the footprint's half diagonal (0.29 m) and a cell of slack
    out->max_tries = 1024;
    out->draw = 0;
    return MRCA_OK;
}

int mrca_scatter(mrca_env* env, const mrca_scatter_params* params, const float* boxes_dev, float* poses_dev, float* goals_dev,
                 int32_t* tries_dev, void* stream) {
    const char* fn = "mrca_scatter";
    mrca::ScatterParams q;
    CHECK(take_params(fn, params, mrca_scatter_default_params, &q));
    CHECK(check_ptr(fn, "boxes_dev", boxes_dev, 4, true));
    CHECK(check_ptr(fn, "poses_dev", poses_dev, 4, true));
    CHECK(check_ptr(fn, "goals_dev", goals_dev, 8, true));
    CHECK(check_ptr(fn, "tries_dev", tries_dev, 4, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (env->cfg.robots_per_world > mrca::kScatterMaxRobots)
        return fail(MRCA_ERR_UNSUPPORTED, "mrca_scatter: robots_per_world %d > %d (a world's placed points are held in 32 KB of LDS)",
                    env->cfg.robots_per_world, mrca::kScatterMaxRobots);
    // (valid before the first mrca_reset: the map, the geometry and the key stand since mrca_create)
    return launched(env->cfg.device, [&] {
        mrca::launch_scatter(env->view, q, boxes_dev, poses_dev, goals_dev, tries_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_hybrid_default_params(mrca_hybrid_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_hybrid_default_params: out is NULL");
    // (safe_scale, corridor, look): tuned on the closed-loop circles, profiles/hybrid/defaults.txt
    out->risk_dist = 0.6f;
    out->stop_dist = 0.3f;          // (the footprint's half diagonal is 0.2907 m)
    out->safe_scale = 0.75f;
    out->corridor = 1.0f;
    out->look = 6.0f;               // as far as the lidar sees
    out->front_cos = 0.5f;          // the front 120 degrees
    out->v_pid = 1.0f;
    out->k_omega = 6.0f;            // ORCA's
    out->max_speed = 1.0f;
    return MRCA_OK;
}

// mrca_hybrid_actions and mrca_hybrid_actions_goal (`fn` names the caller; goal_dev NULL: MRCA_F_LOCAL_GOAL)
static int hybrid_actions(const char* fn, mrca_env* env, const mrca_hybrid_params* params, const float* goal_dev, const uint8_t* mask_dev,
                          const float* policy_dev, float* actions_dev, int32_t* mode_dev, float* clear_dev, void* stream) {
    mrca::HybridParams q;
    CHECK(take_params(fn, params, mrca_hybrid_default_params, &q));
    CHECK(check_ptr(fn, "policy_dev", policy_dev, 4, true));
    CHECK(check_ptr(fn, "actions_dev", actions_dev, 8, true));
    CHECK(check_ptr(fn, "mode_dev", mode_dev, 4, false));
    CHECK(check_ptr(fn, "clear_dev", clear_dev, 4, false));
    CHECK(check_ptr(fn, "goal_dev", goal_dev, 8, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!env->reset_seen) return fail(MRCA_ERR_INVALID, "%s before the first mrca_reset: there is no scan yet", fn);
    return launched(env->cfg.device, [&] {
        mrca::launch_hybrid(env->view, q, goal_dev, mask_dev, policy_dev, actions_dev, mode_dev, clear_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_hybrid_actions(mrca_env* env, const mrca_hybrid_params* params, const uint8_t* mask_dev, const float* policy_dev,
                        float* actions_dev, int32_t* mode_dev, float* clear_dev, void* stream) {
    return hybrid_actions("mrca_hybrid_actions", env, params, nullptr, mask_dev, policy_dev, actions_dev, mode_dev, clear_dev, stream);
}

int mrca_hybrid_actions_goal(mrca_env* env, const mrca_hybrid_params* params, const uint8_t* mask_dev, const float* policy_dev,
                             float* actions_dev, int32_t* mode_dev, float* clear_dev, const float* goal_dev, void* stream) {
    return hybrid_actions("mrca_hybrid_actions_goal", env, params, goal_dev, mask_dev, policy_dev, actions_dev, mode_dev, clear_dev, stream);
}

int mrca_safe_policy_default_params(mrca_safe_policy_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_safe_policy_default_params: out is NULL");
    // tuned on the closed-loop circles, profiles/safe_policy/defaults.txt
    out->scan_scale = 0.3f;
    out->v_cap = 0.75f;
    return MRCA_OK;
}

// mrca_hybrid_plan and mrca_hybrid_plan_goal (`fn` names the caller; goal_dev NULL: MRCA_F_LOCAL_GOAL)
static int hybrid_plan(const char* fn, mrca_env* env, const mrca_hybrid_params* hybrid_params, const mrca_safe_policy_params* safe_params,
                       const float* goal_dev, const uint8_t* mask_dev, int32_t* mode_dev, float* scale_dev, float* pid_dev, float* clear_dev,
                       void* stream) {
    mrca::HybridParams q;
    mrca::SafeParams sq;
    CHECK(take_params(fn, hybrid_params, mrca_hybrid_default_params, &q));
    CHECK(take_params(fn, safe_params, mrca_safe_policy_default_params, &sq));
    CHECK(check_ptr(fn, "mode_dev", mode_dev, 4, true));
    CHECK(check_ptr(fn, "scale_dev", scale_dev, 4, true));
    CHECK(check_ptr(fn, "pid_dev", pid_dev, 8, true));
    CHECK(check_ptr(fn, "clear_dev", clear_dev, 4, false));
    CHECK(check_ptr(fn, "goal_dev", goal_dev, 8, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!env->reset_seen) return fail(MRCA_ERR_INVALID, "%s before the first mrca_reset: there is no scan yet", fn);
    return launched(env->cfg.device, [&] {
        mrca::launch_hybrid_plan(env->view, q, sq, goal_dev, mask_dev, mode_dev, scale_dev, pid_dev, clear_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_hybrid_plan(mrca_env* env, const mrca_hybrid_params* hybrid_params, const mrca_safe_policy_params* safe_params,
                     const uint8_t* mask_dev, int32_t* mode_dev, float* scale_dev, float* pid_dev, float* clear_dev, void* stream) {
    return hybrid_plan("mrca_hybrid_plan", env, hybrid_params, safe_params, nullptr, mask_dev, mode_dev, scale_dev, pid_dev, clear_dev, stream);
}

int mrca_hybrid_plan_goal(mrca_env* env, const mrca_hybrid_params* hybrid_params, const mrca_safe_policy_params* safe_params,
                          const uint8_t* mask_dev, int32_t* mode_dev, float* scale_dev, float* pid_dev, float* clear_dev,
                          const float* goal_dev, void* stream) {
    return hybrid_plan("mrca_hybrid_plan_goal", env, hybrid_params, safe_params, goal_dev, mask_dev, mode_dev, scale_dev, pid_dev, clear_dev,
                       stream);
}

int mrca_hybrid_commit(int32_t n_robots, const mrca_safe_policy_params* safe_params, const uint8_t* mask_dev, const int32_t* mode_dev,
                       const float* pid_dev, const float* policy_dev, float* actions_dev, void* stream) {
    const char* fn = "mrca_hybrid_commit";
    mrca::SafeParams sq;
    CHECK(take_params(fn, safe_params, mrca_safe_policy_default_params, &sq));
    if (n_robots < 1) return fail(MRCA_ERR_INVALID, "mrca_hybrid_commit: n_robots %d (needs >= 1)", n_robots);
    CHECK(check_ptr(fn, "mode_dev", mode_dev, 4, true));
    CHECK(check_ptr(fn, "pid_dev", pid_dev, 8, true));
    CHECK(check_ptr(fn, "policy_dev", policy_dev, 4, true));
    CHECK(check_ptr(fn, "actions_dev", actions_dev, 8, true));
    return launched(mrca::device_of(actions_dev), [&] {     // launch where the buffers live
        mrca::launch_hybrid_commit(n_robots, sq, mask_dev, mode_dev, pid_dev, policy_dev, actions_dev, static_cast<hipStream_t>(stream));
    });
}

int mrca_planner_default_params(mrca_planner_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_planner_default_params: out is NULL");
    out->stride = 2;        // 0.1 m planning cells on the shipped 0.05 m maps
    out->inflate = 7;       // 0.35 m: the footprint's half diagonal (0.29 m) and a cell of slack
    out->lookahead = 15;    // 1.5 m down the path
    out->max_rounds = 0;    // the bound of mrca_planner_device.h (plan_round_bound)
    return MRCA_OK;
}

int mrca_planner_grid(mrca_env* env, const mrca_planner_params* params, int32_t* pw_out, int32_t* ph_out) {
    mrca::PlannerParams q;
    CHECK(take_params("mrca_planner_grid", params, mrca_planner_default_params, &q));
    if (!pw_out || !ph_out) return fail(MRCA_ERR_INVALID, "mrca_planner_grid: pw_out / ph_out is NULL");
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    *pw_out = mrca::plan_cells(env->view.g.width, q.stride);
    *ph_out = mrca::plan_cells(env->view.g.height, q.stride);
    return MRCA_OK;
}

int mrca_goal_fields(mrca_env* env, const mrca_planner_params* params, const float* goals_dev, int32_t G, uint32_t* field_dev,
                     int32_t* rounds_out, void* stream) {
    const char* fn = "mrca_goal_fields";
    mrca::PlannerParams q;
    CHECK(take_params(fn, params, mrca_planner_default_params, &q));
    CHECK(check_int_range(fn, "G", G, 1, mrca::kPlanMaxGoals));
    CHECK(check_ptr(fn, "goals_dev", goals_dev, 4, true));
    CHECK(check_ptr(fn, "field_dev", field_dev, 4, true));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!env->reset_seen) return fail(MRCA_ERR_INVALID, "mrca_goal_fields before the first mrca_reset");
    mrca::DeviceGuard guard(env->cfg.device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (capturing(s))
        return fail(MRCA_ERR_INVALID, "mrca_goal_fields inside a stream capture: it synchronises the stream while it looks for convergence");
    constexpr int kEvery = 4;     // the counters are read every kEvery launches, each launch has its own
    if (!env->plan_counters) HIP_TRY(device_alloc(&env->plan_counters, kEvery * sizeof(uint32_t)));
    uint32_t* counters = env->plan_counters.get();
    const int pw = mrca::plan_cells(env->view.g.width, q.stride), ph = mrca::plan_cells(env->view.g.height, q.stride);
    const int64_t bound = q.max_rounds > 0 ? (int64_t)q.max_rounds : mrca::plan_round_bound(pw, ph);
    HIP_TRY(hipMemsetAsync(counters, 0, kEvery * sizeof(uint32_t), s));
    mrca::launch_goal_field_init(env->view, q, goals_dev, G, field_dev, s);
    HIP_TRY(hipGetLastError());
    int64_t quiet = -1;           // the first launch in which nothing fell
    for (int64_t base = 0; base < bound && quiet < 0; base += kEvery) {
        const int nb = (int)std::min<int64_t>(kEvery, bound - base);
        for (int r = 0; r < nb; ++r) mrca::launch_goal_field_round(env->view, q, G, field_dev, counters + r, s);
        HIP_TRY(hipGetLastError());
        uint32_t seen[kEvery] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(seen, counters, sizeof seen, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemsetAsync(counters, 0, sizeof seen, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int r = nb - 1; r >= 0; --r)
            if (seen[r] == 0) quiet = base + r;
    }
    mrca::launch_goal_field_finish(env->view, q, G, field_dev, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (rounds_out) *rounds_out = (int32_t)std::min<int64_t>(quiet >= 0 ? quiet : bound, INT32_MAX);
    if (quiet < 0)
        return fail(MRCA_ERR_UNSUPPORTED, "mrca_goal_fields: not converged within max_rounds = %lld launches (the field holds upper bounds)",
                    (long long)bound);
    return MRCA_OK;
}

// What mrca_subgoals and mrca_subgoals_los check alike after their params (`fn` names the caller)
static int subgoals_validate(const char* fn, const mrca_env* env, const uint32_t* field_dev, const float* goals_dev, int32_t G,
                             const int32_t* slot_dev, const float* local_dev, const float* subgoal_dev, const float* dist_dev,
                             const int32_t* status_dev, const int32_t* ahead_dev) {
    CHECK(check_int_range(fn, "G", G, 1, mrca::kPlanMaxGoals));
    CHECK(check_ptr(fn, "field_dev", field_dev, 4, true));
    CHECK(check_ptr(fn, "goals_dev", goals_dev, 4, true));
    CHECK(check_ptr(fn, "slot_dev", slot_dev, 4, false));
    CHECK(check_ptr(fn, "local_dev", local_dev, 8, true));
    CHECK(check_ptr(fn, "subgoal_dev", subgoal_dev, 4, false));
    CHECK(check_ptr(fn, "dist_dev", dist_dev, 4, false));
    CHECK(check_ptr(fn, "status_dev", status_dev, 4, false));
    CHECK(check_ptr(fn, "ahead_dev", ahead_dev, 4, false));
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!slot_dev && G != env->cfg.robots_per_world)
        return fail(MRCA_ERR_INVALID, "%s: slot_dev NULL (slot = n %% robots_per_world) needs G == robots_per_world (%d), got %d", fn,
                    env->cfg.robots_per_world, G);
    if (!env->reset_seen) return fail(MRCA_ERR_INVALID, "%s before the first mrca_reset: there is no head record yet", fn);
    return MRCA_OK;
}

int mrca_subgoals(mrca_env* env, const mrca_planner_params* params, const uint32_t* field_dev, const float* goals_dev, int32_t G,
                  const int32_t* slot_dev, const uint8_t* mask_dev, float* local_dev, float* subgoal_dev, float* dist_dev,
                  int32_t* status_dev, void* stream) {
    const char* fn = "mrca_subgoals";
    mrca::PlannerParams q;
    CHECK(take_params(fn, params, mrca_planner_default_params, &q));
    CHECK(subgoals_validate(fn, env, field_dev, goals_dev, G, slot_dev, local_dev, subgoal_dev, dist_dev, status_dev, nullptr));
    // (a measurement switch, tools/planner_probe.py: a robot per thread in place of eight lanes per robot -- the same outputs)
    static const int lanes = [] {
        const char* v = getenv("MRCA_SUBGOAL_LANES");
        return (v && v[0] == '1' && !v[1]) ? 1 : 8;
    }();
    return launched(env->cfg.device, [&] {
        mrca::launch_subgoals(env->view, q, field_dev, goals_dev, G, slot_dev, mask_dev, local_dev, subgoal_dev, dist_dev, status_dev, lanes,
                              static_cast<hipStream_t>(stream));
    });
}

int mrca_los_default_params(mrca_los_params* out) {
    if (!out) return fail(MRCA_ERR_INVALID, "mrca_los_default_params: out is NULL");
    out->reach = 60;        // 6 m on the default 0.1 m planning cells: the lidar's range
    return MRCA_OK;
}

int mrca_subgoals_los(mrca_env* env, const mrca_planner_params* params, const mrca_los_params* los_params, const uint32_t* field_dev,
                      const float* goals_dev, int32_t G, const int32_t* slot_dev, const uint8_t* mask_dev, float* local_dev,
                      float* subgoal_dev, float* dist_dev, int32_t* status_dev, int32_t* ahead_dev, void* stream) {
    const char* fn = "mrca_subgoals_los";
    mrca::PlannerParams q;
    mrca::LosParams lq;
    CHECK(take_params(fn, params, mrca_planner_default_params, &q));
    CHECK(take_params(fn, los_params, mrca_los_default_params, &lq));
    CHECK(subgoals_validate(fn, env, field_dev, goals_dev, G, slot_dev, local_dev, subgoal_dev, dist_dev, status_dev, ahead_dev));
    // A robot's group of lanes: a wavefront where every robot's is resident at once in that shape (256 CUs x 8 workgroups of four:
    // 8192 robots), eight lanes beyond -- what tools/planner_probe.py measured on either side.  The same outputs;
    // MRCA_SUBGOAL_LOS_LANES=8 / 64 forces a shape (read at every call: the probe and the tests run both in one process).
    const char* forced = getenv("MRCA_SUBGOAL_LOS_LANES");
    const bool f8 = forced && forced[0] == '8' && !forced[1], f64 = forced && forced[0] == '6' && forced[1] == '4' && !forced[2];
    const int lanes = f8 ? 8 : f64 ? 64 : (env->view.N <= mrca::kLosWaveRobots ? 64 : 8);
    return launched(env->cfg.device, [&] {
        mrca::launch_subgoals_los(env->view, q, lq, field_dev, goals_dev, G, slot_dev, mask_dev, local_dev, subgoal_dev, dist_dev, status_dev,
                                  ahead_dev, lanes, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
