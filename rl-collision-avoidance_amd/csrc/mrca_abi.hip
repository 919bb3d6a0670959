// mrca_abi.hip -- host side of include/mrca_env.h: config validation, the SoA device arena,
// table / map upload, kernel sequencing and optional HIP-event timing.  No torch, no Python.  What an env is made of is in
// mrca_env_state.h, where its memory lies in mrca_arena.h; the entry points of the renderer, the controllers, the noise model and the planner are in
// mrca_abi_controllers.hip.
#include <hip/hip_runtime.h>
#include <string>
#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mrca_env.h"
#include "mrca_arena.h"
#include "mrca_host.h"
#include "mrca_hostutil.h"
#include "mrca_kernels.h"
#include "mrca_pass_plan.h"
#include "mrca_rollout_store.h"
#include "mrca_env_state.h"      // (last: its `fail` is a macro)

using namespace mrca::env_state;

namespace {
thread_local char g_err[512] = "";
}

namespace mrca {
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace mrca

namespace {

using mrca::DeviceGuard;
using mrca::kAheadTicks;
namespace arena = mrca::arena;

int validate(const mrca_config* c) {
    if (!c) return fail(MRCA_ERR_INVALID, "config is NULL");
    if (c->abi_version != MRCA_ABI_VERSION)
        return fail(MRCA_ERR_INVALID, "abi_version %d != %d", c->abi_version, MRCA_ABI_VERSION);
    if (c->num_worlds < 1) return fail(MRCA_ERR_INVALID, "num_worlds must be >= 1");
    if (c->robots_per_world < 1) return fail(MRCA_ERR_INVALID, "robots_per_world must be >= 1");
    // more than 64 robots per world: the per-robot-thread path with a per-tick broad phase (bw_* kernels).  Its
    // episodes restart per robot or not at all; group-synchronous episodes (Stage-2) need the one-wave-per-world path
    if (c->robots_per_world > 64 && c->auto_reset == MRCA_AUTO_GROUP)
        return fail(MRCA_ERR_UNSUPPORTED, "robots_per_world %d > 64 with group-synchronous episodes (auto_reset 2)",
                    c->robots_per_world);
    if (!(c->collision_raster >= 0.0f)) return fail(MRCA_ERR_INVALID, "collision_raster must be >= 0");
    if (c->collision_raster > 0.0f && (c->collision_raster < 0.1f || mrca::outline_span(1.0f / c->collision_raster) > mrca::kOutlineWin))
        return fail(MRCA_ERR_UNSUPPORTED, "collision_raster %.3f m: an outline is kept as an 8 x 8 bitmap of raster cells, which "
                    "holds cells of >= 0.1 m", (double)c->collision_raster);
    if (c->collision_raster > 0.0f && c->robots_per_world > 64)
        return fail(MRCA_ERR_UNSUPPORTED, "collision_raster with robots_per_world > 64");
    if ((int64_t)c->num_worlds * c->robots_per_world > (1 << 24))
        return fail(MRCA_ERR_UNSUPPORTED, "more than 2^24 robots in one environment");
    if (c->beams < 64 || c->beams > 1024 || c->beams % 64)
        return fail(MRCA_ERR_INVALID, "beams %d must be a multiple of 64 in [64,1024]", c->beams);
    if (c->frames < 1 || c->frames > 8) return fail(MRCA_ERR_INVALID, "frames %d out of [1,8]", c->frames);
    if (c->map_width < 1 || c->map_height < 1 || c->map_words_per_row < (c->map_width + 31) / 32)
        return fail(MRCA_ERR_INVALID, "bad map geometry %dx%d wpr %d", c->map_width, c->map_height,
                    c->map_words_per_row);
    // the grid walks keep cell coordinates in fp32 (exact integers, sub-cell estimates good to << 1 cell up to
    // 2^16) and index the per-cell fields with 24-bit multiplies
    // (and the march addresses a field array with a 32-bit byte offset: the quadrant array of the largest map fits it; the octant
    // array, twice the size, is checked where it is built -- upload_octants)
    static_assert(mrca::field_fits_offsets(mrca::kMaxMapSide, mrca::kMaxMapSide, 4), "the quadrant array of the largest map");
    if (c->map_width > mrca::kMaxMapSide || c->map_height > mrca::kMaxMapSide)
        return fail(MRCA_ERR_UNSUPPORTED, "map %dx%d cells: at most %d per side", c->map_width, c->map_height, mrca::kMaxMapSide);
    if (!(c->map_cell > 0.0f)) return fail(MRCA_ERR_INVALID, "map_cell must be > 0");
    if (!c->map_bits) return fail(MRCA_ERR_INVALID, "map_bits is NULL");
    if (c->auto_reset < 0 || c->auto_reset > 2) return fail(MRCA_ERR_INVALID, "auto_reset %d", c->auto_reset);
    const int R = c->robots_per_world;
    for (int i = 0; i < R; ++i) {
        if (c->reset_mode && (c->reset_mode[i] < 0 || c->reset_mode[i] > 2))
            return fail(MRCA_ERR_INVALID, "reset_mode[%d] = %d", i, c->reset_mode[i]);
        if (c->goal_mode && (c->goal_mode[i] < 0 || c->goal_mode[i] > 2))
            return fail(MRCA_ERR_INVALID, "goal_mode[%d] = %d", i, c->goal_mode[i]);
        if (c->group_id && (c->group_id[i] < 0 || c->group_id[i] > 15))
            return fail(MRCA_ERR_INVALID, "group_id[%d] = %d out of [0,15]", i, c->group_id[i]);
        if (c->reset_mode && c->reset_mode[i] == MRCA_RESET_TABLE && !c->init_table)
            return fail(MRCA_ERR_INVALID, "reset_mode[%d] is TABLE but init_table is NULL", i);
        if (c->goal_mode && c->goal_mode[i] == MRCA_RESET_TABLE && !c->goal_table)
            return fail(MRCA_ERR_INVALID, "goal_mode[%d] is TABLE but goal_table is NULL", i);
    }
    return MRCA_OK;
}

constexpr int kTimingRing = 1024;

// The free-rectangle field depends on the map only and takes ~1 s of host time for an 800 x 800 map:
// environments created on the same map in one process (one per rank thread, per test, per bench leg)
// share one host copy.  Keyed by the bitmap itself.
struct HostField {
    std::vector<uint32_t> bits;
    int32_t width, height, wpr;
    std::vector<uint16_t> entries;      // 4 quadrant entries per cell
    std::vector<uint16_t> octants;      // 8 octant entries per cell (built when first asked for; same pitch)
    int pitch;
};
std::shared_ptr<const HostField> host_field(const mrca_config* c, bool octants) {
    static std::mutex mu;
    static std::vector<std::shared_ptr<HostField>> cache;
    const size_t words = (size_t)c->map_height * c->map_words_per_row;
    std::lock_guard<std::mutex> lock(mu);
    auto with_octants = [&](const std::shared_ptr<HostField>& f) {
        int pitch = 0;
        if (octants && f->octants.empty())
            mrca::build_octant_rect_field(f->bits.data(), f->width, f->height, f->wpr, &f->octants, &pitch);
        return f;
    };
    for (const auto& f : cache)
        if (f->width == c->map_width && f->height == c->map_height && f->wpr == c->map_words_per_row &&
            std::memcmp(f->bits.data(), c->map_bits, words * 4) == 0)
            return with_octants(f);
    auto f = std::make_shared<HostField>();
    f->bits.assign(c->map_bits, c->map_bits + words);
    f->width = c->map_width;
    f->height = c->map_height;
    f->wpr = c->map_words_per_row;
    mrca::build_free_rect_field(c->map_bits, c->map_width, c->map_height, c->map_words_per_row, &f->entries, &f->pitch);
    if (cache.size() >= 4) cache.erase(cache.begin());
    cache.push_back(f);
    return with_octants(f);
}

}  // namespace

constexpr size_t kAheadMaxBytes = 256u << 20;
// World range 1 gets its stream in mrca_create (chains <= 2, bench.py's default, may be captured at once); further ranges get
// theirs at their first use -- an env does not park streams it may never use (the runtime maps a process's streams onto a
// few hardware queues, DESIGN.md 5.10 "what the schedule depends on").
constexpr int kChainStreamsAtCreate = 1;

// the env's view with slot b's buffers in place of the five fields (b = 0: the env's own)
static mrca::EnvView slot_view(const mrca_env* env, int b) {
    mrca::EnvView v = env->view;
    const AheadRing& r = env->ahead;
    if (b > 0) arena::bind_slot(r.slot, r.mem.get() + (size_t)(b - 1) * r.slot.bytes, &v);
    return v;
}

// the ring heads' array: the env's field, or the scratch array a ray cast of several ticks alternates it with
static uint8_t* ring_heads(const mrca_env* env, int in_scratch) {
    return in_scratch ? env->ahead.head_scratch.get() : env->view.ring_head;
}

// the ray cast of `ticks` >= 2 ticks in one launch: its first tick reads slot b >= 1, the ticks behind it slots b - 1, b - 2 ...,
// and slot 0, the env's own fields, can only be the last one's (last_is_env); the ring heads go from head_in to head_out
static mrca::RayTicks slot_ticks(const mrca_env* env, int b, int ticks, bool last_is_env, const uint8_t* head_in, uint8_t* head_out) {
    const AheadRing& r = env->ahead;
    mrca::RayTicks t{};
    t.ticks = ticks;
    t.last_is_env = last_is_env;
    const size_t* off = r.slot.off;
    t.slot0 = r.mem.get() + (size_t)(b - 1) * r.slot.bytes + off[arena::kSlotPose];
    t.stride = -(int32_t)r.slot.bytes;
    t.off_head = (uint32_t)(off[arena::kSlotHead] - off[arena::kSlotPose]);
    t.in.off_goal = (uint32_t)(off[arena::kSlotGoal] - off[arena::kSlotPose]);
    t.in.off_fresh = (uint32_t)(off[arena::kSlotFresh] - off[arena::kSlotPose]);
    t.in.off_outline = (uint32_t)(off[arena::kSlotOutline] - off[arena::kSlotPose]);
    t.in.head_in = head_in;
    t.in.head_out = head_out;
    return t;
}

// `v` for a part of the env: the robots whose lidar outputs (scan, frame stack, local goal) a ray cast produces and the worlds a
// move launch advances
static mrca::EnvView range_view(mrca::EnvView v, int32_t first, int32_t count, int32_t world_first, int32_t world_count) {
    v.ray_first = first;
    v.ray_count = count;
    v.world_first = world_first;
    v.world_count = world_count;
    return v;
}
// `v` for a ray cast (lazy_obs = 0: it forms MRCA_F_SCAN / MRCA_F_OBS of its robots itself -- no materialize launch behind it)
static mrca::EnvView observing(const mrca_env* env, mrca::EnvView v) {
    v.eager_views = env->cfg.lazy_obs ? 0 : (MRCA_VIEW_SCAN | MRCA_VIEW_OBS);
    return v;
}

// world range c of mrca_step_many's P: its stream (range 0: the caller's) and its first world
static inline hipStream_t range_stream(const mrca_env* env, hipStream_t s0, int c) { return c ? env->ranges[c - 1].stream.get() : s0; }
static inline int range_first_world(int W, int P, int c) { return (int)((int64_t)c * W / P); }

// the stream and both events of the next world range: appended only when all three exist
static hipError_t add_world_range(mrca_env* env) {
    WorldRange r;
    hipError_t e = make_stream(&r.stream);
    if (e == hipSuccess) e = make_event(&r.moved);
    if (e == hipSuccess) e = make_event(&r.done);
    if (e == hipSuccess) env->ranges.push_back(std::move(r));
    return e;
}

// join: the caller's stream continues when world ranges 1 .. upto - 1 are through, all of them whatever fails (a forked stream
// left unjoined would dangle from a capture, and its launches would race the caller's next call) -> the first error
static hipError_t join_ranges(const mrca_env* env, hipStream_t s0, int upto) {
    hipError_t err = hipSuccess;
    for (int c = 1; c < upto; ++c) {
        const WorldRange& r = env->ranges[c - 1];
        const hipError_t e1 = hipEventRecord(r.done.get(), r.stream.get());
        const hipError_t e2 = hipStreamWaitEvent(s0, r.done.get(), 0);
        if (err == hipSuccess) err = e1 != hipSuccess ? e1 : e2;
    }
    return err;
}

// env->view -> its device copy (mrca_create; the profiling build's debug switches).  Synchronous: no launch that reads the
// copy is in flight at either place.
static hipError_t upload_view(mrca_env* env) {
    hipError_t e = env->view_dev ? hipSuccess : device_alloc(&env->view_dev, sizeof(mrca::EnvView));
    if (e != hipSuccess) return e;
    env->view.dev = env->view_dev.get();
    if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
    return hipMemcpy(env->view_dev.get(), &env->view, sizeof(mrca::EnvView), hipMemcpyHostToDevice);
}

// the caller's arena, or one of the library's own
static int attach_arena(mrca_env* env, void* arena_dev, size_t arena_bytes) {
    const size_t total = env->layout.total;
    if (arena_dev) {
        if (arena_bytes < total) return fail(MRCA_ERR_NOMEM, "arena of %zu bytes < required %zu", arena_bytes, total);
        if (reinterpret_cast<uintptr_t>(arena_dev) % arena::kAlign) return fail(MRCA_ERR_INVALID, "arena must be %zu-byte aligned", arena::kAlign);
        env->arena = static_cast<char*>(arena_dev);
        return MRCA_OK;
    }
    const hipError_t e = device_alloc(&env->own_arena, total);
    if (e != hipSuccess) return fail(MRCA_ERR_NOMEM, "hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
    env->arena = env->own_arena.get();
    return MRCA_OK;
}

// a host array into the part of the arena that a view's pointer is bound to (the tables' pointers are const: kernels only read them)
template <class T, class U> static hipError_t to_arena(const T* part, const std::vector<U>& src) {
    return hipMemcpy(const_cast<T*>(part), src.data(), src.size() * sizeof(U), hipMemcpyHostToDevice);
}

// the arena's contents at construction (tables, poses, beams, map), written through the pointers of the env's view -> the
// view's free-rectangle pitch and robot groups
static int upload_tables(const mrca_config* cfg, mrca_env* env) {
    mrca::EnvView& v = env->view;
    HIP_TRY(hipMemset(env->arena, 0, env->layout.total));
    const int R = cfg->robots_per_world, B = cfg->beams;
    const size_t N = (size_t)cfg->num_worlds * R;
    // scenario tables
    std::vector<int32_t> reset_mode(R, MRCA_RESET_DISC), goal_mode(R, MRCA_RESET_DISC), group(R, 0);
    std::vector<float> init_tab(R * 3, 0.0f), goal_tab(R * 2, 0.0f);
    if (cfg->reset_mode) memcpy(reset_mode.data(), cfg->reset_mode, R * 4);
    if (cfg->goal_mode) memcpy(goal_mode.data(), cfg->goal_mode, R * 4);
    else if (cfg->reset_mode) goal_mode = reset_mode;
    if (cfg->group_id) memcpy(group.data(), cfg->group_id, R * 4);
    if (cfg->init_table) memcpy(init_tab.data(), cfg->init_table, R * 3 * 4);
    if (cfg->goal_table) memcpy(goal_tab.data(), cfg->goal_table, R * 2 * 4);
    int num_groups = 0;
    for (int i = 0; i < R; ++i) num_groups = group[i] + 1 > num_groups ? group[i] + 1 : num_groups;
    v.num_groups = num_groups;
    // beam directions: bearing_i = -pi/2 + i*pi/(B-1) (stageros.cpp:495-497), evaluated in
    // double, rounded once to fp32
    std::vector<float> bcos(B), bsin(B);
    for (int i = 0; i < B; ++i) {
        const double b = -M_PI / 2.0 + (double)i * (M_PI / (double)(B - 1));
        bcos[i] = (float)std::cos(b);
        bsin[i] = (float)std::sin(b);
    }
    HIP_TRY(to_arena(v.reset_mode, reset_mode));
    HIP_TRY(to_arena(v.goal_mode, goal_mode));
    HIP_TRY(to_arena(v.group_id, group));
    HIP_TRY(to_arena(v.init_table, init_tab));
    HIP_TRY(to_arena(v.goal_table, goal_tab));
    {
        // before the first reset the robots stand at their table poses (= the agent lines of the world file): a start
        // sampled in Stage-2's region keeps 7 m away from the robot's CURRENT position, its first one included
        // (stage_world2.py:250-268)
        std::vector<float> pose0((size_t)N * 3);
        for (size_t n = 0; n < N; ++n)
            for (int k = 0; k < 3; ++k) pose0[n * 3 + k] = init_tab[(n % (size_t)R) * 3 + k];
        HIP_TRY(to_arena(v.pose, pose0));
    }
    HIP_TRY(to_arena(v.beam_cos, bcos));
    HIP_TRY(to_arena(v.beam_sin, bsin));
    HIP_TRY(hipMemcpy(const_cast<uint32_t*>(v.map_bits), cfg->map_bits, arena::part_bytes(*cfg, &mrca::EnvView::map_bits), hipMemcpyHostToDevice));
    const std::shared_ptr<const HostField> hf = host_field(cfg, false);
    v.free_rect_pitch = hf->pitch;
    HIP_TRY(to_arena(v.free_rect, hf->entries));
    std::vector<uint8_t> cf;
    mrca::build_cell_field(cfg->map_bits, cfg->map_width, cfg->map_height, cfg->map_words_per_row, &cf);
    HIP_TRY(to_arena(v.cellfield, cf));
    if (v.big)     // the collision hash starts empty; every tick leaves it empty again (bw_finish_kernel)
        HIP_TRY(hipMemset(v.bw_chead, 0xFF, arena::part_bytes(*cfg, &mrca::EnvView::bw_chead)));
    // live = 1, t = 1 at construction (a robot exists and is idle before the first reset)
    HIP_TRY(hipMemset(v.live, 1, N));
    HIP_TRY(to_arena(v.t, std::vector<int32_t>(N, 1)));
    return MRCA_OK;
}

// Does the march read the OCTANT free-rectangle array (mrca_host.h: build_octant_rect_field) after a ray's first jump?  It
// takes fewer trips per wavefront there (Stage-1: 2.88 -> 2.66 per 64 beams, profiles/octant_field/field_probe.txt) from
// records twice the size: a cache line holds 8 cells instead of 16.  The rule has two sides:
//   * on where the array fits one XCD's 4 MiB L2 -- the 20 m Stage-1 rink (404 x 402 records of 16 bytes: 2.6 MB) does;
//     Stage-2's 800 x 800 map (10.3 MB; its quadrant array, 5.1 MB, already does not) does not, and its trips would fall by
//     1.2 % only (1.543 -> 1.525);
//   * and only with lazy_obs = 1: the eager epilogue streams 60 MB of frame stacks through that L2 per tick of 4096 robots,
//     the field does not stay resident, and the sparser records lose more to the misses than the trips save.
// Measured on an MI355X, the two settings alternated on one box, five pairs, M agent-steps/s at the medians
// (profiles/octant_field/ab.txt): 4096 Stage-1 robots, lazy_obs = 1, 1000 ticks 257.2 (quadrant array, the parent's library)
// -> 267.3; the same with lazy_obs = 0: 178.1 (MRCA_FIELD_OCTANTS=0) -> 174.5 (=1).
// MRCA_FIELD_OCTANTS=0|1, read once per mrca_create, overrides the rule for A/B runs on one box: 0 is the march over the
// quadrant array for every lookup -- the same code, FreeRectField's uniforms 3 and 0.
static bool field_octants(const mrca_config* c) {
    if (const char* v = std::getenv("MRCA_FIELD_OCTANTS")) return std::atoi(v) != 0;
    const size_t bytes = (size_t)(c->map_width + 2 * mrca::kFieldPadX) * (c->map_height + 2 * mrca::kFieldPadY) * 8 * sizeof(uint16_t);
    return c->lazy_obs != 0 && bytes <= ((size_t)4 << 20);
}

// the octant array into a buffer of the env's own, and the march's three uniforms of the view onto it
static int upload_octants(const mrca_config* cfg, mrca_env* env) {
    if (!mrca::field_fits_offsets(cfg->map_width, cfg->map_height, 8))
        return fail(MRCA_ERR_UNSUPPORTED, "map %dx%d cells: the octant free-rectangle array passes 4 GiB (MRCA_FIELD_OCTANTS=0 "
                    "marches over the quadrant array)", cfg->map_width, cfg->map_height);
    const std::shared_ptr<const HostField> hf = host_field(cfg, true);
    const size_t bytes = hf->octants.size() * sizeof(uint16_t);
    HIP_TRY(device_alloc(&env->octant_rect, bytes));
    HIP_TRY(hipMemcpy(env->octant_rect.get(), hf->octants.data(), bytes, hipMemcpyHostToDevice));
    env->view.march_rect = env->octant_rect.get();
    env->view.march_shift = 4;
    env->view.march_major = 8;
    return MRCA_OK;
}

// the view of the arena `a` and of the config that every launch takes (the free-rectangle field's pitch and the robot groups:
// upload_tables)
static mrca::EnvView make_view(const mrca_config* cfg, char* a) {
    const int R = cfg->robots_per_world, B = cfg->beams;
    const size_t N = (size_t)cfg->num_worlds * R;
    mrca::EnvView v = mrca::EnvView();
    v.N = (int32_t)N;
    v.R = R;
    v.W = cfg->num_worlds;
    v.B = B;
    v.F = cfg->frames;
    arena::bind(*cfg, a, &v);
    v.beam_step = mrca::kPi / (float)(B - 1);
    v.beam_inv_step = (float)(B - 1) / mrca::kPi;
    v.march_rect = v.free_rect;      // (mrca_create: upload_octants points the march at the octant array where it is on)
    v.march_shift = 3;
    v.march_major = 0;
    v.big = R > 64 ? 1 : 0;
    v.ray_first = 0;
    v.ray_count = (int32_t)N;
    v.world_first = 0;
    v.world_count = cfg->num_worlds;
    v.g.x0 = cfg->map_x0;
    v.g.y0 = cfg->map_y0;
    v.g.cell = cfg->map_cell;
    v.g.inv_cell = 1.0f / cfg->map_cell;
    v.g.width = cfg->map_width;
    v.g.height = cfg->map_height;
    v.g.wpr = cfg->map_words_per_row;
    v.timeout = cfg->timeout;
    v.w_thresh = cfg->w_thresh;
    v.pre_dist_zero = cfg->pre_dist_zero;
    v.hold_velocity = cfg->hold_velocity ? 1 : 0;
    v.auto_reset = cfg->auto_reset;
    v.key0 = (uint32_t)(cfg->seed & 0xFFFFFFFFull);
    v.key1 = (uint32_t)(cfg->seed >> 32);
    v.foot_hc = (int32_t)std::ceil(0.2907 * (double)v.g.inv_cell) + 1;
    v.edge_slots = mrca::edge_event_slots(v.g.inv_cell);
    v.raster_inv = cfg->collision_raster > 0.0f ? 1.0f / cfg->collision_raster : 0.0f;
    v.raster_res = cfg->collision_raster;
    v.raster_kw = mrca::raster_window(v.raster_inv);
    v.lidar_radius = 0.2917f;
    v.lidar_near = 0.30f;
    v.lidar_reach2 = mrca::kLidarReach2;
    if (cfg->collision_raster > 0.0f) {      // outline CELLS reach one cell diagonal beyond the rectangle
        v.lidar_radius = 0.2917f + 1.4143f * cfg->collision_raster;
        v.lidar_near = v.lidar_radius + 0.01f;
        const float reach = 6.0f + v.lidar_radius + 0.01f;
        v.lidar_reach2 = reach * reach;
    }
    {   // broad phase: rectangles further apart than 2 x circumradius cannot overlap; outlines further apart than that
        // plus one raster-cell diagonal cannot share a cell
        const float reach = 2.0f * 0.2907f + 0.001f + (cfg->collision_raster > 0.0f ? 1.4143f * cfg->collision_raster : 0.0f);
        v.collide_reach2 = cfg->collision_raster > 0.0f ? reach * reach : mrca::kCollideReach2;
    }
    v.r_magic = R <= 64 ? (uint32_t)(((1ull << 32) + (uint64_t)R - 1) / (uint64_t)R) : 0u;
    v.debug_flags = 0;
    v.dev = nullptr;                      // (upload_view, at the end of mrca_create)
    v.eager_views = 0;                    // (set per launch by the step paths of an env with lazy_obs = 0)
#if defined(MRCA_PROFILING)
    v.launch_stamps = nullptr;
    v.launch_slot = 0;
#endif
    // the ray cast's launch shape: the product's (mrca_ray_shape.h, with the measurements behind it)
    v.ray_shift = mrca::product_ray_shift(cfg->beams, v.big);
    v.ray_prep_wave = 0;
    v.ray_sequential = 1;
    return v;
}

// what the move launch and the ray cast need of a CU's LDS
static int check_lds(mrca_env* env) {
    const mrca::EnvView& v = env->view;
    env->lds_bytes = mrca::ray_shape(v).lds_bytes;
    if (!v.big && mrca::move_lds_bytes(v) > 64 * 1024)
        return fail(MRCA_ERR_UNSUPPORTED, "map_cell %.4f m is too fine for the LDS patches: use >= 0.01 m", (double)env->cfg.map_cell);
    if (env->lds_bytes > 160 * 1024)
        return fail(MRCA_ERR_UNSUPPORTED, "the ray cast needs %zu B of LDS per robot (> 160 KiB): too many beams", env->lds_bytes);
    return MRCA_OK;
}

// mrca_step_many's ring (outside the arena: a caller-provided arena keeps its documented size), move stream and first ranges.  As
// many slots as fit the budget, at most one per tick of a pass; none (something could not be made) = the chained schedule, no error
static void init_step_many(mrca_env* env) {
    AheadRing& r = env->ahead;
    const size_t N = (size_t)env->view.N;
    r.slot = arena::make_slot(env->cfg);
    size_t slots = kAheadMaxBytes / r.slot.bytes;
    if (slots > (size_t)kAheadTicks - 1) slots = kAheadTicks - 1;
    if (slots >= 1 && device_alloc(&r.mem, slots * r.slot.bytes) == hipSuccess) r.slots = (int)slots;
    else (void)hipGetLastError();
    bool ok = make_stream(&r.move_stream) == hipSuccess;
    r.moved.resize(kAheadTicks);
    for (Event& e : r.moved) ok = ok && make_event(&e) == hipSuccess;
    for (int c = 0; c < kChainStreamsAtCreate && ok; ++c) ok = add_world_range(env) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        r.slots = 0;
    }
    // ticks per ray-cast launch: as many as the scan ring has frames (every tick of a launch that is not a restart writes a
    // slot of its own: each tick's row is stored), at most the 8 the kernel's tick index has flags for -- where that was
    // measured to pay (mrca::ticks_per_launch).  MRCA_TICKS_PER_LAUNCH, read once here, sets the number for every pass whatever its
    // shape, for A/B runs on one box: 1 is a launch per tick, the schedule before there were such launches
    int ticks = env->view.F < 8 ? env->view.F : 8;
    if (const char* v = std::getenv("MRCA_TICKS_PER_LAUNCH")) {
        const int want = std::atoi(v);
        if (want >= 1) {
            if (want < ticks) ticks = want;
            r.ticks_forced = true;
        }
    }
    // (such a launch addresses the fresh flags of its ticks -- up to 8 slots apart -- from one base with a 32-bit offset:
    // beyond that, a launch per tick)
    if (7ull * r.slot.bytes + (unsigned long long)r.slot.part_bytes[arena::kSlotFresh] > 0xffffffffull) ticks = 1;
    if (ticks > 1 && r.slots > 0 && device_alloc(&r.head_scratch, N) == hipSuccess) r.ticks_per_launch = ticks;
    else (void)hipGetLastError();
}

extern "C" {

int mrca_abi_version(void) { return MRCA_ABI_VERSION; }

const char* mrca_last_error(void) { return g_err; }

int mrca_arena_bytes(const mrca_config* cfg, size_t* bytes_out) {
    if (int rc = validate(cfg)) return rc;
    if (!bytes_out) return fail(MRCA_ERR_INVALID, "bytes_out is NULL");
    *bytes_out = arena::make_layout(*cfg).total;
    return MRCA_OK;
}

int mrca_create(const mrca_config* cfg, void* arena_dev, size_t arena_bytes, mrca_env** env_out) {
    if (int rc = validate(cfg)) return rc;
    if (!env_out) return fail(MRCA_ERR_INVALID, "env_out is NULL");
    *env_out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(MRCA_ERR_INVALID, "device %d not in [0,%d)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));

    std::unique_ptr<mrca_env> env(new (std::nothrow) mrca_env());   // (an early return frees what it holds by then)
    if (!env) return fail(MRCA_ERR_NOMEM, "host allocation failed");
    env->cfg = *cfg;
    env->layout = arena::make_layout(*cfg);
    if (int rc = attach_arena(env.get(), arena_dev, arena_bytes)) return rc;
    env->view = make_view(cfg, env->arena);
    if (int rc = upload_tables(cfg, env.get())) return rc;
    const bool octants = field_octants(cfg);
    env->cfg.map_bits = nullptr;  // host pointers are not retained
    env->cfg.reset_mode = env->cfg.goal_mode = env->cfg.group_id = nullptr;
    env->cfg.init_table = env->cfg.goal_table = nullptr;
    if (octants)
        if (int rc = upload_octants(cfg, env.get())) return rc;
    if (int rc = check_lds(env.get())) return rc;
    if (!env->view.big) init_step_many(env.get());
    HIP_TRY(upload_view(env.get()));       // (the view is final from here on)
    mrca::launch_head_init(env->view, nullptr);   // head records of the construction-time poses (all at the origin)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    *env_out = env.release();
    return MRCA_OK;
}

int mrca_destroy(mrca_env* env) {
    if (!env) return MRCA_OK;
    char* arena = env->own_arena.release();   // (freed last: the one failure reported)
    delete env;
    if (arena) HIP_TRY(hipFree(arena));
    return MRCA_OK;
}

int mrca_get_field(mrca_env* env, int field, void** ptr_dev_out, size_t* offset_out, size_t* bytes_out) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (field < 0 || field >= MRCA_F_COUNT) return fail(MRCA_ERR_INVALID, "field %d out of range", field);
    if (ptr_dev_out) *ptr_dev_out = env->arena + env->layout.field_off[field];
    if (offset_out) *offset_out = env->layout.field_off[field];
    if (bytes_out) *bytes_out = env->layout.field_bytes[field];
    return MRCA_OK;
}

int mrca_reset(mrca_env* env, const uint8_t* mask_dev, const float* poses_dev, const float* goals_dev, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    DeviceGuard guard(env->cfg.device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrca::launch_reset(env->view, mask_dev, poses_dev, goals_dev, s);
    if (env->view.big && env->lidar_counts_pending) {     // (a move phase whose observe phase never came: its counts are void)
        HIP_TRY(hipMemsetAsync(env->view.bw_lcount, 0, ((size_t)env->view.bw_lmask + 1) * sizeof(int32_t), s));
        env->lidar_counts_pending = false;
    }
    mrca::launch_lidar_grid(env->view, /*counted=*/0, s);
    env->lidar_hash_current = true;
    env->reset_seen = true;
    mrca::launch_raycast(env->view, /*only_fresh=*/1, s);
    if (!env->cfg.lazy_obs) mrca::launch_materialize(env->view, MRCA_VIEW_SCAN | MRCA_VIEW_OBS, s);
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_materialize(mrca_env* env, int32_t what, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (what & ~(MRCA_VIEW_SCAN | MRCA_VIEW_OBS)) return fail(MRCA_ERR_INVALID, "mrca_materialize: unknown view bits 0x%x", what);
    DeviceGuard guard(env->cfg.device);
    mrca::launch_materialize(env->view, what, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_newest_obs(mrca_env* env, float* out_dev, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!out_dev) return fail(MRCA_ERR_INVALID, "out_dev is NULL");
    if (reinterpret_cast<uintptr_t>(out_dev) % 16) return fail(MRCA_ERR_INVALID, "out_dev must be 16-byte aligned");
    DeviceGuard guard(env->cfg.device);
    mrca::launch_newest_obs(env->view, out_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

enum { kPhaseMove = 1, kPhaseObserve = 2 };
static int step_impl(mrca_env* env, const float* actions_dev, int32_t first, int32_t count, void* stream,
                     int32_t world_first = 0, int32_t world_count = -1, int phases = kPhaseMove | kPhaseObserve) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if ((phases & kPhaseMove) && !actions_dev) return fail(MRCA_ERR_INVALID, "actions_dev is NULL");
    if ((phases & kPhaseMove) && env->view.big && env->lidar_counts_pending)
        return fail(MRCA_ERR_INVALID, "mrca_move_worlds twice without mrca_observe_worlds in between (robots_per_world > 64: the "
                                      "observe phase consumes what the move phase counted)");
    if (first < 0 || count < 0 || first + count > env->view.N)
        return fail(MRCA_ERR_INVALID, "ray-cast slice [%d, %d) outside [0, %d)", first, first + count, env->view.N);
    if (world_count < 0) world_count = env->view.W;
    DeviceGuard guard(env->cfg.device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool rec = phases == (kPhaseMove | kPhaseObserve) && env->timing > 0 && (env->step_count++ % env->timing) == 0 &&
                     env->ev_used + 4 <= (int)env->ev.size();
    // (the worlds: mrca_step_worlds' range, otherwise all of them)
    const mrca::EnvView v = range_view(env->view, first, count, world_first, world_count);
    env->last_ray_count = count;
    // timing: the launches' own begin / end stamps (hipExtLaunchKernel), not event records around them
    const Event* ev = rec ? &env->ev[env->ev_used] : nullptr;
    if (phases & kPhaseMove) {
        mrca::launch_move(v, actions_dev, s, rec ? ev[0].get() : nullptr, rec ? ev[1].get() : nullptr);
        env->lidar_hash_current = false;           // (big worlds: the poses have moved on, bw_finish_kernel has counted them)
        env->lidar_counts_pending = env->view.big;
    }
    if (phases & kPhaseObserve) {
        // (an observe phase on its own with no move phase before it counts the robots itself)
        mrca::launch_lidar_grid(v, /*counted=*/env->view.big && !env->lidar_counts_pending ? 0 : 1, s);
        env->lidar_hash_current = true;
        env->lidar_counts_pending = false;
        mrca::launch_raycast(observing(env, v), /*only_fresh=*/0, s, rec ? ev[2].get() : nullptr, rec ? ev[3].get() : nullptr);
    }
    if (rec) env->ev_used += 4;
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_step(mrca_env* env, const float* actions_dev, void* stream) {
    return step_impl(env, actions_dev, 0, env ? env->view.N : 0, stream);
}

int mrca_step_slice(mrca_env* env, const float* actions_dev, int32_t first_robot, int32_t num_robots, void* stream) {
    return step_impl(env, actions_dev, first_robot, num_robots, stream);
}

static int worlds_impl(mrca_env* env, const float* actions_dev, int32_t first_world, int32_t num_worlds, void* stream, int phases) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (first_world < 0 || num_worlds < 0 || first_world + num_worlds > env->view.W)
        return fail(MRCA_ERR_INVALID, "world range [%d, %d) outside [0, %d)", first_world, first_world + num_worlds, env->view.W);
    // (the two phases one by one are the same launches as the whole tick, for ALL worlds: mrca_orca_actions_any's contract
    // about the lidar hash is stated and tested between them)
    if (env->view.big && (first_world != 0 || num_worlds != env->view.W))
        return fail(MRCA_ERR_UNSUPPORTED, "a part of the worlds with robots_per_world > 64");
    const int32_t R = env->view.R;
    return step_impl(env, actions_dev, first_world * R, num_worlds * R, stream, first_world, num_worlds, phases);
}

int mrca_step_worlds(mrca_env* env, const float* actions_dev, int32_t first_world, int32_t num_worlds, void* stream) {
    return worlds_impl(env, actions_dev, first_world, num_worlds, stream, kPhaseMove | kPhaseObserve);
}

int mrca_move_worlds(mrca_env* env, const float* actions_dev, int32_t first_world, int32_t num_worlds, void* stream) {
    return worlds_impl(env, actions_dev, first_world, num_worlds, stream, kPhaseMove);
}

int mrca_observe_worlds(mrca_env* env, int32_t first_world, int32_t num_worlds, void* stream) {
    return worlds_impl(env, nullptr, first_world, num_worlds, stream, kPhaseObserve);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Which streams?  The HIP runtime maps a process's streams onto a few hardware queues (four by default, handed out by use
// count), and two streams that share a queue run their kernels ONE AFTER THE OTHER whatever the program says: the schedules
// below then lose what they are built for, silently (tools/queue_alias_probe.hip: of twelve streams every one shares its queue
// with two others; tools/stream_pressure_probe.py: the same mrca_step_many call at 305 M and at 150 M agent-steps/s on the
// Stage-2 map depending on what else the process had created -- round 5's chained schedule halves in the same states).
// Which streams share is the runtime's business, so the env MEASURES it: two 40 us probe kernels, one on each stream of a
// pair (both warmed first: a stream's first launch creates its queue), stamped with the constant clock; if the second started
// only after the first had ended, the pair shares a queue: the env parks that stream (a parked stream keeps its use count on
// its queue, so the next candidate lands elsewhere) and tries another.  At the first mrca_step_many call on a given caller's
// stream (again if more ranges are asked for on it, or a check had to replace one of the env's streams), never inside a capture:
// ~1 ms, and the one place where a call of this library synchronises.
__global__ void stream_probe_kernel(unsigned long long ticks, unsigned long long* stamps, int slot) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(4);
    if (threadIdx.x == 0 && stamps) {
        stamps[slot * 2 + 0] = t0;
        stamps[slot * 2 + 1] = wall_clock64();
    }
}

// 1: the two streams ran the probes side by side; 0: one after the other; -1: a HIP call failed
static int streams_overlap(mrca_env* env, hipStream_t a, hipStream_t b) {
    int serial = 0;
    for (int rep = 0; rep < 3; ++rep) {
        hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, a, 4000ull, env->check.stamps.get(), 0);      // 40 us
        hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, b, 4000ull, env->check.stamps.get(), 1);
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
        unsigned long long h[4];
        if (hipMemcpy(h, env->check.stamps.get(), sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (h[2] >= h[1] || h[0] >= h[3]) ++serial;
    }
    return serial >= 2 ? 0 : 1;
}

static int warm_stream(hipStream_t st) {
    hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, st, 0ull, (unsigned long long*)nullptr, 0);
    HIP_TRY(hipStreamSynchronize(st));
    return MRCA_OK;
}

// make `*slot` a stream that overlaps with every stream of `chosen` and add it there; the ones that do not are parked
static int choose_stream(mrca_env* env, Stream* slot, std::vector<hipStream_t>* chosen) {
    for (int attempt = 0; attempt < 6; ++attempt) {
        if (!*slot) HIP_TRY(make_stream(slot));
        if (int rc = warm_stream(slot->get())) return rc;
        bool good = true;
        for (hipStream_t o : *chosen) {
            const int ov = streams_overlap(env, o, slot->get());
            if (ov < 0) return fail(MRCA_ERR_HIP, "mrca_step_many: stream probe failed: %s", hipGetErrorString(hipGetLastError()));
            if (ov == 0) {
                good = false;
                break;
            }
        }
        if (good) break;
        env->check.parked.push_back(std::move(*slot));
    }
    // (six candidates in a row shared a queue with somebody: take one more as it comes -- correct, only not concurrent)
    if (!*slot) HIP_TRY(make_stream(slot));
    chosen->push_back(slot->get());
    return MRCA_OK;
}

static int choose_streams(mrca_env* env, hipStream_t s0, int P) {
    StreamCheck& chk = env->check;
    if (!chk.stamps) HIP_TRY(device_alloc(&chk.stamps, 4 * sizeof(unsigned long long)));
    const size_t parked_before = chk.parked.size();
    if (int rc = warm_stream(s0)) return rc;
    std::vector<hipStream_t> chosen{s0};
    if (env->ahead.slots > 0)
        if (int rc = choose_stream(env, &env->ahead.move_stream, &chosen)) return rc;
    for (int c = 1; c < P; ++c)
        if (int rc = choose_stream(env, &env->ranges[c - 1].stream, &chosen)) return rc;
    // (a caller that alternates between a few streams is checked once per stream, not once per call -- unless a check had to
    // replace one of the env's streams: then what was verified before no longer holds)
    std::vector<StreamCheck::Record>& rec = chk.checked;
    if (chk.parked.size() != parked_before) rec.clear();
    rec.erase(std::remove_if(rec.begin(), rec.end(), [s0](const StreamCheck::Record& r) { return r.caller == s0; }), rec.end());
    if (rec.size() >= 8) rec.erase(rec.begin());
    rec.push_back({s0, P});
    if (std::getenv("MRCA_DEBUG_STREAMS"))
        std::fprintf(stderr, "[mrca] stream check against %p: %d range stream(s) + move stream chosen, %zu candidate(s) parked\n",
                     (void*)s0, P - 1, chk.parked.size());
    return MRCA_OK;
}

#if defined(MRCA_PROFILING)
// Profiling build, MRCA_LAUNCH_STAMPS=1: the timeline of every run-ahead pass without a profiler attached (rocprofv3's tracing
// triples the host's cost per launch, and a short region is host-paced) -- every launch of the pass stamps its first start and
// last end on the device's constant clock (MRCA_LAUNCH_BEGIN / _END), the host notes when it enqueued it; printed to stderr
// after a device synchronisation at the end of the pass.  tools/region_once.py, DESIGN.md 5.10.
struct LaunchLog {
    unsigned long long* dev = nullptr;
    std::vector<std::string> what;
    std::vector<double> host_at;
    double host_t0 = 0.0;
    bool on = false;
};
static LaunchLog g_log;
constexpr int kLogSlots = 2048;
static double host_now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void log_begin() {
    g_log.on = getenv("MRCA_LAUNCH_STAMPS") != nullptr;
    if (!g_log.on) return;
    if (!g_log.dev && hipMalloc(reinterpret_cast<void**>(&g_log.dev), kLogSlots * 16) != hipSuccess) {
        g_log.on = false;
        return;
    }
    std::vector<unsigned long long> init((size_t)kLogSlots * 2);
    for (int i = 0; i < kLogSlots; ++i) {
        init[2 * i] = ~0ull;
        init[2 * i + 1] = 0ull;
    }
    (void)hipMemcpy(g_log.dev, init.data(), init.size() * 8, hipMemcpyHostToDevice);
    g_log.what.clear();
    g_log.host_at.clear();
    g_log.host_t0 = host_now_us();
}
static void log_note(const char* kind, int tick, int range) {      // a host-side call that is not a launch
    if (!g_log.on) return;
    char buf[64];
    snprintf(buf, sizeof buf, "%s t%d r%d", kind, tick, range);
    fprintf(stderr, "  host %7.1f us: %s\n", host_now_us() - g_log.host_t0, buf);
}
static void log_tag(mrca::EnvView& v, const char* kind, int tick, int range) {
    v.launch_stamps = nullptr;
    if (!g_log.on || (int)g_log.what.size() >= kLogSlots) return;
    char buf[64];
    snprintf(buf, sizeof buf, "%s t%d r%d", kind, tick, range);
    v.launch_stamps = g_log.dev;
    v.launch_slot = (int)g_log.what.size();
    g_log.what.push_back(buf);
    g_log.host_at.push_back(host_now_us() - g_log.host_t0);
}
static void log_end() {
    if (!g_log.on) return;
    const double host_done = host_now_us() - g_log.host_t0;
    (void)hipDeviceSynchronize();
    const double synced = host_now_us() - g_log.host_t0;
    std::vector<unsigned long long> h((size_t)kLogSlots * 2);
    (void)hipMemcpy(h.data(), g_log.dev, h.size() * 8, hipMemcpyDeviceToHost);
    unsigned long long t0 = ~0ull;
    for (size_t i = 0; i < g_log.what.size(); ++i) t0 = h[2 * i] < t0 ? h[2 * i] : t0;
    fprintf(stderr, "# pass of %zu launches: host enqueued for %.1f us, synchronised at %.1f us; device times from the first start\n",
            g_log.what.size(), host_done, synced);
    for (size_t i = 0; i < g_log.what.size(); ++i)
        fprintf(stderr, "%-14s enqueued %7.1f | starts %7.2f ends %7.2f (%6.2f us)\n", g_log.what[i].c_str(), g_log.host_at[i],
                (double)(h[2 * i] - t0) / 100.0, (double)(h[2 * i + 1] - t0) / 100.0, (double)(h[2 * i + 1] - h[2 * i]) / 100.0);
}
#define MRCA_LOG_BEGIN() log_begin()
#define MRCA_LOG_TAG(v, kind, tick, range) log_tag(v, kind, tick, range)
#define MRCA_LOG_END() log_end()
#else
#define MRCA_LOG_BEGIN() ((void)0)
#define MRCA_LOG_TAG(v, kind, tick, range) ((void)0)
#define MRCA_LOG_END() ((void)0)
#endif


// mrca_step_many's action pool: tick k of the call takes the actions at (first_tick + k) modulo the pool's size
struct ActionPool {
    const float* const* dev;
    int32_t count, first_tick;
    const float* operator()(int k) const { return dev[(size_t)((int64_t)first_tick + k) % (size_t)count]; }
};

// One run-ahead pass of mrca_step_many: ticks k0 .. k0 + K - 1 of the call, K <= ahead.slots + 1.  What goes out, and in which
// order, is the pass's plan (mrca_pass_plan.h); this is how.  Tick k's move launch covers ALL worlds, writing its slot and
// reading the tick before's; the first kOwnTicks go out on the caller's stream, the others on the env's move stream, back to
// back -- a slot per tick, so a move launch waits for no ray cast.  The ray casts of world range c run on the range's stream
// (range 0: the caller's), tick after tick, each BLOCK of ticks behind the event "the block's last move launch is through".
// Nothing else is ordered: the ray casts are what a tick costs (16.4 us for 4096 robots as two ranges -- two residency rounds
// of a workgroup's lifetime), the move launches (8.5 us) run beside them.  Every dependency is a stream order
// or an event; nothing spins.
struct AheadPass {
    mrca_env* env;
    ActionPool act;
    int k0, P;
    hipStream_t s0, ms;                // the caller's stream, the move stream
    mrca::PassPlan plan;
    hipError_t herr = hipSuccess;      // the first error: nothing is enqueued behind it
    bool move_forked = false;
    // every range has the ray casts of blocks below ray_blocks, ranges below ray_ranges those of block ray_blocks as well
    int ray_blocks = 0, ray_ranges = 0;

    void moves_of(int b) {
        const int a = plan.first_of[b], e = plan.first_of[b + 1];
        hipStream_t sm = a < mrca::kOwnTicks ? s0 : ms;
        if (a >= mrca::kOwnTicks && !move_forked) {       // the move stream starts behind the caller's last move launch (and so behind the caller's work)
            herr = hipStreamWaitEvent(ms, env->ahead.moved[a - 1].get(), 0);
            if (herr != hipSuccess) return;
            move_forked = true;
        }
        for (int k = a; k < e; ++k) {
            mrca::EnvView mv = slot_view(env, plan.write_slot(k));       // (all worlds, as the env's own view has it)
            const mrca::EnvView in = slot_view(env, plan.read_slot(k));
            MRCA_LOG_TAG(mv, "move", k, 0);
            mrca::launch_move(mv, act(k0 + k), sm, nullptr, nullptr, &in);
        }
        herr = hipEventRecord(env->ahead.moved[e - 1].get(), sm);
    }

    void rays_of(int b) {
        const int W = env->view.W, R = env->view.R;
        const int a = plan.first_of[b], e = plan.first_of[b + 1];
        for (int c = 0; c < P; ++c) {
            hipStream_t sc = range_stream(env, s0, c);
            if (c > 0 || a >= mrca::kOwnTicks) {        // (range 0's first ray casts follow their ticks' move launches on the caller's stream itself)
                herr = hipStreamWaitEvent(sc, env->ahead.moved[e - 1].get(), 0);
                if (herr != hipSuccess) return;
            }
            const int w0 = range_first_world(W, P, c), wn = range_first_world(W, P, c + 1) - w0;
            for (int l = plan.launches_of[b]; l < plan.launches_of[b + 1]; ++l) {
                const mrca::PassPlan::Launch& ln = plan.launch[l];
                const int k = ln.first, slot = plan.write_slot(k);
                mrca::EnvView rv = observing(env, range_view(slot_view(env, ln.ticks > 1 ? 0 : slot), w0 * R, wn * R, w0, wn));
                rv.ring_head = ring_heads(env, ln.heads_in_scratch);
                if (ln.ticks == 1) {
                    MRCA_LOG_TAG(rv, "ray", k, c);
                    mrca::launch_raycast(rv, /*only_fresh=*/0, sc);
                    continue;
                }
                mrca::RayTicks t = slot_ticks(env, slot, ln.ticks, /*last_is_env=*/k + ln.ticks == plan.K, rv.ring_head,
                                              ring_heads(env, !ln.heads_in_scratch));
                MRCA_LOG_TAG(rv, "rays", k, c);
#if defined(MRCA_PROFILING)
                t.in.launch_stamps = rv.launch_stamps;
                t.in.launch_slot = rv.launch_slot;
#endif
                mrca::launch_raycast_ticks(rv, t, sc);
            }
            ray_ranges = c + 1;
        }
        ray_blocks = b + 1;
        ray_ranges = 0;
    }

    // where range c's ring heads are behind the launches it has been given
    int heads_in_scratch(int c) const { return plan.launch[plan.launches_of[ray_blocks + (c < ray_ranges ? 1 : 0)]].heads_in_scratch; }
};

static int run_ahead_pass(mrca_env* env, const ActionPool& act, int k0, int K, int P, hipStream_t s0) {
    const int W = env->view.W, R = env->view.R;
    AheadPass pass{env, act, k0, P, s0, env->ahead.move_stream.get()};
    MRCA_LOG_BEGIN();
    mrca::plan_pass(K, mrca::ticks_per_launch(env->cfg.lazy_obs, env->ahead.ticks_per_launch, env->ahead.ticks_forced,
                                              env->view.raster_inv > 0.0f, W, R, P), &pass.plan);
    for (int i = 0; i < pass.plan.num_ops && pass.herr == hipSuccess; ++i) {
        const mrca::PassPlan::Op& op = pass.plan.ops[i];
        if (op.kind == mrca::PassPlan::kMoves) pass.moves_of(op.block);
        else pass.rays_of(op.block);
    }
    const hipError_t herr = pass.herr;
    // an early exit may leave a range's ring heads in the scratch array: back into the env's field, behind the range's launches
    for (int c = 0; c < P; ++c)
        if (pass.heads_in_scratch(c)) {
            const int n0 = range_first_world(W, P, c) * R, n1 = range_first_world(W, P, c + 1) * R;
            (void)hipMemcpyAsync(env->view.ring_head + n0, env->ahead.head_scratch.get() + n0, (size_t)(n1 - n0),
                                 hipMemcpyDeviceToDevice, range_stream(env, s0, c));
        }
    // join: the caller's stream continues when every range is through (the move stream is: range 0 waited for its last launch)
    hipError_t jerr = join_ranges(env, s0, P);
    if (pass.move_forked && herr != hipSuccess) {     // an early exit: the move stream may still be forked off the caller's
        hipError_t e1 = hipEventRecord(env->fork.get(), pass.ms);
        hipError_t e2 = hipStreamWaitEvent(s0, env->fork.get(), 0);
        if (jerr == hipSuccess) jerr = e1 != hipSuccess ? e1 : e2;
    }
    MRCA_LOG_END();
    if (herr != hipSuccess) return fail(MRCA_ERR_HIP, "mrca_step_many: %s", hipGetErrorString(herr));
    if (jerr != hipSuccess) return fail(MRCA_ERR_HIP, "mrca_step_many (join): %s", hipGetErrorString(jerr));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_step_many(mrca_env* env, const float* const* actions_dev, int32_t num_actions, int32_t first_tick, int32_t num_ticks,
                   int32_t chains, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!actions_dev || num_actions < 1) return fail(MRCA_ERR_INVALID, "mrca_step_many: no actions");
    if (first_tick < 0 || num_ticks < 0) return fail(MRCA_ERR_INVALID, "mrca_step_many: first_tick %d, num_ticks %d", first_tick, num_ticks);
    for (int i = 0; i < num_actions; ++i)
        if (!actions_dev[i]) return fail(MRCA_ERR_INVALID, "mrca_step_many: actions_dev[%d] is NULL", i);
    const int W = env->view.W;
    const bool chained = chains < 0;          // chains = -P: round 5's schedule (P chains `move, ray, move, ray ...` half a tick apart)
    int P = chains < 0 ? -chains : chains;
    if (P < 1) P = 1;
    if (P > W) P = W;
    if (env->view.big) P = 1;
    const ActionPool act{actions_dev, num_actions, first_tick};
    DeviceGuard guard(env->cfg.device);
    hipStream_t s0 = static_cast<hipStream_t>(stream);
    // streams and events of ranges beyond the ones mrca_create made: never inside a capture (stream creation is not capturable)
    while ((int)env->ranges.size() < P - 1) {
        if (capturing(s0))
            return fail(MRCA_ERR_INVALID, "mrca_step_many: chains %d needs streams the env has not created yet -- call it once "
                                          "outside the capture first (mrca_create prepares chains <= %d)", P, kChainStreamsAtCreate + 1);
        HIP_TRY(add_world_range(env));
    }
    if (!env->fork) HIP_TRY(make_event(&env->fork));
    if (num_ticks == 0) return MRCA_OK;
    if (!env->view.big && (P > 1 || (!chained && env->ahead.slots > 0)) && !env->check.covers(s0, P) &&
        !capturing(s0))                                // (inside a capture: the streams as they are)
        if (int rc = choose_streams(env, s0, P)) return rc;
    if (!chained && !env->view.big && env->ahead.slots > 0) {
        // the run-ahead schedule, in passes of at most ahead.slots + 1 ticks (a pass ends with every stream joined)
        const int per = env->ahead.slots + 1 < kAheadTicks ? env->ahead.slots + 1 : kAheadTicks;
        for (int k0 = 0; k0 < num_ticks; k0 += per) {
            const int K = num_ticks - k0 < per ? num_ticks - k0 : per;
            if (int rc = run_ahead_pass(env, act, k0, K, P, s0)) return rc;
        }
        return MRCA_OK;
    }
    if (P == 1) {
        for (int k = 0; k < num_ticks; ++k)
            if (int rc = step_impl(env, act(k), 0, env->view.N, stream)) return rc;
        return MRCA_OK;
    }
    // (fork: range c's stream starts behind range c - 1's FIRST move launch -- which sits behind everything queued on the caller's
    // stream before this call, so that one wait is the fork AND the half tick between the ranges; the first launch of the call
    // goes out before any event is touched)
    int rc = MRCA_OK;
    hipError_t herr = hipSuccess;
    int forked = 1;          // ranges below this index have launches on their streams: they must be joined on every path
    for (int k = 0; k < num_ticks && rc == MRCA_OK && herr == hipSuccess; ++k) {
        const float* a = act(k);
        for (int c = 0; c < P; ++c) {
            hipStream_t sc = range_stream(env, s0, c);
            const int w0 = range_first_world(W, P, c), wn = range_first_world(W, P, c + 1) - w0;
            // half a tick behind the previous range, once: its first move launch has finished, its first ray cast is starting
            if (k == 0 && c > 0) {
                herr = hipStreamWaitEvent(sc, env->ranges[c - 1].moved.get(), 0);
                if (herr != hipSuccess) break;
                forked = c + 1;
            }
            if ((rc = worlds_impl(env, a, w0, wn, sc, kPhaseMove))) break;
            if (k == 0 && c + 1 < P && (herr = hipEventRecord(env->ranges[c].moved.get(), sc)) != hipSuccess) break;
            if ((rc = worlds_impl(env, nullptr, w0, wn, sc, kPhaseObserve))) break;
        }
    }
    const hipError_t jerr = join_ranges(env, s0, forked);      // (on the error paths too)
    if (herr == hipSuccess) herr = jerr;
    if (rc != MRCA_OK) return rc;
    if (herr != hipSuccess) return fail(MRCA_ERR_HIP, "mrca_step_many: %s", hipGetErrorString(herr));
    return MRCA_OK;
}

int mrca_check(mrca_env* env, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    DeviceGuard guard(env->cfg.device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, env->view.status, sizeof(bits), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bits == 0) return MRCA_OK;
    HIP_TRY(hipMemsetAsync(env->view.status, 0, sizeof(bits), s));
    if (bits & mrca::kStatusCollideUndecided)
        return fail(MRCA_ERR_HIP, "collision pass of a world with more than 64 robots gave up waiting for a lower-indexed "
                                  "robot (its bounded wait ran out): at least one robot was left undecided since the last "
                                  "check; the env's state is not to be trusted");
    if (bits & mrca::kStatusOutlineWindow)
        return fail(MRCA_ERR_HIP, "fidelity mode: a cell of a robot's outline fell outside the 8 x 8 window of its bitmap since the "
                                  "last check (coordinates beyond the supported range?); collisions and lidar returns of that "
                                  "robot are not to be trusted");
    if (bits & mrca::kStatusBadRolloutRow)
        return fail(MRCA_ERR_INVALID, "mrca_rollout_store_*: the device-side tick counter was outside [0, horizon) since the last "
                                      "check (that launch stored nothing)");
    if (bits & mrca::kStatusBadBeamIndex)
        return fail(MRCA_ERR_INVALID, "mrca_sparse_obs: the beam table held an index outside [0, beams) since the last check "
                                      "(clamped to the nearest beam)");
    return fail(MRCA_ERR_HIP, "device status word 0x%x", bits);
}

static int check_rows(const mrca_rollout_rows* r) {
    if (!r) return fail(MRCA_ERR_INVALID, "rows is NULL");
    if (!r->frames || !r->fidx || !r->cur || !r->goal || !r->speed || !r->action || !r->logprob || !r->value || !r->reward ||
        !r->done)
        return fail(MRCA_ERR_INVALID, "mrca_rollout_rows: NULL pointer");
    if (r->horizon < 1) return fail(MRCA_ERR_INVALID, "mrca_rollout_rows: horizon %d", r->horizon);
    if ((reinterpret_cast<uintptr_t>(r->frames) % 16) || (reinterpret_cast<uintptr_t>(r->goal) % 8) ||
        (reinterpret_cast<uintptr_t>(r->speed) % 8) || (reinterpret_cast<uintptr_t>(r->action) % 8))
        return fail(MRCA_ERR_INVALID, "mrca_rollout_rows: frames must be 16-byte, goal / speed / action 8-byte aligned");
    return MRCA_OK;
}

int mrca_rollout_store_state(mrca_env* env, const mrca_rollout_rows* rows, const int64_t* tick_dev, const float* action_dev,
                             const float* logprob_dev, const float* value_dev, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (int rc = check_rows(rows)) return rc;
    if (!tick_dev || !action_dev || !logprob_dev || !value_dev)
        return fail(MRCA_ERR_INVALID, "mrca_rollout_store_state: NULL pointer");
    if (reinterpret_cast<uintptr_t>(action_dev) % 8)
        return fail(MRCA_ERR_INVALID, "mrca_rollout_store_state: action_dev must be 8-byte aligned");
    DeviceGuard guard(env->cfg.device);
    mrca::launch_rollout_store_state(env->view, *rows, tick_dev, action_dev, logprob_dev, value_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_rollout_store_outcome(mrca_env* env, const mrca_rollout_rows* rows, int64_t* tick_dev, uint32_t* ticket_dev,
                               void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (int rc = check_rows(rows)) return rc;
    if (!tick_dev || !ticket_dev) return fail(MRCA_ERR_INVALID, "mrca_rollout_store_outcome: NULL pointer");
    DeviceGuard guard(env->cfg.device);
    mrca::launch_rollout_store_outcome(env->view, *rows, tick_dev, ticket_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_normalize_scans(const float* in_dev, float* out_dev, size_t count, void* stream) {
    if (!in_dev || !out_dev) return fail(MRCA_ERR_INVALID, "mrca_normalize_scans: NULL pointer");
    if (count % 4 || reinterpret_cast<uintptr_t>(in_dev) % 16 || reinterpret_cast<uintptr_t>(out_dev) % 16)
        return fail(MRCA_ERR_INVALID, "mrca_normalize_scans: count must be a multiple of 4 and the buffers 16-byte aligned");
    DeviceGuard guard(mrca::device_of(in_dev));
    mrca::launch_normalize(in_dev, out_dev, (long long)count, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_sparse_obs(mrca_env* env, const int32_t* index_dev, int32_t beam_num, float* out_dev, void* stream) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (!index_dev || !out_dev) return fail(MRCA_ERR_INVALID, "mrca_sparse_obs: NULL pointer");
    if (beam_num < 1 || beam_num > env->view.B) return fail(MRCA_ERR_INVALID, "mrca_sparse_obs: beam_num %d not in [1, %d]", beam_num, env->view.B);
    DeviceGuard guard(env->cfg.device);
    mrca::launch_sparse_obs(env->view, index_dev, beam_num, out_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_gae(const float* rewards_dev, const float* values_dev, const float* last_value_dev,
             const uint8_t* dones_dev, float gamma, float lam, int32_t T, int32_t N, float* targets_dev,
             float* advs_dev, void* stream) {
    if (!rewards_dev || !values_dev || !last_value_dev || !dones_dev || !targets_dev || !advs_dev)
        return fail(MRCA_ERR_INVALID, "mrca_gae: NULL pointer");
    if (T < 1 || N < 1) return fail(MRCA_ERR_INVALID, "mrca_gae: T=%d N=%d", T, N);
    DeviceGuard guard(mrca::device_of(rewards_dev));      // launch where the buffers live
    mrca::launch_gae(rewards_dev, values_dev, last_value_dev, dones_dev, gamma, lam, T, N, targets_dev, advs_dev,
                     static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MRCA_OK;
}

int mrca_enable_timing(mrca_env* env, int32_t on) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    if (on && env->ev.empty()) {
        std::vector<Event> ev(4 * kTimingRing);     // (the env's only when every one exists)
        for (Event& e : ev) HIP_TRY(make_event(&e, hipEventDefault));
        env->ev = std::move(ev);
    }
    env->timing = on > 0 ? on : 0;
    env->step_count = 0;
    env->ev_used = 0;
    return MRCA_OK;
}

// What an event pair reads with NOTHING between its two records: the processing time of the second marker, which every
// (event, kernel, event) measurement of mrca_read_timing contains once per kernel.  bench.py reports its kernel
// averages net of this figure so that they add up to no more than the tick they are part of.
int mrca_event_pair_overhead(void* stream, int32_t samples, float* us_out) {
    if (!us_out || samples < 1 || samples > 4096) return fail(MRCA_ERR_INVALID, "mrca_event_pair_overhead: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int dev = 0;
    if (s) {     // the events belong on the stream's device, whatever the caller's current one is
        HIP_TRY(hipStreamGetDevice(s, &dev));
    } else {
        HIP_TRY(hipGetDevice(&dev));
    }
    DeviceGuard guard(dev);
    Event a, b;
    HIP_TRY(make_event(&a, hipEventDefault));
    HIP_TRY(make_event(&b, hipEventDefault));
    double sum = 0.0;
    for (int i = 0; i < samples; ++i) {
        float ms = 0.0f;
        HIP_TRY(hipEventRecord(a.get(), s));
        HIP_TRY(hipEventRecord(b.get(), s));
        HIP_TRY(hipEventSynchronize(b.get()));
        HIP_TRY(hipEventElapsedTime(&ms, a.get(), b.get()));
        sum += ms;
    }
    *us_out = (float)(sum / samples * 1e3);
    return MRCA_OK;
}

#if defined(MRCA_PROFILING)
// Profiling build only (libmrca_env_prof.so): ablation switches (results are WRONG while bits 0-5 are set) and
// launch-shape knobs (results unchanged): bits 8-10 = k > 0:
// 1 << (k-1) beams per marching thread; bit 11: a dedicated fifth preparation wave; bit 12: the beams of a thread marched
// in lock step instead of one after the other.
int mrca_set_debug_flags(mrca_env* env, int32_t flags) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    env->view.debug_flags = flags & 0xFF;
    const int knob = (flags >> 8) & 7;
    if (knob) {
        const int shift = knob - 1;
        if (!mrca::ray_knob_ok(env->cfg.beams, shift, (flags & 0x800) != 0))
            return fail(MRCA_ERR_INVALID, "beams-per-thread knob %d out of range, or more than 1024 threads", knob);
        env->view.ray_shift = shift;
    } else {
        env->view.ray_shift = mrca::product_ray_shift(env->cfg.beams, env->view.big);   // the product's launch shape
    }
    env->view.ray_prep_wave = (flags & 0x800) ? 1 : 0;
    env->view.ray_sequential = (flags & 0x1000) ? 0 : 1;
    DeviceGuard guard(env->cfg.device);
    HIP_TRY(upload_view(env));            // move_kernel / raycast_kernel read the switches from the device copy
    return MRCA_OK;
}

// Profiling build only: average s_memtime ticks between the move kernel's phase stamps (0 -> 1 ... 7 -> 8) over the worlds
// of the LAST launch (synchronises the device).
int mrca_debug_move_stamps(mrca_env* env, double* avg_ticks_out /* [9]: 8 deltas + entry-to-end */) {
    if (!env || !avg_ticks_out) return fail(MRCA_ERR_INVALID, "NULL argument");
    DeviceGuard guard(env->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const int W = env->view.W < 4096 ? env->view.W : 4096;
    std::vector<unsigned long long> h((size_t)10 * W);
    mrca::read_move_stamps(h.data(), W);
    for (int k = 0; k < 8; ++k) {
        double sum = 0.0;
        for (int w = 0; w < W; ++w) sum += (double)(h[(size_t)(k + 1) * W + w] - h[(size_t)k * W + w]);
        avg_ticks_out[k] = sum / W;
    }
    double sum = 0.0;
    for (int w = 0; w < W; ++w) sum += (double)(h[(size_t)8 * W + w] - h[w]);
    avg_ticks_out[8] = sum / W;
    return MRCA_OK;
}

// Profiling build only: the raw stamps of the LAST move launch, out[k * worlds + w] = stamp k (0..8) of world w -- for the
// DISTRIBUTION over worlds (a launch lasts as long as its slowest world): tools/move_tail.py
int mrca_debug_move_stamps_raw(mrca_env* env, unsigned long long* out /* [10 * worlds] */, int32_t* worlds_out) {
    if (!env || !out || !worlds_out) return fail(MRCA_ERR_INVALID, "NULL argument");
    DeviceGuard guard(env->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const int W = env->view.W < 4096 ? env->view.W : 4096;
    mrca::read_move_stamps(out, W);
    *worlds_out = W;
    return MRCA_OK;
}

// Profiling build only: s_memtime stamps of the LAST ray-cast launch (synchronises the device).  out[w * 7 + k], w = 0, 1
// (wave 0 prepares the neighbour list, wave 1 only marches), k = 0..6: mean over workgroups of stamp k minus the
// workgroup's entry stamp; out[14..16] = 0 (reserved).
int mrca_debug_ray_stamps(mrca_env* env, double* out /* [17] */) {
    if (!env || !out) return fail(MRCA_ERR_INVALID, "NULL argument");
    DeviceGuard guard(env->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const int nb = env->last_ray_count < 8192 ? env->last_ray_count : 8192;    // the workgroups whose stamps are this launch's
    if (nb < 1) return fail(MRCA_ERR_INVALID, "no ray-cast launch to read stamps of");
    std::vector<unsigned long long> h((size_t)14 * nb);
    mrca::read_ray_stamps(h.data(), nb);
    auto at = [&](int w, int k, int b) { return h[((size_t)w * 7 + k) * nb + b]; };
    for (int w = 0; w < 2; ++w)
        for (int k = 0; k < 7; ++k) {
            double sum = 0.0;
            for (int b = 0; b < nb; ++b) sum += (double)(long long)(at(w, k, b) - at(0, 0, b));
            out[w * 7 + k] = sum / nb;
        }
    // [14..16] reserved: stamps of different workgroups cannot be compared (s_memtime counters have unrelated origins from
    // die to die and within one), only differences inside a workgroup mean something
    out[14] = out[15] = out[16] = 0.0;
    return MRCA_OK;
}
#endif

int mrca_read_timing(mrca_env* env, float* move_ms_total, float* ray_ms_total, int32_t* launches) {
    if (!env) return fail(MRCA_ERR_INVALID, "env is NULL");
    float mv = 0.0f, ry = 0.0f;
    const int n = env->ev_used / 4;
    if (n > 0) HIP_TRY(hipEventSynchronize(env->ev[env->ev_used - 1].get()));
    for (int i = 0; i < n; ++i) {
        float a = 0.0f, b = 0.0f;
        HIP_TRY(hipEventElapsedTime(&a, env->ev[4 * i].get(), env->ev[4 * i + 1].get()));
        HIP_TRY(hipEventElapsedTime(&b, env->ev[4 * i + 2].get(), env->ev[4 * i + 3].get()));
        mv += a;
        ry += b;
    }
    if (move_ms_total) *move_ms_total = mv;
    if (ray_ms_total) *ray_ms_total = ry;
    if (launches) *launches = n;
    env->ev_used = 0;
    return MRCA_OK;
}

}  // extern "C"
