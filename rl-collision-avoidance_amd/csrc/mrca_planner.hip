// mrca_planner.hip -- the global planner (mrca_goal_fields, mrca_subgoals).  The rule is
// mrca_planner_device.h's; what is decided here is who computes what.
//
// PLANNING (goal_field_*_kernel).  The field is the least fixed point of an integer relaxation, so nothing here depends on the
// order in which anything runs.  A round is ONE launch of one workgroup per (goal, tile of 64 x 64 cells): the tile and a
// one-cell halo go into LDS as they stand in global memory (66 x 66 words, 17 KB), thread (x, band) relaxes the 16 cells
// of column x in rows 16 band .. 16 band + 15 -- down the column in even sweeps, up in odd ones, so that a value crosses a band
// within a sweep; a wave's lanes read consecutive words of a row: no bank conflict at a pitch of 66 -- at most kPlanSweeps
// times, with a workgroup-uniform vote (__syncthreads_or) to leave early, and stores the cells of ITS OWN tile that fell.  A
// halo word read while its owner lowers it is an older upper bound; lanes of the workgroup read LDS words their neighbours are
// lowering in the same sweep, likewise.  A workgroup in which something fell, or whose sweeps ran out, adds one to the round's
// counter.  There is no grid-wide barrier, no cooperative launch, no wait on memory: the host relaunches and reads counters
// (mrca_abi_controllers.hip: mrca_goal_fields).  Every loop has a fixed trip count.
//
// PER TICK (subgoal_kernel).  EIGHT LANES PER ROBOT: lane k loads D of neighbour k -- the eight loads of a step are one
// instruction -- takes the two cells a diagonal squeezes between from the lanes beside it, and three butterfly steps over a
// 64-bit key (cost << 3 | direction) leave the step of the rule in all eight.  One thread per robot (subgoal_thread_kernel:
// plan_robot as it stands) is kept beside it for tools/planner_probe.py, which decided between the two: 9.8 against 14.8 us at
// 4092 robots mid-run on the Stage-2 map, 16.8 against 16.9 us at 49 984, the same words (profiles/planner/planner_probe.json).
// Eight lanes ship; the library launches the other only where MRCA_SUBGOAL_LANES=1 asks.  No atomics, no LDS, no
// barrier, plain vector stores, nothing of the env written.  The arguments are 96 bytes (below the 104 at which a launch gets
// dearer for the host, include/mrca_env.h at mrca_create): the env's fields come through its device-side view.
//
// PER TICK WITH LINE OF SIGHT (subgoal_los_kernel).  Two phases with different shapes.  The WALK is a chain of
// dependent loads, up to max(lookahead, reach) long: the eight lanes of subgoal_kernel, unchanged, and the first lane of the
// robot's group drops every cell reached into LDS (one word, j << 16 | i: a map side is at most 16384 cells; 1 KiB per robot).
// The VISIBILITY TESTS of the cells c_W .. c_1 are independent of each other: the group's lanes take candidates from the far end,
// lane l the l-th farthest, one ballot per group of candidates, and the robot leaves at the first group that holds a visible
// one -- its lowest lane is the largest m.  A lane's test is plan_visible as it stands (a divergent loop of loads, at most
// 2 * 256 trips).  The group is a template parameter: 8 lanes (32 robots and 33 KB of LDS per workgroup) or a whole wavefront
// (4 robots, 4 KB; the walk then runs eight times over in the same instructions).  tools/planner_probe.py measured both and
// neither wins everywhere (profiles/planner_los/planner_los_probe.json, medians, Stage-2 map, reach 15 / 60 / 256): at 4092
// robots a wavefront takes 22 / 87 / 285 us against 24 / 154 / 1029 us for eight lanes -- the launch is latency-bound and a
// wavefront tests 64 candidates in the time eight lanes test 8 -- at 49 984 robots 144 / 450 / 935 us against 53 / 307 / 1878:
// there the redundant walks and the 16 times as many workgroups cost more than the wider search saves, except at reach 256.
// The library gives a robot a wavefront while every robot's fits on the chip at once in that shape (8192 robots) and eight
// lanes beyond (mrca_abi_controllers.hip); the same words either way.  A group never spans wavefronts: the LDS row of a robot is written and read by one wave, so a
// wavefront-scope fence stands where a barrier would.  No atomics, no spinning, every loop has a fixed bound, nothing of the
// env written.  The arguments are 96 bytes as subgoal_kernel's: stride, lookahead and reach travel packed in one word.
#include "mrca_planner.h"

namespace mrca {

namespace {

constexpr int kBlock = 256;
constexpr int kPitch = kPlanTile + 2;
constexpr int kBand = kPlanTile * kPlanTile / kBlock;   // 16 cells of a column per thread
static_assert(kBlock == 4 * kPlanTile && kBand * 4 == kPlanTile, "a thread owns a quarter of a column");

// the seed of goal point (gx, gy): its planning cell index, or -1 (off grid)
__device__ __forceinline__ long long seed_index(const GridGeom& g, int s, int pw, float gx, float gy) {
    int ix, iy;
    if (!plan_map_cell(g, gx, gy, &ix, &iy)) return -1;
    return (long long)(iy / s) * pw + (ix / s);
}

__global__ __launch_bounds__(kBlock) void goal_field_init_kernel(const EnvView* __restrict__ view_p, const int s, const int inflate,
                                                                 const float* __restrict__ goals, uint32_t* __restrict__ field) {
    const EnvView& e = *view_p;
    const GridGeom g = e.g;
    const int pw = plan_cells(g.width, s), ph = plan_cells(g.height, s);
    const long long cells = (long long)pw * ph;
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    const int goal = blockIdx.y;
    const int i = (int)(c % pw), j = (int)(c / pw);
    const long long seed = seed_index(g, s, pw, goals[2 * (size_t)goal], goals[2 * (size_t)goal + 1]);
    field[(size_t)goal * (size_t)cells + (size_t)c] = plan_field_init(c == seed, plan_blocked(e.cellfield, g, s, inflate, i, j));
}

__global__ __launch_bounds__(kBlock) void goal_field_finish_kernel(const long long words, uint32_t* __restrict__ field) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (c < words && field[c] == kPlanWall) field[c] = kPlanInf;
}

// (field is read -- the halo -- where another workgroup of the launch writes: no __restrict__)
__global__ __launch_bounds__(kBlock) void goal_field_kernel(const int pw, const int ph, const int tiles_x, uint32_t* field,
                                                            uint32_t* __restrict__ counter) {
    __shared__ uint32_t lds[kPitch * kPitch];
    const int tid = threadIdx.x;
    const int ti = (int)(blockIdx.x % (unsigned)tiles_x), tj = (int)(blockIdx.x / (unsigned)tiles_x);
    uint32_t* f = field + (size_t)blockIdx.y * (size_t)pw * (size_t)ph;
    const int i0 = ti * kPlanTile - 1, j0 = tj * kPlanTile - 1;
    for (int t = tid; t < kPitch * kPitch; t += kBlock) {
        const int lx = t % kPitch, ly = t / kPitch;
        const int i = i0 + lx, j = j0 + ly;
        const bool in = i >= 0 && j >= 0 && i < pw && j < ph;
        lds[t] = in ? f[(size_t)j * (size_t)pw + (size_t)i] : kPlanWall;
    }
    __syncthreads();
    const int lx = (tid & (kPlanTile - 1)) + 1;
    const int ly0 = (tid >> 6) * kBand + 1;
    uint32_t orig[kBand];
#pragma unroll
    for (int r = 0; r < kBand; ++r) orig[r] = lds[(ly0 + r) * kPitch + lx];
    int more = 1;
    for (int sweep = 0; sweep < kPlanSweeps; ++sweep) {
        int changed = 0;
        for (int r = 0; r < kBand; ++r) {
            const int ly = ly0 + ((sweep & 1) ? kBand - 1 - r : r);
            const int at = ly * kPitch + lx;
            uint32_t n[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) n[k] = lds[at + plan_dy(k) * kPitch + plan_dx(k)];
            const uint32_t cur = lds[at];
            const uint32_t v = plan_relax(cur, n);
            if (v != cur) {
                lds[at] = v;
                changed = 1;
            }
        }
        more = __syncthreads_or(changed);
        if (!more) break;           // (workgroup-uniform)
    }
    // the cells that fell: only this workgroup stores to its tile, and only lower values
    int fell = 0;
    const int i = i0 + lx;
#pragma unroll
    for (int r = 0; r < kBand; ++r) {
        const int j = j0 + ly0 + r;
        const uint32_t v = lds[(ly0 + r) * kPitch + lx];
        if (i < pw && j < ph && v < orig[r]) {
            f[(size_t)j * (size_t)pw + (size_t)i] = v;
            fell = 1;
        }
    }
    fell = __syncthreads_or(fell);
    if (tid == 0 && (fell || more)) atomicAdd(counter, 1u);
}

// what a robot's walk starts from, read once
struct RobotIn {
    float x, y, sn, cs, gx, gy, sgx, sgy;
    const uint32_t* f;       // its slot's field, or nullptr: no slot
};
__device__ __forceinline__ RobotIn robot_in(const EnvView& e, int n, int G, size_t cells, const uint32_t* field, const float* goals,
                                            const int32_t* slot) {
    RobotIn r;
    r.x = e.pose[3 * (size_t)n];
    r.y = e.pose[3 * (size_t)n + 1];
    const float4 hd = e.head[n];
    r.sn = hd.x;
    r.cs = hd.y;
    r.gx = e.goal[2 * (size_t)n];
    r.gy = e.goal[2 * (size_t)n + 1];
    const int sl = slot ? slot[n] : n % e.R;
    const bool has = sl >= 0 && sl < G;
    r.f = has ? field + (size_t)sl * cells : nullptr;
    r.sgx = has ? goals[2 * (size_t)sl] : 0.0f;
    r.sgy = has ? goals[2 * (size_t)sl + 1] : 0.0f;
    return r;
}
__device__ __forceinline__ void robot_out(const PlanResult& r, int n, float* local, float* subgoal, float* dist, int32_t* status) {
    *reinterpret_cast<float2*>(local + 2 * (size_t)n) = make_float2(r.lx, r.ly);
    if (subgoal) {
        subgoal[2 * (size_t)n] = r.sx;
        subgoal[2 * (size_t)n + 1] = r.sy;
    }
    if (dist) dist[n] = r.dist;
    if (status) status[n] = r.status;
}

__global__ __launch_bounds__(kBlock) void subgoal_kernel(const EnvView* __restrict__ view_p, const PlannerParams q, const int32_t N,
                                                         const int32_t G, const uint32_t* __restrict__ field,
                                                         const float* __restrict__ goals, const int32_t* __restrict__ slot,
                                                         const uint8_t* __restrict__ mask, float* __restrict__ local,
                                                         float* __restrict__ subgoal, float* __restrict__ dist,
                                                         int32_t* __restrict__ status) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int k = t & 7;
    const int n = t >> 3;
    // a robot that is not there or not asked for keeps its eight lanes in the shuffles below and touches no memory
    const bool active = n < N && (!mask || mask[n < N ? n : 0]);
    const EnvView& e = *view_p;
    const GridGeom g = e.g;
    const int s = q.stride, pw = plan_cells(g.width, s), ph = plan_cells(g.height, s);
    RobotIn rb = {};
    if (active) rb = robot_in(e, n, G, (size_t)pw * (size_t)ph, field, goals, slot);
    int ix = 0, iy = 0;
    const bool walked = active && plan_map_cell(g, rb.x, rb.y, &ix, &iy) && rb.f != nullptr;
    int ci = ix / s, cj = iy / s;
    uint32_t dc = walked ? rb.f[(size_t)cj * (size_t)pw + (size_t)ci] : kPlanInf;
    const uint32_t d0 = dc;
    bool nocand = false, live = walked;
    const int dxk = plan_dx(k), dyk = plan_dy(k);
    for (int step = 0; step < q.lookahead; ++step) {
        live = live && dc != 0u;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;       // (wave-uniform: every lane stays in the shuffles)
        const int ni = ci + dxk, nj = cj + dyk;
        const bool in = live && ni >= 0 && nj >= 0 && ni < pw && nj < ph;
        const uint32_t dn = in ? rb.f[(size_t)nj * (size_t)pw + (size_t)ni] : kPlanInf;
        const uint32_t da = (uint32_t)__shfl((int)dn, (k + 7) & 7, 8);
        const uint32_t db = (uint32_t)__shfl((int)dn, (k + 1) & 7, 8);
        unsigned long long key = plan_key(dc, dn, da, db, k);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) key = plan_key_min(key, __shfl_xor(key, o, 8));
        if (live) {
            if (key == ~0ull) {
                nocand = step == 0;
                live = false;
            } else {
                live = plan_take(key, &ci, &cj, &dc);
            }
        }
    }
    if (active && k == 0) {
        const PlanResult r = plan_result(g, s, rb.f != nullptr, walked, nocand, ci, cj, dc, d0, rb.sgx, rb.sgy, rb.gx, rb.gy, rb.x, rb.y,
                                         rb.sn, rb.cs);
        robot_out(r, n, local, subgoal, dist, status);
    }
}

__global__ __launch_bounds__(kBlock) void subgoal_thread_kernel(const EnvView* __restrict__ view_p, const PlannerParams q, const int32_t N,
                                                                const int32_t G, const uint32_t* __restrict__ field,
                                                                const float* __restrict__ goals, const int32_t* __restrict__ slot,
                                                                const uint8_t* __restrict__ mask, float* __restrict__ local,
                                                                float* __restrict__ subgoal, float* __restrict__ dist,
                                                                int32_t* __restrict__ status) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    if (mask && !mask[n]) return;
    const EnvView& e = *view_p;
    const GridGeom g = e.g;
    const size_t cells = (size_t)plan_cells(g.width, q.stride) * (size_t)plan_cells(g.height, q.stride);
    const RobotIn rb = robot_in(e, n, G, cells, field, goals, slot);
    const float sg[2] = {rb.sgx, rb.sgy}, gl[2] = {rb.gx, rb.gy};
    robot_out(plan_robot(g, q, rb.f, sg, gl, rb.x, rb.y, rb.sn, rb.cs), n, local, subgoal, dist, status);
}

constexpr int kLosPitch = kLosMaxPath + 1;          // (odd: robots of a wave that store step W alike hit different banks)

template <int LPR>
__global__ __launch_bounds__(kBlock) void subgoal_los_kernel(const EnvView* __restrict__ view_p, const uint32_t packed, const int32_t N,
                                                             const int32_t G, const uint32_t* __restrict__ field,
                                                             const float* __restrict__ goals, const int32_t* __restrict__ slot,
                                                             const uint8_t* __restrict__ mask, float* __restrict__ local,
                                                             float* __restrict__ subgoal, float* __restrict__ dist,
                                                             int32_t* __restrict__ status, int32_t* __restrict__ ahead) {
    static_assert(LPR == 8 || LPR == 64, "a robot's group is eight lanes or a wavefront");
    constexpr int kRobots = kBlock / LPR;
    __shared__ uint32_t path[kRobots * kLosPitch];
    const int s = (int)(packed & 0xFu), L = (int)((packed >> 8) & 0x1FFu), reach = (int)((packed >> 20) & 0x1FFu);
    const int gl = threadIdx.x & (LPR - 1);             // the lane within the robot's group
    const int k = gl & 7;
    uint32_t* my_path = path + (threadIdx.x / LPR) * kLosPitch;
    const int n = (int)((blockIdx.x * (unsigned)kBlock + threadIdx.x) / (unsigned)LPR);
    // a robot that is not there or not asked for keeps its lanes in the shuffles and ballots below and touches no memory
    const bool active = n < N && (!mask || mask[n < N ? n : 0]);
    const EnvView& e = *view_p;
    const GridGeom g = e.g;
    const int pw = plan_cells(g.width, s), ph = plan_cells(g.height, s);
    RobotIn rb = {};
    if (active) rb = robot_in(e, n, G, (size_t)pw * (size_t)ph, field, goals, slot);
    int ix = 0, iy = 0;
    const bool walked = active && plan_map_cell(g, rb.x, rb.y, &ix, &iy) && rb.f != nullptr;
    const int i0 = ix / s, j0 = iy / s;
    int ci = i0, cj = j0;
    uint32_t dc = walked ? rb.f[(size_t)cj * (size_t)pw + (size_t)ci] : kPlanInf;
    const uint32_t d0 = dc;
    bool nocand = false, live = walked;
    int W = 0;
    const int dxk = plan_dx(k), dyk = plan_dy(k);
    const int steps = imin(imax(L, reach), kLosMaxPath);
    // ---- the walk: subgoal_kernel's, every group of eight lanes of the robot's group alike
    for (int step = 0; step < steps; ++step) {
        live = live && dc != 0u;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;       // (wave-uniform: every lane stays in the shuffles)
        const int ni = ci + dxk, nj = cj + dyk;
        const bool in = live && ni >= 0 && nj >= 0 && ni < pw && nj < ph;
        const uint32_t dn = in ? rb.f[(size_t)nj * (size_t)pw + (size_t)ni] : kPlanInf;
        const uint32_t da = (uint32_t)__shfl((int)dn, (k + 7) & 7, 8);
        const uint32_t db = (uint32_t)__shfl((int)dn, (k + 1) & 7, 8);
        unsigned long long key = plan_key(dc, dn, da, db, k);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) key = plan_key_min(key, __shfl_xor(key, o, 8));
        if (live) {
            if (key == ~0ull) {
                nocand = step == 0;
                live = false;
            } else {
                live = plan_take(key, &ci, &cj, &dc);
                if (live) {
                    if (gl == 0) my_path[W] = ((uint32_t)cj << 16) | (uint32_t)ci;      // (W < steps <= kLosMaxPath)
                    ++W;
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- the largest visible m: candidates from the far end, LPR at a time
    const int shift = (int)(threadIdx.x & (kWave - 1)) & ~(LPR - 1);
    const unsigned long long group = LPR == 64 ? ~0ull : ((1ull << (LPR & 63)) - 1ull);
    int m_vis = 0;
    bool searching = W >= 1;
    for (int base = 0; base < kLosMaxPath; base += LPR) {
        if (__builtin_amdgcn_ballot_w64(searching) == 0ull) break;  // (wave-uniform)
        const int m = W - base - gl;
        bool vis = false;
        if (searching && m >= 1) {
            const uint32_t c = my_path[m - 1];
            vis = plan_visible(rb.f, pw, ph, i0, j0, (int)(c & 0xFFFFu), (int)(c >> 16));
        }
        const unsigned long long seen = (__builtin_amdgcn_ballot_w64(vis) >> shift) & group;
        if (searching && seen != 0ull) {
            m_vis = W - base - (int)__builtin_ctzll(seen);
            searching = false;
        }
        searching = searching && base + LPR < W;
    }
    if (active && gl == 0) {
        const int m = plan_los_choose(m_vis, L, W);
        if (m >= 1) {
            const uint32_t c = my_path[m - 1];
            ci = (int)(c & 0xFFFFu);
            cj = (int)(c >> 16);
            dc = rb.f[(size_t)cj * (size_t)pw + (size_t)ci];
        }
        const PlanResult r = plan_result(g, s, rb.f != nullptr, walked, nocand, ci, cj, dc, d0, rb.sgx, rb.sgy, rb.gx, rb.gy, rb.x, rb.y,
                                         rb.sn, rb.cs);
        robot_out(r, n, local, subgoal, dist, status);
        if (ahead) {
            ahead[2 * (size_t)n] = m;
            ahead[2 * (size_t)n + 1] = m_vis;
        }
    }
}

}  // namespace

void launch_goal_field_init(const EnvView& e, const PlannerParams& p, const float* goals, int G, uint32_t* field, hipStream_t s) {
    const long long cells = (long long)plan_cells(e.g.width, p.stride) * plan_cells(e.g.height, p.stride);
    hipLaunchKernelGGL(goal_field_init_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock), (unsigned)G), dim3(kBlock), 0, s, e.dev,
                       (int)p.stride, (int)p.inflate, goals, field);
}

void launch_goal_field_round(const EnvView& e, const PlannerParams& p, int G, uint32_t* field, uint32_t* counter, hipStream_t s) {
    const int pw = plan_cells(e.g.width, p.stride), ph = plan_cells(e.g.height, p.stride);
    const int tx = plan_cells(pw, kPlanTile), ty = plan_cells(ph, kPlanTile);
    hipLaunchKernelGGL(goal_field_kernel, dim3((unsigned)(tx * ty), (unsigned)G), dim3(kBlock), 0, s, pw, ph, tx, field, counter);
}

void launch_goal_field_finish(const EnvView& e, const PlannerParams& p, int G, uint32_t* field, hipStream_t s) {
    const long long words = (long long)plan_cells(e.g.width, p.stride) * plan_cells(e.g.height, p.stride) * G;
    hipLaunchKernelGGL(goal_field_finish_kernel, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, words, field);
}

void launch_subgoals(const EnvView& e, const PlannerParams& p, const uint32_t* field, const float* goals, int G, const int32_t* slot,
                     const uint8_t* mask, float* local, float* subgoal, float* dist, int32_t* status, int lanes, hipStream_t s) {
    if (lanes == 1) {
        hipLaunchKernelGGL(subgoal_thread_kernel, dim3((e.N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, e.dev, p, (int32_t)e.N, (int32_t)G,
                           field, goals, slot, mask, local, subgoal, dist, status);
        return;
    }
    constexpr int kRobotsPerBlock = kBlock / 8;
    hipLaunchKernelGGL(subgoal_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, e.dev, p, (int32_t)e.N,
                       (int32_t)G, field, goals, slot, mask, local, subgoal, dist, status);
}

void launch_subgoals_los(const EnvView& e, const PlannerParams& p, const LosParams& lp, const uint32_t* field, const float* goals, int G,
                         const int32_t* slot, const uint8_t* mask, float* local, float* subgoal, float* dist, int32_t* status,
                         int32_t* ahead, int lanes, hipStream_t s) {
    const uint32_t packed = (uint32_t)p.stride | ((uint32_t)p.lookahead << 8) | ((uint32_t)lp.reach << 20);
    if (lanes == 64) {
        constexpr int kRobotsPerBlock = kBlock / 64;
        hipLaunchKernelGGL(subgoal_los_kernel<64>, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, e.dev, packed,
                           (int32_t)e.N, (int32_t)G, field, goals, slot, mask, local, subgoal, dist, status, ahead);
        return;
    }
    constexpr int kRobotsPerBlock = kBlock / 8;
    hipLaunchKernelGGL(subgoal_los_kernel<8>, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, e.dev, packed,
                       (int32_t)e.N, (int32_t)G, field, goals, slot, mask, local, subgoal, dist, status, ahead);
}

}  // namespace mrca
