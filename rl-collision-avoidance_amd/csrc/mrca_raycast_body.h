// mrca_raycast_body.h -- what one workgroup of a ray cast does for its robot: raycast_body, shared by the single-tick
// raycast_kernel (mrca_kernels.hip) and raycast_ticks_kernel (mrca_raycast_ticks.hip), which casts several ticks of
// mrca_step_many in one launch.  Device code only.
#pragma once
#include "mrca_kernels.h"

namespace mrca {

namespace {

// the profiling build's phase stamps (mrca_kernels.hip defines them before it includes this file)
#if !defined(MRCA_RSTAMP)
#define MRCA_RSTAMP(k) do { } while (0)
#endif

// A launch of several ticks (raycast_body<..., TICKS = true>): which tick of the launch this workgroup casts and where the
// fresh flags of all its ticks and the two head arrays are.  The single-tick kernel passes an empty one.
struct RayTick {
    int j, T;                       // this workgroup's tick of the launch's T
    // The fresh flags of the ticks that read ring slots -- all T, or all but the last when that one reads the env's own field
    // (last_is_env) --: tick t's lie (t - lo_tick) * stride bytes behind fresh_lo, the lowest-addressed of them, so that an
    // unsigned 32-bit offset reaches every one (launch_raycast_ticks checks that it does).
    const uint8_t* fresh_lo;
    int stride, lo_tick, ring_last; // (ring_last: the last tick whose flags are in a ring slot)
    int env_tick;                   // the tick that reads the env's own field: T - 1, or none of 0 .. 63
    const uint8_t* head_in;         // the ring heads before the launch's first tick
    uint8_t* head_out;              // ... and where its last tick leaves them (never the same array)
};

// a robot's x and y in the pose array [N][3]: a pair that is aligned like a float
struct alignas(4) PoseXY { float x, y; };

// LDS |= without a return value (ds_or_b64): nothing to wait for
__device__ __forceinline__ void mask_or(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// blockIdx -> robot: consecutive robots (one world's robots) share an XCD's L2 (block b runs on
// XCD b % 8, guide T1); a pure permutation, so correctness never depends on it.
// (unsigned arithmetic: b and N are never negative, and a signed % 8 and / 8 are eleven scalar instructions where three do)
__device__ __forceinline__ int block_to_robot(int b, int N) {
    const uint32_t ub = (uint32_t)b, un = (uint32_t)N;
    if (un & 7u) return b;
    return (int)((ub & 7u) * (un >> 3) + (ub >> 3));
}

// The march reads the free-rectangle field straight from its L1/L2-resident global copy: ~2 dependent
// lookups per ray.  (Staging a tile of it in LDS per robot was measured slower at every granularity tried,
// the tile costs more to fill than the few lookups it serves.  So were persistent workgroups
// walking several robots each -- 39 vs 37 us, profiles/r01/r01_ad_ablation.txt -- and nontemporal stores made
// no difference.)  Marching the K beams of a thread in LOCK STEP (grid_march_skip_n: K lookups in flight per wait) is
// implemented and measured too: slower than one after the other (34.7 vs 28.1 us, profiles/r02/r02_c_*), see mrca_abi.hip.
// RKW > 0: fidelity mode's lidar (the other robots seen through the collision raster; RKW = cells per side of an outline's
// window, 4 or 8) -- a kernel of its own so that the default one does not carry the code: with the raster path behind a
// run-time branch the default launch was 0.85 us slower (A/B on one box, profiles/r04_h_ab_raster_path_in_default_kernel.txt:
// twice the instructions for the same instruction cache).  Since round 5 a beam's return from another robot's outline is a
// closed form over that robot's 16-byte outline record (ray_outline_entry) instead of a walk through a window of LDS bits.
// TICKS: the workgroup casts tick mt.j of a launch of mt.T ticks (raycast_ticks_kernel) -- pose_p / head_p / e.goal / e.outline
// are that tick's; what differs is the ring's bookkeeping (ring_rule, mrca_device.h) and that only the launch's last tick
// stores local_goal and the head.  ring_head_p is unused then.
template <int K, bool BIG, bool SEQ, int RKW, bool VIEWS, bool TICKS = false>
__device__ __forceinline__ void raycast_body(int only_fresh, int ray_first, int ray_count, int R_, const float* __restrict__ pose_p,
                                             const float4* __restrict__ head_p, const float* __restrict__ bcos_p,
                                             const float* __restrict__ bsin_p, uint8_t* ring_head_p, const EnvView& e, int views,
                                             const RayTick& mt = RayTick{}) {
    // (the leading arguments repeat e.ray_first, e.ray_count, e.R, e.pose, e.head, e.beam_cos, e.beam_sin, e.ring_head: 14
    // dwords preloaded into SGPRs, see move_kernel)
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    MRCA_RSTAMP(0);
    const int n = ray_first + block_to_robot(blockIdx.x, ray_count);
    const int tid = threadIdx.x;
    // (A variant of this kernel without the early exit -- so that nothing is waited for before every request of the
    // workgroup is out -- was measured and changed nothing: 27.96 us either way, profiles/r03/r03_l_bench_env.json.  The
    // launch ALONE uses ~45 % of the VALU issue slots: what it waits for is a workgroup's chain of dependent round trips at full
    // occupancy, and one early exit less does not shorten that chain.  Under mrca_step_many's run-ahead schedule, launches of
    // two world ranges and the move launches in flight at once, the same instructions fill ~60 % of the slots and the tick
    // follows their count nearly 1 : 1 -- DESIGN.md 5.2.)
    if (only_fresh && e.fresh[n] == 0) return;  // block-uniform

    float4* nb = reinterpret_cast<float4*>(lds);
    int2* nbi = reinterpret_cast<int2*>(nb + kWave);
    int* nb_count = reinterpret_cast<int*>(nbi + kWave);
    unsigned long long* nbmask = reinterpret_cast<unsigned long long*>(nb_count + 4);   // [B] neighbours per beam
    int* nb_more = nb_count + 1;                                      // big worlds: another chunk of neighbours follows
    // Small worlds' exact rectangles test the (neighbour, beam) pairs dealt densely to the threads instead of each thread its
    // beams' neighbours (slab_pair_locate, mrca_device.h).  Then nbi[k] is (lo_k, start_k), nb_count[2] the number of pairs, and
    // the masks' space holds the beams' ranges, 4 of its 8 bytes per beam: the marched range's bit pattern, which the pairs'
    // entry distances are merged into (slab_pair_merge).
    constexpr bool PAIRS = !BIG && RKW == 0;
    int* rmin = reinterpret_cast<int*>(nb_count + 4);                 // [B]
    // fidelity mode (never in big worlds): the neighbours' outline records
    constexpr bool raster = RKW > 0 && !BIG;
    int4* nbo = reinterpret_cast<int4*>(nbmask + e.B);   // [64] OutlineBits as (ax, ay, lo, hi)

    const int T = e.B / K;                    // marching threads
    const bool extra = (int)blockDim.x > T;   // a dedicated preparation wave sits behind the marching ones
    const int prep_base = extra ? T : 0;
    const bool is_prep = tid >= prep_base && tid < prep_base + kWave;   // wave-uniform
    const bool marches = tid < T;                                       // wave-uniform
    // n / R without the ~25 scalar instructions of a 32-bit division: small worlds (R <= 64, n < 2^24) take the exact multiply-high
    // with the host's ceil(2^32 / R) (error n x (m R - 2^32) < 2^24 x 64 < 2^32).  (A scalar instruction costs the launch twice
    // what a vector one costs -- one scalar unit per CU for 32 waves: profiles/r06_ac_*.)
    const int world = BIG ? n / R_ : (R_ == 1 ? n : (int)__umulhi((uint32_t)n, e.r_magic));   // (2^32 / 1 does not fit the magic)
    const int local = n - world * R_;
    // the robot's own record: pose, sin / cos and the field entry of its cell.  Block-uniform -- but fetched with VECTOR
    // loads (the index goes through an opaque zero): as scalar loads they shared the out-of-order scalar counter with
    // the kernel arguments, and the neighbour candidate below could not be requested before they were back.
    // (Not in big worlds: there the neighbour enumeration hashes the robot's cell per chunk, wave-uniform work that
    // belongs on the scalar unit -- measured: 513 vs 492 us per 50 000-robot launch, profiles/r03/r03_s_bigworld_shards8.jsonl.)
    int lane_zero = 0;
    if constexpr (!BIG) asm volatile("v_mov_b32 %0, 0" : "=v"(lane_zero));
    const int nv = n + lane_zero;
    // (pose_p, head_p and the beam table are kernel arguments, uniform: every load through them is base + a 32-bit byte offset,
    // n < 2^24 -- one global_load with the base in scalar registers, like the loads through the view)
    // (x and y as ONE load of a pair that is aligned like a float; small worlds: the index in a vector register, a full-rate
    // 24-bit multiply)
    auto pose_xy = [&](int i) { return global_load<PoseXY>(pose_p, BIG ? (uint32_t)i * 12u : __umul24((uint32_t)i, 12u)); };
    const PoseXY xy = pose_xy(nv);
    const float x = xy.x, y = xy.y;
    const float4 hd = global_load<float4>(head_p, (uint32_t)nv * 16u);
    const float s = hd.x, c = hd.y;
    // the preparation wave requests "its" neighbour candidate in the same memory round trip
    const int pl = tid - prep_base;
    const bool cand = !BIG && is_prep && (pl < R_) && (pl != local);
    const int jn = world * R_ + (cand ? pl : local);
    float xj = 0.0f, yj = 0.0f;
    float4 hj = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int4 oj = make_int4(0, 0, 0, 0);
    if (!BIG && is_prep) {
        const PoseXY pj = pose_xy(jn);
        xj = pj.x;
        yj = pj.y;
        if constexpr (raster) {
            oj = global_load<int4>(e.outline, (uint32_t)jn * 16u);
        } else {        // (sin and cos: the half of the record the slab tests want)
            const float2 sc = global_load<float2>(head_p, (uint32_t)jn * 16u);
            hj.x = sc.x;
            hj.y = sc.y;
        }
    }
    // beam directions in the robot frame for this thread's K beams (tid + k*T)
    float bc[K], bs[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t boff = (uint32_t)((marches ? tid : 0) + k * T) * 4u;
        bc[k] = global_load<float>(bcos_p, boff);
        bs[k] = global_load<float>(bsin_p, boff);
    }
    // slot of the newest frame so far (read by every thread BEFORE the first barrier, advanced by thread 0 after it) and
    // the fresh flag: requested last, used last
    // (TICKS: lane t of every wave requests tick t's flag -- the T bytes ring_rule wants, in the same round trip -- and the
    // head comes from the array no workgroup of this launch writes)
    uint8_t fresh_byte;
    int ring_slot;
    if constexpr (TICKS) {
        // (every lane loads -- the lanes behind the last ring tick that tick's flag again: ring_rule ignores their bits -- and
        // through a global address: behind a lane mask or as a flat load the request would wait for every other one of the
        // prologue.  The offset wraps to (t - lo_tick) * stride + n >= 0 whatever the sign of stride.)
        const uint32_t lt = (uint32_t)tid & (uint32_t)(kWave - 1);
        const uint32_t t = lt < (uint32_t)mt.ring_last ? lt : (uint32_t)mt.ring_last;
        fresh_byte = global_load<uint8_t>(mt.fresh_lo, (t - (uint32_t)mt.lo_tick) * (uint32_t)mt.stride + (uint32_t)n);
        // (the pass's last launch of a range: lane T - 1 takes the env's own flag instead.  Every launch requests it -- one
        // line per wave -- and no lane of another launch takes it: a second load and a select, no branch to hold up the
        // requests behind it and no lane mask)
        const uint8_t env_byte = global_load<uint8_t>(e.fresh, (uint32_t)nv);
        fresh_byte = lt == (uint32_t)mt.env_tick ? env_byte : fresh_byte;
        ring_slot = global_load<uint8_t>(mt.head_in, (uint32_t)nv);
    } else {
        fresh_byte = e.fresh[n];
        ring_slot = ring_head_p[n];
    }
    // (The frame stack -- ppo_stage1.py:87-89: popleft / append -- is a ring of raw scans: only the newest one is written,
    // into the slot behind the previous newest one; see materialize_kernel.)
    // big worlds: the candidates come from the lidar hash (3 x 3 cells of 6.5 m around the robot's cell) and may
    // exceed the 64 a chunk holds: the preparation wave walks the nine bucket ranges 64 entries at a time and hands
    // the marching threads one chunk of <= 64 neighbours per barrier pair (see the chunk loop below).
    // The nine ranges are ONE list to it: lanes 0..8 fetch "their" cell's range in the same memory round trip, a prefix sum
    // over those lanes numbers the entries, and a batch of 64 takes entries off.. off + 63 of that list whichever cells they
    // belong to.  (Rounds 2-3 walked the cells one after the other -- range, entry, pose, head: four dependent round trips
    // per cell, 36 per workgroup, and a workgroup lived 25 us whatever else the chip was doing:
    // profiles/r04_o_slice_sweep.txt.  Now it is five.)
    int big_off = 0;                   // enumeration state of the preparation wave (wave-uniform): entries consumed so far
    auto big_chunk = [&]() {
        const int icx = hash_cell_coord(x, kLidarCell), icy = hash_cell_coord(y, kLidarCell);
        for (int b = pl; b < e.B; b += kWave) nbmask[b] = 0ull;
        int cell_start = 0, cell_count = 0;
        if (pl < 9) {
            const uint32_t h = hash_cell(icx + pl % 3 - 1, icy + pl / 3 - 1, world) & (uint32_t)e.bw_lmask;
            cell_start = global_load<int>(e.bw_lstart, h * 4u);
            cell_count = global_load<int>(e.bw_lstart, h * 4u + 4u) - cell_start;
        }
        int cell_end = cell_count;         // inclusive prefix sum over lanes 0..8 (lanes >= 9 hold zeros)
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const int up = __shfl_up(cell_end, d, kWave);
            if (pl >= d) cell_end += up;
        }
        const int total = __shfl(cell_end, 8, kWave);
        int cnt = 0;
        while (big_off < total) {
            const int entry = big_off + pl;
            int q = 0;                     // the cell entry falls into: the number of cells ending at or before it
#pragma unroll
            for (int t = 0; t < 8; ++t) q += __shfl(cell_end, t, kWave) <= entry ? 1 : 0;
            const bool valid = entry < total;          // then q <= 8
            q = valid ? q : 0;
            const int qx = icx + q % 3 - 1, qy = icy + q / 3 - 1;
            const int q_end = __shfl(cell_end, q, kWave), q_count = __shfl(cell_count, q, kWave);
            const int idx = __shfl(cell_start, q, kWave) + (entry - (q_end - q_count));
            const int j = valid ? global_load<int>(e.bw_lsorted, (uint32_t)idx * 4u) : -1;
            bool keep = false;
            float cxj = 0.0f, cyj = 0.0f;
            float4 chj = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int lo = 0, hi = -1;
            if (j >= 0 && j != n && j / R_ == world) {
                const PoseXY pj = pose_xy(j);
                cxj = pj.x;
                cyj = pj.y;
                // a bucket may hold other cells too (hash collisions) and the same bucket may serve two of the nine
                // cells: a robot counts only for the cell it really is in, so nobody is listed twice
                if (hash_cell_coord(cxj, kLidarCell) == qx && hash_cell_coord(cyj, kLidarCell) == qy) {
                    const float ddx = cxj - x, ddy = cyj - y;
                    if (ddx * ddx + ddy * ddy <= kLidarReach2) {
                        beam_interval_approx(ddx * c + ddy * s, ddy * c - ddx * s, e.B, e.beam_step, e.beam_inv_step, e.lidar_radius,
                                             e.lidar_near, CullHardwareOps{}, &lo, &hi);
                        keep = lo <= hi;
                        if (keep) chj = global_load<float4>(head_p, (uint32_t)j * 16u);
                    }
                }
            }
            const unsigned long long m = __ballot(keep);
            const int add = __popcll(m);
            if (cnt + add > kWave) break;          // this batch opens the next chunk
            if (keep) {
                const int idx2 = cnt + __popcll(m & ((1ull << pl) - 1ull));
                float olx, oly;         // the lidar's origin in the neighbour's frame: once per neighbour, not per beam
                ray_box_origin(x, y, cxj, cyj, chj.x, chj.y, &olx, &oly);
                nb[idx2] = make_float4(olx, oly, chj.x, chj.y);
                nbi[idx2] = make_int2(lo, hi);
            }
            cnt += add;
            big_off += kWave;
        }
        if (pl == 0) {
            *nb_count = MRCA_DBG(e, 1) ? 0 : cnt;
            *nb_more = big_off < total ? 1 : 0;
        }
        for (int k = 0; k < cnt; ++k) {
            const int2 iv = nbi[k];
            for (int b = iv.x + pl; b <= iv.y; b += kWave) mask_or(&nbmask[b], 1ull << k);
        }
    };
    MRCA_RSTAMP(1);     // robot record, beam table, neighbour candidate requested (debug flag 64: arrived)
    if (is_prep) {
      if constexpr (BIG) {
        big_chunk();
      } else {
        if constexpr (!PAIRS) {
            for (int b = pl; b < e.B; b += kWave) nbmask[b] = 0ull;
        }
        const float ddx = xj - x, ddy = yj - y;
        // conservative cull: a hit below 6 m needs the centre within 6 + circumradius(0.2907) m (fidelity mode: + one
        // raster-cell diagonal -- what is tested there are the robot's outline CELLS)
        // (kept: a candidate with a beam in its interval.  The length first and the test on it: one compare, and the ballot is it)
        int lo = 0, hi = -1, len = 0;
        if (cand && (ddx * ddx + ddy * ddy <= e.lidar_reach2)) {
            // (the cull at the hardware's accuracy, v_rsq_f32 and v_rcp_f32: a beam more or less at an interval's end)
            beam_interval_approx(ddx * c + ddy * s, ddy * c - ddx * s, e.B, e.beam_step, e.beam_inv_step, e.lidar_radius,
                                 e.lidar_near, CullHardwareOps{}, &lo, &hi);
            len = imax(hi - lo + 1, 0);
        }
        const bool keep = len > 0;
        const unsigned long long m = __ballot(keep);
        if constexpr (PAIRS) {
            // pair-major slab tests (slab_pair_locate, mrca_device.h): the kept neighbours' intervals laid end to end number the
            // (neighbour, beam) pairs, and neighbour k's record is (lo_k, start_k), the exclusive prefix sum of the lengths before
            // it.  The sum runs over the LANES -- a dropped candidate adds nothing, and the ballot's compaction keeps the lanes'
            // order -- as six v_add_u32_dpp (lane_scan_dpp: the sum lane_scan_step's six doubling steps give, without their six
            // round trips through the LDS crossbar).  The list's slots behind the kept ones hold the pad that ends the search, so
            // that it reads the starts eight at a time without a tail: EVERY lane stamps the pad on its own slot's start first, and
            // the kept lanes' records go over the first `kept` of them -- a wave's LDS instructions take effect in the order it
            // issues them -- instead of each dropped lane working out a slot behind the list.
            // (pl is the lane's number in its wave -- T is a multiple of 64 --: the kept lanes below it are v_mbcnt's count)
            const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const int end = lane_scan_dpp(len);
            nbi[pl].y = kSlabPairPad;
            if (pl == kWave - 1) {      // the last lane holds P, the number of pairs: it stores the list's length beside it
                nb_count[0] = MRCA_DBG(e, 1) ? 0 : __popcll(m);
                nb_count[2] = end;
            }
            if (keep) {
                float olx, oly;         // the lidar's origin in the neighbour's frame: once per neighbour, not per pair
                ray_box_origin(x, y, xj, yj, hj.x, hj.y, &olx, &oly);
                nb[below] = make_float4(olx, oly, hj.x, hj.y);
                nbi[below] = make_int2(lo, end - len);
            }
        } else {        // the raster lidar: beam-major, a mask of neighbours per beam
            if (keep) {
                const int idx = __popcll(m & ((1ull << pl) - 1ull));
                // the fidelity mode's closed form wants the neighbour's outline record
                nbo[idx] = oj;
                nbi[idx] = make_int2(lo, hi);
            }
            const int cnt0 = MRCA_DBG(e, 1) ? 0 : __popcll(m);
            if (pl == 0) *nb_count = cnt0;
            // scatter: bit k of nbmask[b] = "neighbour k can touch beam b".  ds_or_b64 without a return value: the wave
            // fires one per neighbour and moves on (as a read-modify-write every neighbour cost an LDS round trip, ~2 000
            // of the 5 600 ticks wave 0 spent preparing, profiles/r03/r03_k_ablate_raycast_phase_stamps.txt).
            for (int k = 0; k < cnt0; ++k) {
                const int2 iv = nbi[k];
                for (int b = iv.x + pl; b <= iv.y; b += kWave) mask_or(&nbmask[b], 1ull << k);
            }
        }
      }
    }
    MRCA_RSTAMP(2);     // wave 0: neighbour list and the pairs' starts (beam-major: the per-beam masks) built
    // --- the march: K beams per thread in lock step
    float dx[K], dy[K], rng[K];
    bool from_robot[K];        // the range is a return from another robot (ranger_return 0.5: LaserScan intensity 0)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        dx[k] = c * bc[k] - s * bs[k];
        dy[k] = s * bc[k] + c * bs[k];
        rng[k] = kRangeMax;
        from_robot[k] = false;
    }
    if (marches && !MRCA_DBG(e, 2)) {
        // (the origin's entry is the quadrant one of the head record; every later lookup reads the march's own array)
        const FreeRectField field{e.march_rect, e.g.width, e.g.height, e.free_rect_pitch, (uint32_t)e.march_shift,
                                  (uint32_t)e.march_major};
        MarchOrigin org;                      // once per robot: shared by all its beams
        org.fx = (x - e.g.x0) * e.g.inv_cell;
        org.fy = (y - e.g.y0) * e.g.inv_cell;
        org.ix0 = (int)floorf(org.fx);
        org.iy0 = (int)floorf(org.fy);
        org.v_lo = __float_as_uint(hd.z);
        org.v_hi = __float_as_uint(hd.w);
        // Big worlds are open worlds (scenario.circle_big: the map is a token patch at the origin, the robots stand
        // kilometres from it), and outside the map the field knows nothing: a ray crawls from cell to cell, one dependent
        // lookup of the zero border each -- 40 000 of the 54 000 ticks a workgroup of the 50 000-robot circle lived
        // (profiles/r04_t_bigworld_raycast_phases.txt), to return kRangeMax.  A robot whose 6 m cannot reach the map's
        // bounding box (two cells of slack for the roundings of fx / fy) has nothing to march through: every beam is
        // kRangeMax exactly as the march would return it.
        bool map_in_reach = true;
        if constexpr (BIG) {
            const float reach = kRangeMax * e.g.inv_cell + 2.0f;
            map_in_reach = org.fx + reach >= 0.0f && org.fx - reach <= (float)e.g.width && org.fy + reach >= 0.0f &&
                           org.fy - reach <= (float)e.g.height;
        }
        if (map_in_reach) {
            if constexpr (K == 1 || SEQ) {   // one ray at a time: the hand-tuned single-ray loop (57 vector instructions per jump)
#pragma unroll
                for (int k = 0; k < K; ++k) rng[k] = grid_march_skip(field, e.g, org, dx[k], dy[k], kRangeMax);
            } else {                         // K rays in lock step: K lookups in flight per wait
                grid_march_skip_n<K>(field, e.g, org, dx, dy, kRangeMax, rng);
            }
        }
    }
    MRCA_RSTAMP(3);     // this wave's beams marched
    if constexpr (PAIRS) {      // what the pairs' entry distances are merged into: behind the same barrier as the list
        if (marches) {
#pragma unroll
            for (int k = 0; k < K; ++k) rmin[tid + k * T] = __float_as_int(rng[k]);
        }
    }
    __syncthreads();  // neighbour list ready (the preparation wave built it while the others marched)
    MRCA_RSTAMP(4);     // through the barrier / past the flag
    if constexpr (!BIG) {
        if (!marches) return;  // the dedicated preparation wave is done (whole wave: the barrier below counts live waves)
    }
    if constexpr (PAIRS) {
        // (cnt and P are the workgroup's: on the scalar side, so that the search's trips and the branch around the second barrier
        // are uniform to the compiler too)
        const int cnt = __builtin_amdgcn_readfirstlane(nb_count[0]);
        if (cnt > 0) {
            const int P = __builtin_amdgcn_readfirstlane(nb_count[2]);
            // thread tid tests pairs tid, tid + T, ...: a wave whose lowest pair is behind the last one has no lane in the loop
            for (int p = tid; p < P; p += T) {
                const int q = slab_pair_locate(p, cnt, [&](int k) { return nbi[k].y; });
                const int2 iq = nbi[q];
                const float4 nbq = nb[q];
                const int b = slab_pair_beam(p, iq.x, iq.y);
                // the beam's direction as its owner formed it above: the same loads, the same separately rounded operations
                const float pc = global_load<float>(bcos_p, (uint32_t)b * 4u), ps = global_load<float>(bsin_p, (uint32_t)b * 4u);
                const float t = ray_box_local(nbq.x, nbq.y, c * pc - s * ps, s * pc + c * ps, nbq.z, nbq.w);
                // slab_pair_merge, as ds_min_i32 without a return value: nothing to wait for
                (void)__hip_atomic_fetch_min(&rmin[b], __float_as_int(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();      // every pair merged (the dedicated preparation wave has left: the barrier counts live waves)
            // r = min(marched, the t of every pair of the beam), and `r < marched` is the flag of the running minimum
            // `from_robot |= t < r; r = t < r ? t : r` over the same t in any order: that loop sets the flag at some t below the
            // minimum so far, which is never above marched -- so only if the least t is below marched; and the first t below
            // marched in its order finds the minimum so far still at marched, and sets it.  Neither is true of marched = -0.0.
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float r = __int_as_float(rmin[tid + k * T]);
                from_robot[k] = r < rng[k];
                rng[k] = r;
            }
        }
    } else {        // big worlds' chunks and the raster lidar: beam-major, each thread its beams' flagged neighbours
        for (;;) {
            const int cnt = *nb_count;
            const int more = BIG ? *nb_more : 0;
            if (marches) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int b = tid + k * T;
                    float r = rng[k];
                    unsigned long long m = cnt > 0 ? nbmask[b] : 0ull;
                    if constexpr (raster) {
                        // fidelity mode: the entry time of the first raster cell of each flagged neighbour's outline the beam's
                        // walk visits -- in closed form, the same times grid_march's walk over the raster would compare
                        if (m) {
                            const float fxr = x * e.raster_inv, fyr = y * e.raster_inv;
                            const int ixr = (int)floorf(fxr), iyr = (int)floorf(fyr);
                            const float tmax_c = kRangeMax * e.raster_inv;
                            const float inv_dx = dx[k] != 0.0f ? rcp_exact(dx[k]) : kInf;
                            const float inv_dy = dy[k] != 0.0f ? rcp_exact(dy[k]) : kInf;
                            // (the 4 x 4 form: an axis the ray never steps along gets origin -inf, see ray_outline_entry4)
                            const float fxe = dx[k] != 0.0f ? fxr : -kInf, fye = dy[k] != 0.0f ? fyr : -kInf;
                            const bool xpos = dx[k] > 0.0f, ypos = dy[k] > 0.0f;
                            do {
                                const int q = __ffsll((long long)m) - 1;
                                m &= m - 1;
                                const int4 oq = nbo[q];
                                const OutlineBits ob{oq.x, oq.y, (uint32_t)oq.z, (uint32_t)oq.w};
                                const float tc = RKW == 4
                                                     ? ray_outline_entry4(fxe, fye, ixr, iyr, xpos, ypos, inv_dx, inv_dy, ob)
                                                     : ray_outline_entry<RKW>(fxr, fyr, ixr, iyr, dx[k], dy[k], inv_dx, inv_dy, ob);
                                const float t = tc < tmax_c ? tc * e.raster_res : kInf;
                                from_robot[k] = from_robot[k] || t < r;
                                r = t < r ? t : r;
                            } while (m);
                        }
                    } else {
                        while (m) {
                            const int q = __ffsll((long long)m) - 1;
                            m &= m - 1;
                            const float4 nbq = nb[q];
                            const float t = ray_box_local(nbq.x, nbq.y, dx[k], dy[k], nbq.z, nbq.w);
                            from_robot[k] = from_robot[k] || t < r;
                            r = t < r ? t : r;
                        }
                    }
                    rng[k] = r;
                }
            }
            if (!more) break;
            __syncthreads();          // everybody is through with this chunk ...
            if (is_prep) big_chunk();
            __syncthreads();          // ... and the next one is ready
        }
    }
    if (!marches) return;
    MRCA_RSTAMP(5);     // neighbour slab tests done
    // --- the scan (stageros.cpp:479-516) goes into the ring slot behind the newest one -- ONE store stream: the
    //     observation x / 6 - 0.5 (stage_world1.py:140) and the deque order (ppo_stage1.py:59-60,87-89) are the readers'
    //     business (materialize_kernel).  Every thread stores its own beams -- lane l of a wave holds beam base + l, so
    //     each store instruction of a wave covers 256 contiguous bytes.
    {
        // (row = n x F fits 32 bits -- n < 2^24, F <= 8 --: one 32 x 32 -> 64 multiply per address instead of a 64 x 32 chain of ten)
        const uint32_t row = (uint32_t)n * (uint32_t)e.F;
        float* ring_row = e.scan_ring + (size_t)row * (uint32_t)e.B;
        const int words = e.B >> 6;
        unsigned long long* hit_row = e.hit_bits + (size_t)row * (uint32_t)words;
        int new_slot;
        bool fresh;
        uint32_t stores = 0u;     // TICKS: the slots a fresh tick of the launch stores (ring_rule)
        bool any = true;          // TICKS: this tick stores a slot at all (no later tick of the launch restarts the robot)
        if constexpr (TICKS) {
            // ring_rule in its parts.  What hangs on the flags, j and T alone is wave-uniform and the compiler leaves it on the
            // scalar unit: the two tests the branches below want there anyway and the mask of the ticks up to j, about eight instructions.
            // What hangs on the head stays on the vector unit, where the load left it -- an add, a wrap, and the slot goes into
            // the store's offset as it is --: a scalar instruction is priced at two vector ones (see above), and the head on the
            // scalar side would cost a v_readfirstlane_b32 and the offset's multiply there.  The launch's last tick leaves the
            // head behind itself: its `slot` (ring_rule's head for j = T - 1).  Only a restart wants the store mask.
            const uint32_t fresh_bits = (uint32_t)__ballot(fresh_byte != 0);
            const RingTicks u = ring_ticks(mt.T, fresh_bits, mt.j);
            new_slot = ring_wrap(ring_slot + u.stale_to_j, e.F);
            fresh = u.fresh;
            any = !u.later;
            if (fresh && any) stores = (uint32_t)__builtin_amdgcn_readfirstlane((int)ring_fresh_stores(e.F, new_slot, mt.T - 1 - mt.j));
        } else {
            new_slot = ring_slot + 1 == e.F ? 0 : ring_slot + 1;
            fresh = __builtin_amdgcn_readfirstlane((int)fresh_byte) != 0;
        }
        // (what each beam stores first, then ONE test of the store selection around the K beams' stores, and the K words of hit
        // bits under ONE lane mask behind the K rows: tested per beam, the compiler repeated the scalar compares and branches K
        // times and split a wave's row store in two around the word's)
        float rk[K];
        unsigned long long hmk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // (the range as the march returned it, the sign of a zero included: a beam that enters an occupied cell at boundary
            // time -0 -- a sensor exactly on the face of a wall, looking into it -- has range -0.0 in the oracle, and a caller that
            // compares scans bit for bit sees it here too.  The readers that normalise take |x|.)
            rk[k] = rng[k] < kRangeMax ? rng[k] : kRangeMax;
            // what the beam hit: one bit per beam beside the ring (MRCA_F_HIT_BITS), set = another robot.  stageros casts
            // Stage's return value to uint8 for LaserScan.intensities (stageros.cpp:506): 1 floorplan, 0 robot or miss.  A wave
            // holds 64 consecutive beams (T is a multiple of 64: product_ray_shift), so its ballot IS the row's word b >> 6.
            // (ABI 4-5 kept the flag in the range's sign bit: a reader that forgot |x| got negative ranges.)
            hmk[k] = __ballot(from_robot[k] && rng[k] < kRangeMax);
        }
        const bool word_lane = (tid & (kWave - 1)) == 0;
        {
            // (nontemporal stores: the launch does not read its rows again.  Measured A/B on one box, round 4: 21.7 us with
            // them, 22.9 us with plain stores (profiles/r04_g_ab_nontemporal_row_stores.txt) -- although FETCH_SIZE does not
            // move, 2502 vs 2504 KiB: what they relieve is the write path, not the free-rectangle field's residency)
            if (fresh) {     // deque([obs] * F), ppo_stage1.py:59-60: every slot, the head stays where it is
                for (int f = 0; f < e.F; ++f) {
                    if (TICKS && !((stores >> f) & 1u)) continue;       // a later tick of the launch writes this slot
#pragma unroll
                    for (int k = 0; k < K; ++k) global_store_nt(ring_row, (uint32_t)(f * e.B + tid + k * T) * 4u, rk[k]);
                    if (word_lane) {
#pragma unroll
                        for (int k = 0; k < K; ++k) global_store(hit_row, (uint32_t)(f * words + ((tid + k * T) >> 6)) * 8u, hmk[k]);
                    }
                }
            } else if (any) {
                // (TICKS: the slot is a vector register's, below 8 -- a 24-bit multiply, full rate)
                const uint32_t at = TICKS ? __umul24((uint32_t)new_slot, (uint32_t)e.B) : (uint32_t)(new_slot * e.B);
#pragma unroll
                for (int k = 0; k < K; ++k) global_store_nt(ring_row, (at + (uint32_t)(tid + k * T)) * 4u, rk[k]);
                if (word_lane) {
#pragma unroll
                    for (int k = 0; k < K; ++k) global_store(hit_row, ((at >> 6) + (uint32_t)((tid + k * T) >> 6)) * 8u, hmk[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int b = tid + k * T;
            const float r = rk[k];
            // lazy_obs = 0: the two reference-shaped views of this robot, formed here instead of by a materialize_kernel launch
            // behind every ray cast (get_laser_observation, stage_world1.py:127-141: the newest scan; the stack in deque order,
            // x / 6 - 0.5) -- the same numbers: norm_obs of the ring's rows, the older ones as earlier launches stored them.  The
            // launch uses 5 % of HBM: the 8 kB per robot ride along (131 -> ... M agent-steps/s for a reference-shaped caller).
            if (VIEWS && views) {
                const float nr = norm_obs(r);
                // (nontemporal like the ring row: the launch does not read them again)
                if (views & 1) global_store_nt(e.scan + (size_t)n * (uint32_t)e.B, (uint32_t)b * 4u, r);
                if (views & 2) {
                    float* dst = e.obs + (size_t)row * (uint32_t)e.B;      // (the robot's stack: workgroup-uniform)
                    if (fresh) {
                        for (int f = 0; f < e.F; ++f) global_store_nt(dst, (uint32_t)(f * e.B + b) * 4u, nr);
                    } else {
                        int slot = new_slot;
                        for (int f = 0; f < e.F - 1; ++f) {        // oldest first: the slot behind the newest, and on round the ring
                            slot = slot + 1 == e.F ? 0 : slot + 1;
                            const float older = global_load<float>(ring_row, (uint32_t)(slot * e.B + b) * 4u);
                            global_store_nt(dst, (uint32_t)(f * e.B + b) * 4u, norm_obs(fabsf(older)));
                        }
                        global_store_nt(dst, (uint32_t)((e.F - 1) * e.B + b) * 4u, nr);
                    }
                }
            }
        }
        if constexpr (TICKS) {
            if (tid == 0 && mt.j == mt.T - 1) global_store(mt.head_out, (uint32_t)n, (uint8_t)new_slot);
        } else {
            if (tid == 0 && !fresh) global_store(ring_head_p, (uint32_t)n, (uint8_t)new_slot);
        }
    }
    if (tid == 0 && (!TICKS || mt.j == mt.T - 1)) {  // get_local_goal (stage_world1.py:155-160)
        const float gx = global_load<float>(e.goal, (uint32_t)n * 8u) - x, gy = global_load<float>(e.goal, (uint32_t)n * 8u + 4u) - y;
        global_store(e.local_goal, (uint32_t)n * 8u, gx * c + gy * s);
        global_store(e.local_goal, (uint32_t)n * 8u + 4u, gy * c - gx * s);
    }
    MRCA_RSTAMP(6);     // stores issued (debug flag 64: acknowledged)
}

}  // namespace

}  // namespace mrca
