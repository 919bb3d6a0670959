// mrca_orca.hip -- the ORCA baseline controller (mrca_orca_actions): one launch, one WAVEFRONT per robot.
// The rule is mrca_orca_device.h's; what is decided here is who computes what.
//
// A robot has at most 16 static constraints (one per sector of its scan) and 48 robot constraints: 64 lines, one per lane.
// Lanes 0..15 own the sectors, lane 16 + r the neighbour of rank r; a lane without a line is marked invalid and the order of
// the valid lanes is the contract's order, so nothing is compacted.  The linear programs walk the lines in order (a scalar
// loop: "the first lane that violates" is a ballot and a count of trailing zeros) and clip a line by ALL earlier ones at once:
// each lane clips by its own line, the interval's ends are a wave maximum / minimum, the two ways to fail are ballots.
// A lane per robot would serialise about 26 x 26 clips per lane and could not read the scan row coalesced.
// No atomics, no LDS: every exchange between lanes is a shuffle.
//
// Who a robot's neighbours are is the one part that depends on the world's size.  Up to 64 robots: every lane j < R is robot j
// (orca_kernel<false>).  More (mrca_orca_actions_any, orca_kernel<true>): the candidates come from the env's lidar hash, 64 at a time,
// and the best max_neighbors keys stay in registers (hashed_neighbours); from "lane 16 + r holds neighbour r" on it is the
// same code.
//
// The NH-ORCA baseline (mrca_nhorca_actions) is the same body with a second flag, orca_kernel<BIG, true>: two
// heading lines in lanes 0 and 1 and the solve run twice (mrca_nhorca_device.h).
#include "mrca_orca.h"

#include <type_traits>

namespace mrca {

namespace {

struct OrcaArgs {
    int32_t N, R, B, F;
    uint32_t key0, key1;
    const float* pose;
    const float4* head;
    const float* speed_gt;
    const float* goal;
    const float* scan_ring;
    const uint8_t* ring_head;
    const unsigned long long* hit_bits;
    const float* beam_cos;
    const float* beam_sin;
    OrcaParams p;
};

constexpr int kBlock = 256;
constexpr int kRobotsPerBlock = kBlock / kWave;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const float t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const float t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}

__device__ __forceinline__ OrcaLine line_of_lane(const OrcaLine& l, int k) {
    return OrcaLine{__shfl(l.px, k), __shfl(l.py, k), __shfl(l.dx, k), __shfl(l.dy, k)};
}

__device__ __forceinline__ unsigned long long lanes_from(int k) { return k >= kWave ? 0ull : ~0ull << k; }

// LP2 over the wave's lines (`line` / `valid` per lane): -> 64 when every line holds, else the lane of the first line that
// could not be satisfied.  Every argument but line / valid is wave-uniform, and so are the result and (rx, ry).
__device__ int lp2_wave(const OrcaLine& line, bool valid, int lane, float max_speed, float ox, float oy, bool dir_opt, float* rx,
                        float* ry) {
    orca_lp2_start(ox, oy, max_speed, dir_opt, rx, ry);
    unsigned long long consider = ~0ull;
    for (;;) {
        const unsigned long long viol = __ballot(valid && orca_violation(line, *rx, *ry) > 0.0f) & consider;
        if (!viol) return kWave;
        const int k = __ffsll((long long)viol) - 1;
        const OrcaLine lk = line_of_lane(line, k);
        float tl, tr;
        if (!orca_lp1_begin(lk, max_speed, &tl, &tr)) return k;
        bool ok = true;
        if (valid && lane < k) ok = orca_lp1_clip(lk, line, &tl, &tr);
        tl = wave_max(tl);
        tr = wave_min(tr);
        if (__ballot(!ok)) return k;
        float nx, ny;
        if (!orca_lp1_end(lk, tl, tr, ox, oy, dir_opt, &nx, &ny)) return k;
        // (the +0 of orca_lp1_end made the ends, and with them the point, the same bits in every lane)
        *rx = nx;
        *ry = ny;
        consider = lanes_from(k + 1);
    }
}

// Worlds of more than kOrcaMaxRobots robots: the lidar hash of the env (EnvView's bw_lstart / bw_lsorted / bw_lmask, built over
// the CURRENT poses) and g = orca_rings(neighbor_dist)
struct OrcaHash {
    const int32_t* lstart;
    const int32_t* lsorted;
    int32_t lmask, rings;
};

using Key = unsigned long long;

// forward permute: lane dest[l] receives v of lane l (the highest such l where several send to one lane); a lane nobody sends
// to receives kOrcaNoKey -- the complement travels, and what ds_permute leaves in a lane without a sender is 0.
// Every lane of the wave takes part.
__device__ __forceinline__ Key push_key(Key v, int dest) {
    const Key t = ~v;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)(uint32_t)t);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)(uint32_t)(t >> 32));
    return ~(((Key)hi << 32) | lo);
}

// The kept neighbours of robot n (at (px, py) in `world`) of a world of ANY size, from the lidar hash: on return lane r < the
// count holds the key of the neighbour of rank r (orca_key: index in the env), every other lane kOrcaNoKey.  What
// orca_neighbours_hashed (mrca_orca_device.h) states, with the wave doing the work:
//   lanes 0 .. (2g+1)^2 - 1 fetch the bucket range of "their" cell in one round trip and a prefix sum over the wave makes the
//   ranges ONE list (the ray cast's big_chunk does this for nine lanes);
//   the list streams through the wave 64 entries at a time: a lane finds the cell its entry belongs to (a binary search over
//   the prefix sums), loads the candidate's pose once, applies the cell / world / self / distance filters and forms its key;
//   the best max_neighbors keys so far stay in registers, sorted, one per lane.  A chunk merges into them BY RANK: a key's
//   place in the union is the number of keys before it (the chunk's by a loop over its candidates, the kept ones by a binary
//   search since they are sorted), and every key is pushed to the lane of its rank.  Keys are totally ordered (distinct
//   indices), so ranks are distinct and the order in which the hash lists the robots cannot show.  A chunk key that is not
//   before the worst kept key of a full list is dropped before it is ranked: in a jam most chunks add little.
__device__ __forceinline__ Key hashed_neighbours(const OrcaArgs& a, const OrcaHash hsh, int lane, int n, int world, float px, float py) {
    const OrcaParams& q = a.p;
    const int g = hsh.rings, side = 2 * g + 1, K = q.max_neighbors;
    const int icx = hash_cell_coord(px, kLidarCell), icy = hash_cell_coord(py, kLidarCell);
    int cell_start = 0, cell_count = 0;
    if (lane < side * side) {                // (at most 49 cells)
        const uint32_t h = hash_cell(icx + lane % side - g, icy + lane / side - g, world) & (uint32_t)hsh.lmask;
        cell_start = hsh.lstart[h];
        cell_count = hsh.lstart[h + 1] - cell_start;
    }
    int cell_end = cell_count;               // inclusive prefix sum (lanes without a cell hold the total)
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(cell_end, d, kWave);
        if (lane >= d) cell_end += up;
    }
    const int total = __shfl(cell_end, kWave - 1);
    const float nd2 = q.neighbor_dist * q.neighbor_dist;
    Key best = kOrcaNoKey;
    for (int off = 0; off < total && K > 0; off += kWave) {
        const int entry = off + lane;
        const bool in = entry < total;
        int cq = 0;                          // the entry's cell: the number of cells that end at or before it (< 64 while `in`)
#pragma unroll
        for (int step = kWave / 2; step > 0; step >>= 1) {
            const int end = __shfl(cell_end, cq + step - 1);
            if (end <= entry) cq += step;
        }
        cq = in ? cq : 0;
        const int qx = icx + cq % side - g, qy = icy + cq / side - g;
        const int idx = __shfl(cell_start, cq) + (entry - (__shfl(cell_end, cq) - __shfl(cell_count, cq)));
        int j = -1;
        if (in && (unsigned)idx < (unsigned)a.N) j = hsh.lsorted[idx];
        Key key = kOrcaNoKey;
        if ((unsigned)j < (unsigned)a.N && j != n && j / a.R == world) {
            const float xj = a.pose[3 * (size_t)j], yj = a.pose[3 * (size_t)j + 1];
            // a bucket may hold other cells and other worlds, and may serve two of the cells asked for: a robot counts for
            // the cell it really is in
            if (hash_cell_coord(xj, kLidarCell) == qx && hash_cell_coord(yj, kLidarCell) == qy) {
                const float d2 = orca_dist2(px, py, xj, yj);
                if (d2 < nd2) key = orca_key(d2, j);
            }
        }
        const Key worst = __shfl(best, K - 1);           // kOrcaNoKey while the list is not full
        const unsigned long long cands = __ballot(key < worst);
        if (!cands) continue;
        if (!(key < worst)) key = kOrcaNoKey;
        int before_best = 0, before_key = 0;             // chunk keys before this lane's kept key / before its chunk key
        for (unsigned long long m = cands; m; m &= m - 1) {
            const Key ck = __shfl(key, __ffsll((long long)m) - 1);
            before_best += ck < best ? 1 : 0;
            before_key += ck < key ? 1 : 0;
        }
        int pos = 0;                                     // kept keys before this lane's chunk key
#pragma unroll
        for (int step = kWave / 2; step > 0; step >>= 1) {
            const Key bk = __shfl(best, pos + step - 1);
            if (bk < key) pos += step;
        }
        const int to_best = lane + before_best, to_key = pos + before_key;
        // lane 63 is nobody's place (K <= 48): what falls off the list, and every lane without a key, is sent there
        const Key kept = push_key(best, best != kOrcaNoKey && to_best < K ? to_best : kWave - 1);
        const Key came = push_key(key, key != kOrcaNoKey && to_key < K ? to_key : kWave - 1);
        best = kept < came ? kept : came;                // (a place receives one key: ranks are distinct)
        if (lane >= K) best = kOrcaNoKey;
    }
    return best;
}

struct OrcaNoHash {};

// NH-ORCA (mrca_nhorca_device.h): what nhorca_derive gave (the grown radius travels as a.p.radius), the tracking time, and where
// the modes go (or nullptr)
struct NhArgs {
    float sm, cm, u_cap, track_time;
    int32_t* mode;
};

struct OrcaNoNh {};

// The solve over the wave's lines: LP2, and where it falls short LP3, in which the lanes below `hard` stay hard and the robot
// lines are relaxed evenly.  (rx, ry) is wave-uniform.
__device__ __forceinline__ void solve_wave(const OrcaLine& line, bool valid, int lane, int hard, float max_speed, float ox, float oy,
                                           float* rx_out, float* ry_out) {
    float rx, ry;
    const int short_at = lp2_wave(line, valid, lane, max_speed, ox, oy, false, &rx, &ry);
    if (short_at < kWave) {
        float distance = 0.0f;
        unsigned long long consider = lanes_from(short_at);
        for (;;) {
            const unsigned long long m = __ballot(valid && orca_violation(line, rx, ry) > distance) & consider;
            if (!m) break;
            const int i = __ffsll((long long)m) - 1;
            consider = lanes_from(i + 1);
            const OrcaLine li = line_of_lane(line, i);
            OrcaLine pl = line;
            bool pvalid = valid;
            if (lane >= hard) pvalid = valid && lane < i && orca_project(li, line, &pl);
            float tx, ty;
            if (lp2_wave(pl, pvalid, lane, max_speed, -li.dy, li.dx, true, &tx, &ty) == kWave) {
                rx = tx;
                ry = ty;
            }
            distance = orca_violation(li, rx, ry);
        }
    }
    *rx_out = rx;
    *ry_out = ry;
}

// BIG: worlds of more than kOrcaMaxRobots robots (`hsh` is their lidar hash); otherwise `hsh` is empty and the kernel is, but for
// its name, the one that worlds of up to 64 robots have always run.
// NH: the NH-ORCA rule -- lanes 0 and 1 own the two heading lines, the sectors and the neighbours move up by two lanes (so
// max_neighbors <= kNhMaxNeighbors = 46: lane 63 stays the top-K merge's spare), and the solve runs twice: free (the heading lanes
// invalid, max_speed), then tracked (all lanes, u_cap).  Otherwise `nh` is empty and nothing of it is compiled.
template <bool BIG, bool NH>
__global__ __launch_bounds__(kBlock) void orca_kernel(const OrcaArgs a, const uint8_t* __restrict__ mask, float* __restrict__ actions,
                                                      float* __restrict__ vel, const std::conditional_t<BIG, OrcaHash, OrcaNoHash> hsh,
                                                      const std::conditional_t<NH, NhArgs, OrcaNoNh> nh) {
    constexpr int kFirst = NH ? kNhHeadingLines : 0;        // the lane of sector 0
    constexpr int kNb = kFirst + kOrcaSectors;              // the lane of the nearest neighbour
    const int lane = threadIdx.x & (kWave - 1);
    const int n = blockIdx.x * kRobotsPerBlock + (threadIdx.x >> 6);
    if (n >= a.N) return;                    // (wave-uniform, like every branch around a shuffle below)
    if (mask && !mask[n]) return;
    const OrcaParams& q = a.p;
    const int world = n / a.R;
    const int base = world * a.R, local = n - base;

    float jx = 0.0f, jy = 0.0f, jvx = 0.0f, jvy = 0.0f;
    float px, py, s, c, vx, vy;
    if constexpr (!BIG) {
        // ---- every lane j < R: robot j of the world (its own robot among them)
        const int j = lane < a.R ? lane : local;
        jx = a.pose[3 * (size_t)(base + j)];
        jy = a.pose[3 * (size_t)(base + j) + 1];
        const float4 jh = a.head[base + j];      // (sin, cos, ...)
        const float jsp = a.speed_gt[2 * (size_t)(base + j)];
        jvx = jsp * jh.y;
        jvy = jsp * jh.x;
        px = __shfl(jx, local);
        py = __shfl(jy, local);
        s = __shfl(jh.x, local);
        c = __shfl(jh.y, local);
        vx = __shfl(jvx, local);
        vy = __shfl(jvy, local);
    } else {
        // ---- the robot's own record, loaded directly (wave-uniform)
        px = a.pose[3 * (size_t)n];
        py = a.pose[3 * (size_t)n + 1];
        const float4 h = a.head[n];
        const float sp = a.speed_gt[2 * (size_t)n];
        s = h.x;
        c = h.y;
        vx = sp * h.y;
        vy = sp * h.x;
    }

    float ox, oy;
    orca_pref_velocity(q, (uint32_t)n, a.key0, a.key1, px, py, a.goal[2 * (size_t)n], a.goal[2 * (size_t)n + 1], &ox, &oy);

    // ---- the scan row: lane l holds beams [l * per, (l + 1) * per), a sector is four consecutive lanes
    const int per = a.B >> 6;
    const size_t slot = (size_t)n * (size_t)a.F + a.ring_head[n];
    const float* ranges = a.scan_ring + slot * (size_t)a.B;
    const unsigned long long* hits = a.hit_bits + slot * (size_t)per;
    float best_r = kInf;
    int best_b = 0x7fffffff;
    for (int k = 0; k < per; ++k) {          // ascending beams and a strict comparison: ties go to the lowest beam
        const int b = lane * per + k;
        const float r = ranges[b];
        const bool hit = (hits[b >> 6] >> (b & 63)) & 1ull;
        if (orca_beam_counts(r, hit, q.obst_dist) && orca_beam_before(r, b, best_r, best_b)) {
            best_r = r;
            best_b = b;
        }
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const float r = __shfl_xor(best_r, o);
        const int b = __shfl_xor(best_b, o);
        if (orca_beam_before(r, b, best_r, best_b)) {
            best_r = r;
            best_b = b;
        }
    }
    const float sec_r = __shfl(best_r, (4 * (lane - kFirst)) & (kWave - 1));
    const int sec_b = __shfl(best_b, (4 * (lane - kFirst)) & (kWave - 1));

    int src = -1;
    float nbx, nby, nvx, nvy;
    if constexpr (!BIG) {
        // ---- the neighbours: rank among the candidates by (dist2, index), then lane kNb + rank fetches its neighbour
        const float ddx = jx - px, ddy = jy - py;
        const float d2 = dot2(ddx, ddy, ddx, ddy);
        const bool cand = lane < a.R && lane != local && d2 < q.neighbor_dist * q.neighbor_dist;
        const unsigned long long cands = __ballot(cand);
        int rank = 0;
        for (unsigned long long m = cands; m; m &= m - 1) {
            const int o = __ffsll((long long)m) - 1;
            rank += orca_key_before(__shfl(d2, o), o, d2, lane) ? 1 : 0;
        }
        for (unsigned long long m = __ballot(cand && rank < q.max_neighbors); m; m &= m - 1) {
            const int o = __ffsll((long long)m) - 1;
            if (lane == kNb + __shfl(rank, o)) src = o;
        }
        const int from = src < 0 ? 0 : src;
        nbx = __shfl(jx, from);
        nby = __shfl(jy, from);
        nvx = __shfl(jvx, from);
        nvy = __shfl(jvy, from);
    } else {
        // ---- the neighbours from the lidar hash; lane kNb + rank takes the neighbour of that rank and loads its record once
        const Key best = hashed_neighbours(a, hsh, lane, n, world, px, py);
        const Key mine = __shfl(best, (lane - kNb) & (kWave - 1));
        if (lane >= kNb && mine != kOrcaNoKey) src = orca_key_index(mine);
        const int from = src < 0 ? n : src;
        nbx = a.pose[3 * (size_t)from];
        nby = a.pose[3 * (size_t)from + 1];
        const float4 h = a.head[from];
        const float sp = a.speed_gt[2 * (size_t)from];
        nvx = sp * h.y;
        nvy = sp * h.x;
    }

    // ---- one constraint per lane
    bool valid;
    float rpx = 0.0f, rpy = 0.0f, rvx = vx, rvy = vy, R, inv_t, resp;
    if (lane < kNb) {
        valid = lane >= kFirst && sec_b != 0x7fffffff;
        if (valid) orca_static_rel(sec_r, s, c, a.beam_cos[sec_b], a.beam_sin[sec_b], &rpx, &rpy);
        R = q.radius;
        inv_t = 1.0f / q.time_horizon_obst;
        resp = 1.0f;
    } else {
        valid = src >= 0;
        rpx = nbx - px;
        rpy = nby - py;
        rvx = vx - nvx;
        rvy = vy - nvy;
        R = 2.0f * q.radius;
        inv_t = 1.0f / q.time_horizon;
        resp = q.responsibility;
    }
    OrcaLine line{0.0f, 0.0f, 1.0f, 0.0f};
    if (valid) orca_constraint(rpx, rpy, rvx, rvy, vx, vy, R, inv_t, resp, &line);

    // ---- solve
    float rx, ry;
    if constexpr (!NH) {
        solve_wave(line, valid, lane, kNb, q.max_speed, ox, oy, &rx, &ry);
        if (lane == 0) {
            float v, w;
            orca_command(rx, ry, s, c, q.max_speed, q.k_omega, &v, &w);
            *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(v, w);
            if (vel) {
                vel[2 * (size_t)n] = rx;
                vel[2 * (size_t)n + 1] = ry;
            }
        }
    } else {
        // ---- the free solve decides what the tracked solve aims at; lanes 0 and 1 take the heading lines for the second
        float s1x, s1y;
        solve_wave(line, valid, lane, kNb, q.max_speed, ox, oy, &s1x, &s1y);
        float turn;
        const bool track = nhorca_aim(s1x, s1y, ox, oy, s, c, nh.cm, &turn);
        OrcaLine left, right;
        nhorca_heading_lines(s, c, nh.sm, nh.cm, &left, &right);
        if (lane < kFirst) {
            line = lane == 0 ? left : right;
            valid = true;
        }
        solve_wave(line, valid, lane, kNb, nh.u_cap, track ? ox : 0.0f, track ? oy : 0.0f, &rx, &ry);
        if (lane == 0) {
            float v, w;
            const int mode = nhorca_command(rx, ry, s, c, track, turn, q.max_speed, nh.track_time, &v, &w);
            *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(v, w);
            if (vel) {
                vel[2 * (size_t)n] = rx;
                vel[2 * (size_t)n + 1] = ry;
            }
            if (nh.mode) nh.mode[n] = mode;
        }
    }
}

OrcaArgs orca_args(const EnvView& e, const OrcaParams& p) {
    OrcaArgs a;
    a.N = e.N; a.R = e.R; a.B = e.B; a.F = e.F;
    a.key0 = e.key0; a.key1 = e.key1;
    a.pose = e.pose; a.head = e.head; a.speed_gt = e.speed_gt; a.goal = e.goal;
    a.scan_ring = e.scan_ring; a.ring_head = e.ring_head; a.hit_bits = e.hit_bits;
    a.beam_cos = e.beam_cos; a.beam_sin = e.beam_sin;
    a.p = p;
    return a;
}

}  // namespace

void launch_orca(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s) {
    const OrcaArgs a = orca_args(e, p);
    hipLaunchKernelGGL((orca_kernel<false, false>), dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, a, mask, actions,
                       vel, OrcaNoHash{}, OrcaNoNh{});
}

void launch_orca_big(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s) {
    const OrcaArgs a = orca_args(e, p);
    const OrcaHash hsh{e.bw_lstart, e.bw_lsorted, e.bw_lmask, orca_rings(p.neighbor_dist)};
    hipLaunchKernelGGL((orca_kernel<true, false>), dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, a, mask, actions,
                       vel, hsh, OrcaNoNh{});
}

void launch_nhorca(const EnvView& e, const NhOrcaParams& p, bool big, const uint8_t* mask, float* actions, float* vel, int32_t* mode,
                   hipStream_t s) {
    const NhOrcaDerived d = nhorca_derive(p);
    OrcaArgs a = orca_args(e, p.o);
    a.p.radius = d.radius;
    const NhArgs nh{d.sm, d.cm, d.u_cap, p.track_time, mode};
    const dim3 grid((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock);
    if (big) {
        const OrcaHash hsh{e.bw_lstart, e.bw_lsorted, e.bw_lmask, orca_rings(p.o.neighbor_dist)};
        hipLaunchKernelGGL((orca_kernel<true, true>), grid, dim3(kBlock), 0, s, a, mask, actions, vel, hsh, nh);
    } else {
        hipLaunchKernelGGL((orca_kernel<false, true>), grid, dim3(kBlock), 0, s, a, mask, actions, vel, OrcaNoHash{}, nh);
    }
}

}  // namespace mrca
