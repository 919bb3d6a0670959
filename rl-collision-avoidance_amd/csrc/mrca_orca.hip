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
#include "mrca_orca.h"

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

__global__ __launch_bounds__(kBlock) void orca_kernel(const OrcaArgs a, const uint8_t* __restrict__ mask, float* __restrict__ actions,
                                                      float* __restrict__ vel) {
    const int lane = threadIdx.x & (kWave - 1);
    const int n = blockIdx.x * kRobotsPerBlock + (threadIdx.x >> 6);
    if (n >= a.N) return;                    // (wave-uniform, like every branch around a shuffle below)
    if (mask && !mask[n]) return;
    const OrcaParams& q = a.p;
    const int world = n / a.R;
    const int base = world * a.R, local = n - base;

    // ---- every lane j < R: robot j of the world (its own robot among them)
    const int j = lane < a.R ? lane : local;
    const float jx = a.pose[3 * (size_t)(base + j)], jy = a.pose[3 * (size_t)(base + j) + 1];
    const float4 jh = a.head[base + j];      // (sin, cos, ...)
    const float jsp = a.speed_gt[2 * (size_t)(base + j)];
    const float jvx = jsp * jh.y, jvy = jsp * jh.x;
    const float px = __shfl(jx, local), py = __shfl(jy, local);
    const float s = __shfl(jh.x, local), c = __shfl(jh.y, local);
    const float vx = __shfl(jvx, local), vy = __shfl(jvy, local);

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
    const float sec_r = __shfl(best_r, (4 * lane) & (kWave - 1));
    const int sec_b = __shfl(best_b, (4 * lane) & (kWave - 1));

    // ---- the neighbours: rank among the candidates by (dist2, index), then lane 16 + rank fetches its neighbour
    const float ddx = jx - px, ddy = jy - py;
    const float d2 = dot2(ddx, ddy, ddx, ddy);
    const bool cand = lane < a.R && lane != local && d2 < q.neighbor_dist * q.neighbor_dist;
    const unsigned long long cands = __ballot(cand);
    int rank = 0;
    for (unsigned long long m = cands; m; m &= m - 1) {
        const int o = __ffsll((long long)m) - 1;
        rank += orca_key_before(__shfl(d2, o), o, d2, lane) ? 1 : 0;
    }
    int src = -1;
    for (unsigned long long m = __ballot(cand && rank < q.max_neighbors); m; m &= m - 1) {
        const int o = __ffsll((long long)m) - 1;
        if (lane == kOrcaSectors + __shfl(rank, o)) src = o;
    }
    const int from = src < 0 ? 0 : src;
    const float nbx = __shfl(jx, from), nby = __shfl(jy, from), nvx = __shfl(jvx, from), nvy = __shfl(jvy, from);

    // ---- one constraint per lane
    bool valid;
    float rpx = 0.0f, rpy = 0.0f, rvx = vx, rvy = vy, R, inv_t, resp;
    if (lane < kOrcaSectors) {
        valid = sec_b != 0x7fffffff;
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
    const int short_at = lp2_wave(line, valid, lane, q.max_speed, ox, oy, false, &rx, &ry);
    if (short_at < kWave) {                  // LP3: static lines stay hard, robot lines are relaxed evenly
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
            if (lane >= kOrcaSectors) pvalid = valid && lane < i && orca_project(li, line, &pl);
            float tx, ty;
            if (lp2_wave(pl, pvalid, lane, q.max_speed, -li.dy, li.dx, true, &tx, &ty) == kWave) {
                rx = tx;
                ry = ty;
            }
            distance = orca_violation(li, rx, ry);
        }
    }

    if (lane == 0) {
        float v, w;
        orca_command(rx, ry, s, c, q.max_speed, q.k_omega, &v, &w);
        *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(v, w);
        if (vel) {
            vel[2 * (size_t)n] = rx;
            vel[2 * (size_t)n + 1] = ry;
        }
    }
}

}  // namespace

void launch_orca(const EnvView& e, const OrcaParams& p, const uint8_t* mask, float* actions, float* vel, hipStream_t s) {
    OrcaArgs a;
    a.N = e.N; a.R = e.R; a.B = e.B; a.F = e.F;
    a.key0 = e.key0; a.key1 = e.key1;
    a.pose = e.pose; a.head = e.head; a.speed_gt = e.speed_gt; a.goal = e.goal;
    a.scan_ring = e.scan_ring; a.ring_head = e.ring_head; a.hit_bits = e.hit_bits;
    a.beam_cos = e.beam_cos; a.beam_sin = e.beam_sin;
    a.p = p;
    hipLaunchKernelGGL(orca_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, a, mask, actions, vel);
}

}  // namespace mrca
