// mrca_dwa.hip -- the DWA baseline controller (mrca_dwa_actions): one launch, one WAVEFRONT per robot.
// The rule is mrca_dwa_device.h's; what is decided here is who computes what.
//
// The scan row is cut into 64 sectors and lane s IS sector s: it reads its beams / 64 consecutive ranges and keeps the nearest
// one, so the sector minimum needs no step across lanes.  The 64 obstacle points go to LDS (512 B per wave, 2 KiB per
// workgroup).  Then the lanes change roles: the nv * nw candidates are dealt to them, c = lane, lane + 64, ..., and every lane
// rolls its candidate out against the points, which stand packed at the front of the rows (a robot in the open tests few of
// the 64 slots; the minimum does not depend on the order) -- the reads of the points are same-address (broadcast) reads, no
// bank conflict and no v_readlane per point (a scalar instruction costs this chip twice a vector one).  The
// winner is a wave maximum over the key (score, ~c): a total order, so it cannot show which lane held which candidate.
// A wave's LDS rows are written and read by that wave alone: no workgroup barrier (waves leave early on the mask), only the
// wavefront-scope fence that keeps the compiler from moving the reads above the writes.
// No atomics, no scratch, no global writes except actions / choice / score.
#include "mrca_dwa.h"

namespace mrca {

namespace {

struct DwaArgs {
    int32_t N, B, F;
    const float* local_goal;
    const float* speed;
    const float* scan_ring;
    const uint8_t* ring_head;
    const float* beam_cos;
    const float* beam_sin;
    DwaParams p;
};

constexpr int kBlock = 256;
constexpr int kRobotsPerBlock = kBlock / kWave;

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        v = t > v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void dwa_kernel(const DwaArgs a, const uint8_t* __restrict__ mask, float* __restrict__ actions,
                                                     int32_t* __restrict__ choice, float* __restrict__ score) {
    __shared__ float pts_x[kRobotsPerBlock][kDwaSectors];
    __shared__ float pts_y[kRobotsPerBlock][kDwaSectors];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x * kRobotsPerBlock + wave;
    if (n >= a.N) return;                    // (wave-uniform, like every branch around a shuffle below)
    if (mask && !mask[n]) return;
    const DwaParams& q = a.p;

    const DwaRobot r = dwa_robot_begin(q, a.local_goal[2 * (size_t)n], a.local_goal[2 * (size_t)n + 1], a.speed[2 * (size_t)n],
                                       a.speed[2 * (size_t)n + 1]);
    unsigned long long best = 0ull;
    if (!r.at_goal) {
        // ---- the scan row: lane s holds beams [s * per, (s + 1) * per), sector s
        const int per = a.B >> 6;
        const size_t slot = (size_t)n * (size_t)a.F + a.ring_head[n];
        const float* ranges = a.scan_ring + slot * (size_t)a.B;
        float br;
        const int bb = dwa_sector_min(ranges, lane * per, per, dwa_range_cut(q.obst_dist), &br);
        float x = kInf, y = 0.0f;
        if (bb >= 0) dwa_point(br, a.beam_cos[bb], a.beam_sin[bb], &x, &y);
        // the points packed to the front of the wave's LDS rows, the empty slots ((+inf, 0)) behind them: every slot is written
        const unsigned long long have = __ballot(bb >= 0);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int n_points = __popcll(have);
        const int slot_of = bb >= 0 ? __popcll(have & below) : n_points + __popcll(~have & below);
        pts_x[wave][slot_of] = x;
        pts_y[wave][slot_of] = y;
        const int n_slots = (n_points + 3) & ~3;         // (whole groups of four: dwa_candidate takes four at a time)
        const bool any_point = n_points > 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- the candidates, 64 at a time
        const int nc = q.nv * q.nw;
        for (int base = 0; base < nc; base += kWave) {
            const int c = base + lane;
            if (c < nc) {
                const unsigned long long key = dwa_candidate(q, r, c, pts_x[wave], pts_y[wave], n_slots, any_point, nullptr, nullptr);
                best = key > best ? key : best;
            }
        }
        best = wave_max_key(best);
    }

    if (lane == 0) {
        float cmd[2], sc;
        int ch;
        dwa_result(q, r, best, cmd, &ch, &sc);
        *reinterpret_cast<float2*>(actions + 2 * (size_t)n) = make_float2(cmd[0], cmd[1]);
        if (choice) choice[n] = ch;
        if (score) score[n] = sc;
    }
}

}  // namespace

void launch_dwa(const EnvView& e, const DwaParams& p, const float* goal, const uint8_t* mask, float* actions, int32_t* choice, float* score,
                hipStream_t s) {
    DwaArgs a;
    a.N = e.N; a.B = e.B; a.F = e.F;
    a.local_goal = goal ? goal : e.local_goal; a.speed = e.speed;
    a.scan_ring = e.scan_ring; a.ring_head = e.ring_head;
    a.beam_cos = e.beam_cos; a.beam_sin = e.beam_sin;
    a.p = p;
    hipLaunchKernelGGL(dwa_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, a, mask, actions, choice, score);
}

}  // namespace mrca
