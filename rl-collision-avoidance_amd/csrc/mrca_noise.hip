// mrca_noise.hip -- the lidar noise model (mrca_scan_noise): one launch, one WAVEFRONT per robot.
// The rule is mrca_noise_device.h's; what is decided here is who computes what.
//
// In round k lane l owns beam 64 k + l: a round reads and writes 256 contiguous bytes of the row, draws one Philox block per
// lane, and the beams whose hit bit must go are ONE ballot -- hit word k of the row becomes old & ~ballot, stored by lane 0
// with an ordinary vector store.  What is the same for a robot (its head, fresh flag, T, episode) is loaded once and made
// wave-uniform.  A wave touches its own robot's rows only: no atomics, no LDS, no barrier, no scratch.
#include "mrca_noise.h"

namespace mrca {

namespace {

struct NoiseArgs {
    int32_t N, B, F, views;
    float* scan_ring;
    unsigned long long* hit_bits;
    float* scan;
    float* obs;
    const uint8_t* ring_head;
    const uint8_t* fresh;
    const int32_t* t;
    const int32_t* episode;
    uint32_t key0, key1;
    ScanNoiseParams p;
};

constexpr int kBlock = 256;
constexpr int kRobotsPerBlock = kBlock / kWave;

__global__ __launch_bounds__(kBlock) void scan_noise_kernel(const NoiseArgs a, const uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x * kRobotsPerBlock + wave;
    if (n >= a.N) return;                    // (wave-uniform, like every branch around the ballot below)
    if (mask && !mask[n]) return;
    const int head = __builtin_amdgcn_readfirstlane((int)a.ring_head[n]);
    if (head >= a.F) return;                 // (never in an env the library keeps: a head outside the ring must not become an address)
    const bool fresh = __builtin_amdgcn_readfirstlane((int)a.fresh[n]) != 0;
    const int32_t t = __builtin_amdgcn_readfirstlane(a.t[n]);
    const int32_t episode = __builtin_amdgcn_readfirstlane(a.episode[n]);

    const int B = a.B, F = a.F, words = a.B >> 6;
    const size_t row = (size_t)n * (size_t)F;
    float* ring = a.scan_ring + row * (size_t)B;                 // the robot's F rows
    unsigned long long* hits = a.hit_bits + row * (size_t)words; // ... and their words
    float* obs = a.obs + row * (size_t)B;
    float* scan = a.scan + (size_t)n * (size_t)B;
    // a fresh robot: every slot (deque([obs] * F), ppo_stage1.py:59-60); otherwise the newest one
    const int f0 = fresh ? 0 : head, f1 = fresh ? F : head + 1;

    for (int k = 0; k < words; ++k) {
        const int b = (k << 6) + lane;
        const NoisyBeam nb = noise_beam(a.p, ring[head * B + b], noise_draw((uint32_t)n, episode, b, t, a.key0, a.key1));
        const unsigned long long gone = __ballot(nb.clear);
        // (the slot loops are short -- F <= 8, one trip unless the robot is fresh -- and stay plain loops: vectorised, the word
        // loop of a one-word row grew two more loop nests and ten spilled SGPRs)
#pragma clang loop vectorize(disable) unroll(disable)
        for (int f = f0; f < f1; ++f) ring[f * B + b] = nb.range;
        if (lane == 0) {
            const unsigned long long w = hits[head * words + k] & ~gone;
#pragma clang loop vectorize(disable) unroll(disable)
            for (int f = f0; f < f1; ++f) hits[f * words + k] = w;
        }
        // lazy_obs = 0: the two views follow the ring (what the ray cast's epilogue wrote of this row, written again)
        if (a.views & 1) scan[b] = nb.range;
        if (a.views & 2) {
            const float nr = norm_obs(nb.range);                 // (the range is >= +0 here: no |x|)
#pragma clang loop vectorize(disable) unroll(disable)
            for (int f = fresh ? 0 : F - 1; f < F; ++f) obs[f * B + b] = nr;     // deque order: the newest frame is the last
        }
    }
}

}  // namespace

void launch_scan_noise(const EnvView& e, const ScanNoiseParams& p, const uint8_t* mask, int views, hipStream_t s) {
    NoiseArgs a;
    a.N = e.N; a.B = e.B; a.F = e.F; a.views = views;
    a.scan_ring = e.scan_ring; a.hit_bits = e.hit_bits; a.scan = e.scan; a.obs = e.obs;
    a.ring_head = e.ring_head; a.fresh = e.fresh; a.t = e.t; a.episode = e.episode;
    a.key0 = e.key0; a.key1 = e.key1;
    a.p = p;
    hipLaunchKernelGGL(scan_noise_kernel, dim3((e.N + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kBlock), 0, s, a, mask);
}

}  // namespace mrca
