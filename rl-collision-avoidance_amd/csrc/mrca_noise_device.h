// mrca_noise_device.h -- the rule of the lidar noise model (mrca_scan_noise), stated once for the gfx950 kernel
// of mrca_noise.hip and for a plain host build (tests/test_scan_noise_host.py drives the same functions through g++).
//
// The ray cast leaves exact ranges in the scan ring.  This rule turns the row a cast has just stored into what a real ranger
// would have reported: range noise with a constant and a range-proportional part, a quantised read-out, and beams that
// report nothing although something was there (dropout).  Per beam b of robot n with clean range r:
//
//   U  = philox4x32_10(n, episode[n], b, (T[n] << 2) | 2, key)      the key and the robot word are the reset sampler's
//   r >= 6            the beam returned nothing: it stays as it is, and its hit bit stays clear
//   z  = (((u01(U.x) + u01(U.y)) + u01(U.z)) - 1.5) * 2             a THREE-UNIFORM IRWIN-HALL deviate, NOT a Gaussian:
//                                                                   mean 0, variance 1, support [-3, 3), kurtosis 2.6 -- no
//                                                                   transcendental, so nothing hangs on a libm
//   r1 = r + (sigma_const + sigma_prop * r) * z                     if one of the sigmas is > 0, else r1 = r to the bit
//   r2 = quantum * rintf(r1 / quantum)                              if quantum > 0 (ties to even), else r2 = r1
//   !(r2 > 0) -> +0.0;   r2 >= 6 -> 6.0 and the beam's hit bit is cleared (a set bit never stands on a 6.0)
//   u01(U.w) < dropout -> 6.0, the bit cleared, whatever the above gave
//
// The reset sampler's streams use counter word 3 = 0 (pose) and 1 (goal): a word whose low two bits are 2 meets neither.
// The draw hangs on (seed, robot, episode, T, beam) and on nothing else -- not on the launch shape, the mask or the order
// of calls.
//
// The transform is IN PLACE and NOT IDEMPOTENT: it is applied ONCE per cast, to the row that cast stored.  A second call
// behind the same cast draws the same numbers and adds them again.  (With all four params 0 the rule changes nothing but a
// range of -0.0, which leaves as +0.0; mrca_scan_noise launches nothing then.)
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 + - * / or a comparison, in a fixed order
// (-ffp-contract=off, correctly rounded division); rintf is round-to-nearest-even on both sides.  A NumPy float32
// restatement (tests/noise_ref.py) gives the same bits.
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_scan_noise_params (include/mrca_env.h)
struct ScanNoiseParams {
    float sigma_const, sigma_prop, dropout, quantum;
};

constexpr uint32_t kStreamNoise = 2u;     // the low two bits of counter word 3 (kStreamPose = 0, kStreamGoal = 1 are whole words)

MRCA_HD uint32_t noise_counter_word(int32_t t) { return ((uint32_t)t << 2) | kStreamNoise; }

MRCA_HD U4 noise_draw(uint32_t gid, int32_t episode, int beam, int32_t t, uint32_t k0, uint32_t k1) {
    return philox4x32_10(gid, (uint32_t)episode, (uint32_t)beam, noise_counter_word(t), k0, k1);
}

// unit variance, zero mean, |z| <= 3: the sum of three uniforms, centred and scaled (its variance is 3 / 12)
MRCA_HD float noise_deviate(const U4& u) { return (((u01(u.x) + u01(u.y)) + u01(u.z)) - 1.5f) * 2.0f; }

struct NoisyBeam {
    float range;
    bool clear;       // the beam's bit in MRCA_F_HIT_BITS must be cleared
};

// the rule for one beam, the draw given
MRCA_HD NoisyBeam noise_beam(const ScanNoiseParams& p, float r, const U4& u) {
    if (r >= kRangeMax) return NoisyBeam{r, false};
    const float r1 = (p.sigma_const > 0.0f || p.sigma_prop > 0.0f) ? r + (p.sigma_const + p.sigma_prop * r) * noise_deviate(u) : r;
    float r2 = p.quantum > 0.0f ? p.quantum * rintf(r1 / p.quantum) : r1;
    if (!(r2 > 0.0f)) r2 = 0.0f;
    bool clear = false;
    if (r2 >= kRangeMax) {
        r2 = kRangeMax;
        clear = true;
    }
    if (u01(u.w) < p.dropout) {
        r2 = kRangeMax;
        clear = true;
    }
    return NoisyBeam{r2, clear};
}

// ---- the rule as plain loops.  The kernel runs the same pieces with a beam per lane and a ballot per hit word.

// one row of `beams` ranges (a multiple of 64) and its beams / 64 hit words, in place
MRCA_HD void noise_row(const ScanNoiseParams& p, uint32_t gid, int32_t episode, int32_t t, uint32_t k0, uint32_t k1, int beams,
                       float* row, unsigned long long* hits) {
    for (int b = 0; b < beams; ++b) {
        const NoisyBeam nb = noise_beam(p, row[b], noise_draw(gid, episode, b, t, k0, k1));
        row[b] = nb.range;
        if (nb.clear) hits[b >> 6] &= ~(1ull << (b & 63));
    }
}

}  // namespace mrca
