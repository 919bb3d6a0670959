// mrca_ray_shape.h -- which instantiation of the ray cast a launch runs and with what geometry, decided in one place: the
// beams a marching thread owns, the outline window of the raster lidar, the workgroup's size and its LDS.  Integers and one
// float, no HIP and no allocation: launch_raycast (mrca_kernels.hip), launch_raycast_ticks (mrca_raycast_ticks.hip) and
// mrca_abi.hip take the shape from here, tests/test_ray_shape_host.py compiles this header for the host and checks every shape
// a config or a profiling knob can select.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mrca_device.h"

namespace mrca {

// Launch shape of the ray cast, measured (profiles/r02/r02_c_ablation_launch_shapes.txt, 4096 / 8228 robots, HIP events):
//   2 beams per thread one after the other, first wave prepares the neighbours   28.1 / 33.7 us   <- product
//   1 beam per thread (512 threads), first wave prepares                           31.6 / 41.1 us
//   2 beams per thread in lock step (two lookups in flight), first wave prepares   34.7 / 37.9 us
//   the same three with a dedicated fifth preparation wave                          31.5-37.8 / 39.9-48.5 us
// i.e. neither more lookups in flight per thread nor taking the preparation off the marching waves pays: the
// lock-step loop costs 62 instead of 54 VALU instructions per jump and keeps finished rays idling, the extra
// wave costs a resident workgroup per CU.
// Worlds of more than 64 robots (the chunked neighbour lists of the big-world path), one circle of 50 000, PROFILING build
// (profiles/r04_m_slice_probe*.txt; full launch / one rank's slice of 6 250 robots):
//   4 beams per thread one after the other (2 waves per workgroup, 4096 workgroups resident)   445 /  77 us   <- product
//   2 beams per thread one after the other                                                      536 /  88 us
//   2 / 4 beams per thread in lock step (rounds 2-3)                                      548, 578 / 88, 94 us
//   1 beam per thread                                                                           844 / 133 us
//
// log2 of the beams a marching thread of the ray cast owns (EnvView::ray_shift): 2 per thread, 4 in worlds of more than 64
// robots -- as long as that leaves the workgroup two whole wavefronts or more
// (the marching threads of a workgroup are whole wavefronts -- beams >> shift is a multiple of 64: a wave's ballot is one word of
// MRCA_F_HIT_BITS)
inline int32_t product_ray_shift(int32_t beams, int32_t big) {
    if (big && (beams >> 2) >= 128 && (beams >> 2) % 64 == 0) return 2;
    return (beams >= 256 && (beams >> 1) % 64 == 0) ? 1 : 0;
}

// EnvView::raster_kw: the ray cast tests 4 x 4 cells of a neighbour's outline window where that covers every outline (Stage's
// 0.2 m), else 8 x 8.  raster_inv = 1 / collision_raster, 0 without a raster
inline int raster_window(float raster_inv) { return (raster_inv > 0.0f && outline_span(raster_inv) <= 4) ? 4 : 8; }

// the profiling build's beams-per-thread knob (mrca_set_debug_flags): whole marching wavefronts, at most 4 beams per thread --
// and, what the inline condition this replaces left to the launch to refuse, a workgroup of at most 1024 threads: 1024 beams at
// one per thread leave no room for the dedicated preparation wave
inline bool ray_knob_ok(int beams, int shift, bool prep_wave) {
    if (shift < 0 || shift > 2) return false;
    const int threads = beams >> shift;
    return threads >= 64 && threads % 64 == 0 && threads >= (beams >> 2) && threads + (prep_wave ? 64 : 0) <= 1024;
}

struct RayShape {
    int k;              // beams per marching thread: 1, 2 or 4
    bool big, seq;      // the big-world kernel; a thread's beams one after the other (false: in lock step, or k = 1)
    int rkw;            // the raster lidar's outline window, 4 or 8; 0: exact rectangles
    int threads;        // of a workgroup
    size_t lds_bytes;   // of a workgroup
};

// The shape for `beams` beams per robot.  big, raster_inv, raster_kw, ray_shift: the EnvView's; sequential, prep_wave: its
// ray_sequential and ray_prep_wave (1 and 0 in the product; the profiling build's knobs set all three).
inline RayShape ray_shape(int beams, bool big, float raster_inv, int raster_kw, int ray_shift, bool sequential, bool prep_wave) {
    RayShape s{};
    s.big = big;
    const bool raster = !big && raster_inv > 0.0f;
    if (raster) {
        // Fidelity mode is compiled in the product's shapes only: 1 beam per thread, or 2 one after the other, the first wave
        // preparing.  So a ray_shift of 2 launches the two-beam kernel, and the lock-step and preparation-wave knobs are ignored.
        s.k = ray_shift == 0 ? 1 : 2;
        s.seq = s.k == 2;
        s.rkw = raster_kw <= 4 ? 4 : 8;
        s.threads = beams >> (ray_shift == 0 ? 0 : 1);
    } else {
        s.k = ray_shift == 0 ? 1 : ray_shift == 1 ? 2 : 4;      // (a ray_shift beyond 2 never passes ray_knob_ok)
        s.seq = s.k > 1 && sequential;                          // one beam per thread has no order to choose
        s.rkw = 0;
        s.threads = (beams >> ray_shift) + (prep_wave ? 64 : 0);        // the dedicated preparation wave is a wave more
    }
    // per neighbour of the list (at most a wavefront's 64) a float4 and an int2, 16 bytes of counters, 8 bytes per beam; in
    // fidelity mode also the neighbours' outline records (OutlineBits, 16 bytes) -- mrca_kernels.hip asserts the sizes
    s.lds_bytes = 64 * (16 + 8) + 16 + (size_t)beams * 8 + (raster ? 64 * 16 : 0);
    return s;
}

// (K, BIG, SEQ, RKW) of a shape as compile-time constants: the leading template arguments of raycast_kernel, and without BIG of
// raycast_ticks_kernel
template <int K_, bool BIG_, bool SEQ_, int RKW_>
struct RayVariant {
    static constexpr int K = K_, RKW = RKW_;
    static constexpr bool BIG = BIG_, SEQ = SEQ_;
};

// f(RayVariant<...>{}) for the shape's variant: exactly the 14 combinations the library instantiates --
// exact rectangles and big worlds: 1, 2 one after the other, 2 in lock step, 4 one after the other, 4 in lock step each;
// the raster lidar: (1 | 2 one after the other) x (window of 4 | 8)
template <bool BIG, class F>
inline void with_plain_ray_variant(const RayShape& s, F&& f) {
    if (s.k == 1) f(RayVariant<1, BIG, false, 0>{});
    else if (s.k == 2 && s.seq) f(RayVariant<2, BIG, true, 0>{});
    else if (s.k == 2) f(RayVariant<2, BIG, false, 0>{});
    else if (s.seq) f(RayVariant<4, BIG, true, 0>{});
    else f(RayVariant<4, BIG, false, 0>{});
}
template <int RKW, class F>
inline void with_raster_ray_variant(const RayShape& s, F&& f) {
    if (s.k == 1) f(RayVariant<1, false, false, RKW>{});
    else f(RayVariant<2, false, true, RKW>{});
}
template <class F>
inline void with_ray_variant(const RayShape& s, F&& f) {
    if (s.rkw == 4) with_raster_ray_variant<4>(s, f);
    else if (s.rkw) with_raster_ray_variant<8>(s, f);
    else if (s.big) with_plain_ray_variant<true>(s, f);
    else with_plain_ray_variant<false>(s, f);
}

}  // namespace mrca
