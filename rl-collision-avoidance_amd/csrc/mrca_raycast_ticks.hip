// mrca_raycast_ticks.hip -- the ray casts of several consecutive ticks of one world range in ONE launch (mrca_step_many's
// run-ahead schedule).
//
// Inside a run-ahead pass the ray casts of ticks k, k + 1, k + 2 do not depend on each other: each reads its own slot of the
// move ring (pose, head record, goal, fresh flag, outline) and they meet only in the scan ring's slot bookkeeping, which
// ring_rule (mrca_device.h) settles without any workgroup reading what another one of the launch writes.  A launch of T ticks
// is a grid of (robots of the range) x T workgroups, tick-major: a tick's workgroups are dispatched before the next tick's, and
// within a tick the block -> robot map is the single-tick kernel's (workgroup (b, j) has linear id j x robots + b: the same
// XCD as block b of a single-tick launch whenever the map uses XCDs at all, robots % 8 == 0).  Workgroup (b, j) runs
// raycast_body for its robot against tick j's slot.  What a launch of several residency rounds buys: its later rounds start
// as workgroups of the earlier ones retire, not behind a launch boundary.
//
// A translation unit and a kernel of its own, so that the single-tick raycast_kernel carries none of this (the project's rule
// for the VIEWS and raster paths too).  Never big worlds, never the lazy_obs = 0 epilogue (it reads rows earlier ticks stored).
#include "mrca_kernels.h"

#include <assert.h>
#include <hip/hip_ext.h>

#include "mrca_raycast_body.h"

namespace mrca {

namespace {

// The kernel's arguments behind the 14 leading dwords: RayTicksIn with the fresh flags as the base the kernel addresses them
// from (RayTick::fresh_lo) instead of their offset in a slot -- the same 40 bytes.
struct TicksIn {
    const float4* env_head;
    const uint8_t* head_in;
    uint8_t* head_out;
    const uint8_t* fresh_lo;
    uint32_t off_goal, off_outline;
#if defined(MRCA_PROFILING)
    unsigned long long* launch_stamps;
    int32_t launch_slot;
#endif
};

// The leading 14 dwords (preloaded into SGPRs) are what the prologue needs first: the launch's range, where tick j's pose and
// head record are, the beam table, the env's own pose; the env's head record -- the last tick's second load -- comes with the
// rest.  `ticks`: T | env_tick << 8 | lo_tick << 16 | ring_last << 24 (RayTick).  104 bytes of arguments (a launch costs the
// host more from 128 bytes on, tools/launch_cost_probe.hip).
template <int K, bool SEQ, int RKW>
__global__ __launch_bounds__(1024, (RKW == 4 ? 8 : 1)) void raycast_ticks_kernel(int ray_first, int ray_count, int R_, uint32_t ticks,
                                                       const char* __restrict__ slot0, int stride, uint32_t off_head,
                                                       const float* __restrict__ bcos_p, const float* __restrict__ bsin_p,
                                                       const float* __restrict__ env_pose, const EnvView* __restrict__ view_p,
                                                       TicksIn in) {
    EnvView e = *view_p;        // (the env's view from device memory: its pose / head / goal / fresh / outline are slot 0's)
    const int T = ticks & 0xff, j = blockIdx.y;
    const int env_tick = (ticks >> 8) & 0xff;
    const bool own = j == env_tick;                      // workgroup-uniform: this tick reads the env's own fields
    const char* slot = slot0 + (long long)j * stride;
    const float* pose_p = own ? env_pose : reinterpret_cast<const float*>(slot);
    const float4* head_p = own ? in.env_head : reinterpret_cast<const float4*>(slot + off_head);
    if (!own) {
        e.goal = reinterpret_cast<float*>(const_cast<char*>(slot + in.off_goal));
        e.outline = reinterpret_cast<OutlineBits*>(const_cast<char*>(slot + in.off_outline));
    }
    e.pose = const_cast<float*>(pose_p);
    e.head = const_cast<float4*>(head_p);
    const RayTick mt{j, T, in.fresh_lo, stride, (int)((ticks >> 16) & 0xff), (int)(ticks >> 24), env_tick, in.head_in, in.head_out};
#if defined(MRCA_PROFILING)
    e.launch_stamps = in.launch_stamps;
    e.launch_slot = in.launch_slot;
#endif
    MRCA_LAUNCH_BEGIN(e);
    raycast_body<K, false, SEQ, RKW, false, true>(0, ray_first, ray_count, R_, pose_p, head_p, bcos_p, bsin_p, nullptr, e, 0, mt);
    MRCA_LAUNCH_END(e);
}

}  // namespace

void launch_raycast_ticks(const EnvView& e, const RayTicks& t, hipStream_t s) {
    if (e.ray_count <= 0 || t.ticks <= 0) return;
    const RayShape shape = ray_shape(e);
    assert(!shape.big);
    // The fresh flags of the launch's ticks that read ring slots, addressed from the lowest of them (RayTick::fresh_lo): every
    // offset the kernel forms, (t - lo_tick) * stride + n, is below (ticks - 1) * |stride| + N, which mrca_create holds below
    // 2^32 for every launch of several ticks it allows.
    assert(t.ticks >= 2 && t.ticks <= 8);
    const int ring_last = t.ticks - 1 - (t.last_is_env ? 1 : 0), lo_tick = t.stride < 0 ? ring_last : 0;
    assert((unsigned long long)ring_last * (unsigned long long)(t.stride < 0 ? -(long long)t.stride : (long long)t.stride) +
               (unsigned long long)(e.ray_first + e.ray_count) <= 0xffffffffull);
    const uint32_t ticks = (uint32_t)t.ticks | (t.last_is_env ? (uint32_t)t.ticks - 1u : 0xffu) << 8 | (uint32_t)lo_tick << 16 | (uint32_t)ring_last << 24;
    TicksIn in{};
    in.env_head = e.head;
    in.head_in = t.in.head_in;
    in.head_out = t.in.head_out;
    in.fresh_lo = reinterpret_cast<const uint8_t*>(t.slot0) + t.in.off_fresh + (long long)lo_tick * t.stride;
    in.off_goal = t.in.off_goal;
    in.off_outline = t.in.off_outline;
#if defined(MRCA_PROFILING)
    in.launch_stamps = t.in.launch_stamps;
    in.launch_slot = t.in.launch_slot;
#endif
    static_assert(sizeof(TicksIn) <= sizeof(RayTicksIn), "the ray cast of several ticks: no more than 104 bytes of arguments");
    with_ray_variant(shape, [&](auto v) {
        using V = decltype(v);
        hipLaunchKernelGGL((raycast_ticks_kernel<V::K, V::SEQ, V::RKW>), dim3(e.ray_count, t.ticks), dim3(shape.threads),
                           shape.lds_bytes, s, e.ray_first, e.ray_count, e.R, ticks, t.slot0, t.stride, t.off_head, e.beam_cos,
                           e.beam_sin, e.pose, e.dev, in);
    });
}

}  // namespace mrca
