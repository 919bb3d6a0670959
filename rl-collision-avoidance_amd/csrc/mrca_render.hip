// mrca_render.hip -- top-down views of worlds as ID images and RGB8 pictures (mrca_render): three launches per
// call.  The rules are mrca_render_device.h's; what is decided here is who computes what and how it reaches memory.
#include "mrca_render.h"

namespace mrca {

namespace {

// What the three kernels read, by value: the env's pointers they need and the views of this set of launches.
struct RenderArgs {
    int32_t W, H, R, B, F;
    uint32_t layers;
    GridGeom g;
    const uint32_t* map_bits;
    const float* pose;
    const float4* head;
    const float* goal;
    const float* scan_ring;
    const uint8_t* ring_head;
    const unsigned long long* hit_bits;
    const float* beam_cos;
    const float* beam_sin;
    const uint8_t* crashed;
    const uint8_t* first_result;
    const uint8_t* live;
    RenderView views[kRenderViewsPerLaunch];
};

constexpr int kBlock = 256;
constexpr int kRobotsPerBlock = kBlock / kWave;

// (a) clear + map: one thread per four consecutive pixels of a view (blockIdx.y), one 16-byte store where the image allows
// it.  Writes every pixel of ids: 4 B per pixel out, the bit-packed map (L2-resident) in.  Bound by its stores.
__global__ __launch_bounds__(kBlock) void render_clear_map_kernel(const RenderArgs a, uint32_t* __restrict__ ids, int vec) {
    const uint32_t hw = (uint32_t)a.W * (uint32_t)a.H;
    const uint32_t p0 = (blockIdx.x * (uint32_t)kBlock + threadIdx.x) * 4u;
    if (p0 >= hw) return;
    const RenderFrame f = render_frame(a.views[blockIdx.y], a.W, a.H);
    uint32_t* out = ids + (size_t)blockIdx.y * hw;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t p = p0 + k;
        v[k] = 0u;
        if ((a.layers & kRenderMap) && p < hw) {
            const int row = (int)(p / (uint32_t)a.W), col = (int)(p - (uint32_t)row * (uint32_t)a.W);
            if (render_map_at(a.g, a.map_bits, pixel_x(f, col), pixel_y(f, row))) v[k] = render_id(kLayerMap, 0u);
        }
    }
    if (vec) {      // (hw % 4 == 0 and a 16-byte aligned image: p0 + 3 < hw)
        *reinterpret_cast<uint4*>(out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < hw) out[p0 + k] = v[k];
    }
}

struct AtomicMaxPut {
    uint32_t* img;
    __device__ __forceinline__ void operator()(int pixel, uint32_t id) { atomicMax(img + pixel, id); }
};

// (b) splat: one WAVEFRONT per robot of a viewed world (blockIdx.y = view) -- work per robot, not per pixel x robot.  The
// wave's lanes share the robot's pixel boxes (goal, body) and its beams; a robot whose boxes miss the image runs no loop
// iteration at all (every bound is wave-uniform).  Integer atomicMax: the image does not depend on who comes first.
// Bound by latency (one dependent load chain per wave, then a few scattered atomics).
__global__ __launch_bounds__(kBlock) void render_splat_kernel(const RenderArgs a, uint32_t* __restrict__ ids,
                                                               uint32_t* __restrict__ trail) {
    const int lane = threadIdx.x & (kWave - 1);
    const int local = blockIdx.x * kRobotsPerBlock + (threadIdx.x >> 6);
    if (local >= a.R) return;
    const RenderView view = a.views[blockIdx.y];
    const RenderFrame f = render_frame(view, a.W, a.H);
    const size_t n = (size_t)view.world * (size_t)a.R + (size_t)local;
    const size_t image = (size_t)blockIdx.y * ((size_t)a.W * (size_t)a.H);
    const float px = a.pose[3 * n], py = a.pose[3 * n + 1];
    const float4 hd = a.head[n];      // (sin, cos, ...)
    AtomicMaxPut put{ids + image};
    render_splat_robot(f, a.layers, px, py, hd.x, hd.y, a.goal[2 * n], a.goal[2 * n + 1], (uint32_t)local, lane, kWave, put);
    if ((a.layers & kRenderBeams) && pixel_box(f, px, py, kRangeMax).count() > 0) {
        const size_t slot = n * (size_t)a.F + a.ring_head[n];
        const float* ranges = a.scan_ring + slot * (size_t)a.B;
        const unsigned long long* hits = a.hit_bits + slot * (size_t)(a.B >> 6);
        for (int b = lane; b < a.B; b += kWave)
            render_splat_beam(f, px, py, hd.x, hd.y, a.beam_cos[b], a.beam_sin[b], ranges[b], (hits[b >> 6] >> (b & 63)) & 1ull,
                              (uint32_t)local, put);
    }
    int col, row;
    if (trail && lane == 0 && pixel_of(f, px, py, &col, &row)) atomicMax(trail + image + (size_t)(row * a.W + col), (uint32_t)local + 1u);
}

// (c) resolve: one thread per four consecutive pixels of the whole [V,H,W] stack: 16 B (+ 16 B of trail) in, 12 B = three
// whole dwords of RGB out; the state bytes of a robot are read only under its body.  Bound by HBM traffic.
__global__ __launch_bounds__(kBlock) void render_resolve_kernel(const RenderArgs a, const uint32_t* __restrict__ ids,
                                                                 const uint32_t* __restrict__ trail, uint8_t* __restrict__ rgb,
                                                                 unsigned long long total, int vec) {
    const unsigned long long p0 = ((unsigned long long)blockIdx.x * kBlock + threadIdx.x) * 4ull;
    if (p0 >= total) return;
    const uint32_t hw = (uint32_t)a.W * (uint32_t)a.H;
    uint32_t id[4], tr[4] = {0u, 0u, 0u, 0u};
    const bool full = p0 + 4ull <= total;
    if (vec && full) {
        const uint4 q = *reinterpret_cast<const uint4*>(ids + p0);
        id[0] = q.x; id[1] = q.y; id[2] = q.z; id[3] = q.w;
        if (trail) {
            const uint4 t = *reinterpret_cast<const uint4*>(trail + p0);
            tr[0] = t.x; tr[1] = t.y; tr[2] = t.z; tr[3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            id[k] = p0 + k < total ? ids[p0 + k] : 0u;
            if (trail && p0 + k < total) tr[k] = trail[p0 + k];
        }
    }
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t crashed = 0u, first = 0u, live = 1u;
        const uint32_t index = id[k] & kIndexMask;
        if ((id[k] >> kLayerShift) >= kLayerBody && index < (uint32_t)a.R && p0 + k < total) {
            const uint32_t v = (uint32_t)((p0 + k) / hw);
            const size_t n = (size_t)a.views[v].world * (size_t)a.R + index;
            crashed = a.crashed[n];
            first = a.first_result[n];
            live = a.live[n];
        }
        c[k] = render_rgb(id[k], tr[k], crashed, first, live);
    }
    if (full) {     // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        uint32_t* out = reinterpret_cast<uint32_t*>(rgb + p0 * 3ull);
        out[0] = c[0] | c[1] << 24;
        out[1] = c[1] >> 8 | c[2] << 16;
        out[2] = c[2] >> 16 | c[3] << 8;
    } else {
        for (int k = 0; k < 4 && p0 + k < total; ++k) {
            uint8_t* o = rgb + (p0 + k) * 3ull;
            o[0] = (uint8_t)c[k];
            o[1] = (uint8_t)(c[k] >> 8);
            o[2] = (uint8_t)(c[k] >> 16);
        }
    }
}

}  // namespace

void launch_render(const EnvView& e, const RenderView* views, int num_views, int W, int H, uint32_t layers, uint32_t* ids,
                   uint32_t* trail, uint8_t* rgb, hipStream_t s) {
    RenderArgs a;
    a.W = W; a.H = H; a.R = e.R; a.B = e.B; a.F = e.F;
    a.layers = layers;
    a.g = e.g;
    a.map_bits = e.map_bits;
    a.pose = e.pose; a.head = e.head; a.goal = e.goal;
    a.scan_ring = e.scan_ring; a.ring_head = e.ring_head; a.hit_bits = e.hit_bits;
    a.beam_cos = e.beam_cos; a.beam_sin = e.beam_sin;
    a.crashed = e.crashed; a.first_result = e.first_result; a.live = e.live;
    const size_t hw = (size_t)W * (size_t)H;
    const unsigned quads = (unsigned)((hw + 3) / 4);
    for (int first = 0; first < num_views; first += kRenderViewsPerLaunch) {
        const int count = num_views - first < kRenderViewsPerLaunch ? num_views - first : kRenderViewsPerLaunch;
        for (int v = 0; v < kRenderViewsPerLaunch; ++v) a.views[v] = views[first + (v < count ? v : 0)];
        uint32_t* ids_v = ids + (size_t)first * hw;
        uint32_t* trail_v = trail ? trail + (size_t)first * hw : nullptr;
        const int vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(ids_v) % 16 == 0;
        hipLaunchKernelGGL(render_clear_map_kernel, dim3((quads + kBlock - 1) / kBlock, count), dim3(kBlock), 0, s, a, ids_v, vec);
        if ((layers & (kRenderGoals | kRenderBodies | kRenderBeams)) || trail_v)
            hipLaunchKernelGGL(render_splat_kernel, dim3((e.R + kRobotsPerBlock - 1) / kRobotsPerBlock, count), dim3(kBlock), 0, s, a,
                               ids_v, trail_v);
        if (rgb) {
            const unsigned long long total = (unsigned long long)count * hw;
            // the stack's pixels are contiguous across views: aligned 16-byte loads need only an aligned start
            const int vec_in = reinterpret_cast<uintptr_t>(ids_v) % 16 == 0 && (!trail_v || reinterpret_cast<uintptr_t>(trail_v) % 16 == 0);
            hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((total + 4ull * kBlock - 1) / (4ull * kBlock))), dim3(kBlock), 0, s, a,
                               ids_v, trail_v, rgb + (size_t)first * hw * 3, total, vec_in);
        }
    }
}

}  // namespace mrca
