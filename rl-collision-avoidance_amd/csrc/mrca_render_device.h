// mrca_render_device.h -- the rules of the top-down renderer (mrca_render), stated once for the gfx950 kernels
// of mrca_render.hip and for a plain host build (tests/test_render_host.py drives the same functions through g++).
//
// Like mrca_device.h: every step is a separately rounded IEEE fp32 operation in a fixed order (-ffp-contract=off, correctly
// rounded division), so a NumPy float32 restatement gives the same bits and an image can be compared for EQUALITY.
// Everything is point-sampled at pixel centres; a pixel's value is the MAXIMUM of `layer << 24 | local robot index` over
// everything that covers it, so neither the order of the robots nor of the hardware's threads shows in the result.
#pragma once
#include "mrca_device.h"

namespace mrca {

// same layout as mrca_render_view (include/mrca_env.h)
struct RenderView {
    int32_t world;
    float cx, cy, m;    // centre of the image [m], metres per pixel
};

// enum mrca_render_layers
constexpr uint32_t kRenderMap = 1u, kRenderGoals = 2u, kRenderBodies = 4u, kRenderBeams = 8u;

// layers of the ID image, low to high: the higher one wins a pixel, inside a layer the higher robot index
constexpr uint32_t kLayerBackground = 0u, kLayerMap = 1u, kLayerGoal = 2u, kLayerBeamWall = 3u, kLayerBeamRobot = 4u,
                   kLayerBody = 5u, kLayerNose = 6u;
constexpr int kLayerShift = 24;
constexpr uint32_t kIndexMask = (1u << kLayerShift) - 1u;

constexpr float kGoalMark2 = 0.0625f;   // a goal is drawn as the disc of 0.25 m around MRCA_F_GOAL (squared radius)
constexpr float kGoalReach = 0.25f;
constexpr float kNoseU = 0.11f;         // the front quarter of the footprint (u >= 0.11 of +-0.22) is the nose
constexpr float kBodyReach = 0.30f;     // > the footprint's circumradius 0.2907: what a robot's pixel box is built around

// The image's frame in the world: x of the left edge, y of the TOP edge (row 0 is +y: the map's convention and Stage's GUI's).
struct RenderFrame {
    float x0, y1, m;
    int32_t W, H;
};

MRCA_HD RenderFrame render_frame(const RenderView& v, int W, int H) {
    RenderFrame f;
    f.x0 = v.cx - (0.5f * (float)W) * v.m;
    f.y1 = v.cy + (0.5f * (float)H) * v.m;
    f.m = v.m;
    f.W = W;
    f.H = H;
    return f;
}

MRCA_HD float pixel_x(const RenderFrame& f, int col) { return f.x0 + ((float)col + 0.5f) * f.m; }
MRCA_HD float pixel_y(const RenderFrame& f, int row) { return f.y1 - ((float)row + 0.5f) * f.m; }

// The pixel CONTAINING a point: the floor of the IEEE quotients.  false: outside the image (or not a number).
MRCA_HD bool pixel_of(const RenderFrame& f, float x, float y, int* col, int* row) {
    const float fc = floorf((x - f.x0) / f.m);
    const float fr = floorf((f.y1 - y) / f.m);
    if (!(fc >= 0.0f && fc < (float)f.W && fr >= 0.0f && fr < (float)f.H)) return false;
    *col = (int)fc;
    *row = (int)fr;
    return true;
}

// Conservative pixel box (inclusive, clipped to the image; empty: c1 < c0) of the disc of `reach` metres around a point:
// the box of the pixels containing the disc's extremes and ONE more pixel on every side, which covers the rounding of the
// quotients and of the pixel centres as long as a pixel is wider than a few ulps of the coordinates (a view zoomed in past
// that has no distinct pixel centres any more).
struct PixelBox {
    int32_t c0, c1, r0, r1;
    MRCA_HD int32_t width() const { return c1 - c0 + 1; }
    MRCA_HD int32_t count() const { return (c1 < c0 || r1 < r0) ? 0 : (c1 - c0 + 1) * (r1 - r0 + 1); }
};

MRCA_HD PixelBox pixel_box(const RenderFrame& f, float x, float y, float reach) {
    const float fc0 = floorf(((x - reach) - f.x0) / f.m) - 1.0f;
    const float fc1 = floorf(((x + reach) - f.x0) / f.m) + 1.0f;
    const float fr0 = floorf((f.y1 - (y + reach)) / f.m) - 1.0f;
    const float fr1 = floorf((f.y1 - (y - reach)) / f.m) + 1.0f;
    PixelBox b{0, -1, 0, -1};
    // (a comparison with a NaN is false: a robot without a finite pose has an empty box)
    if (!(fc1 >= 0.0f && fc0 <= (float)(f.W - 1) && fr1 >= 0.0f && fr0 <= (float)(f.H - 1))) return b;
    b.c0 = (int32_t)fmaxf(fc0, 0.0f);
    b.c1 = (int32_t)fminf(fc1, (float)(f.W - 1));
    b.r0 = (int32_t)fmaxf(fr0, 0.0f);
    b.r1 = (int32_t)fminf(fr1, (float)(f.H - 1));
    return b;
}

// ---- the inside tests, all at a pixel centre (wx, wy)

// layer 1: the map cell under the point is occupied; cells outside the grid are free
MRCA_HD bool render_map_at(const GridGeom& g, const uint32_t* bits, float wx, float wy) {
    const float fx = floorf((wx - g.x0) * g.inv_cell);
    const float fy = floorf((wy - g.y0) * g.inv_cell);
    if (!(fx >= 0.0f && fx < (float)g.width && fy >= 0.0f && fy < (float)g.height)) return false;
    const int ix = (int)fx, iy = (int)fy;
    return (bits[(uint32_t)(iy * g.wpr + (ix >> 5))] >> (ix & 31)) & 1u;
}

// layers 5 / 6 (0: outside): the 0.44 x 0.38 footprint in the robot's frame, (s, c) = the head record's sine and cosine
MRCA_HD uint32_t render_body_at(float wx, float wy, float px, float py, float s, float c) {
    const float dx = wx - px, dy = wy - py;
    const float u = dx * c + dy * s;
    const float v = dy * c - dx * s;
    if (!(fabsf(u) <= kHalfLen && fabsf(v) <= kHalfWid)) return 0u;
    return u >= kNoseU ? kLayerNose : kLayerBody;
}

// layer 2: within 0.25 m of the goal
MRCA_HD bool render_goal_at(float wx, float wy, float gx, float gy) {
    const float dx = wx - gx, dy = wy - gy;
    return dx * dx + dy * dy <= kGoalMark2;
}

MRCA_HD uint32_t render_id(uint32_t layer, uint32_t index) { return layer << kLayerShift | index; }

// ---- the SCATTER form: what ONE robot contributes to the ID image of one view.  `put(pixel, id)` takes the maximum into
// pixel row * W + col (atomicMax in the kernel, a plain max on the host); lanes lane, lane + lanes, ... share the work.
template <class Put>
MRCA_HD void render_splat_disc(const RenderFrame& f, float x, float y, float reach, bool body, float s, float c, uint32_t index,
                               int lane, int lanes, Put& put) {
    const PixelBox b = pixel_box(f, x, y, reach);
    const int n = b.count(), bw = b.width();
    for (int k = lane; k < n; k += lanes) {
        const int row = b.r0 + k / bw, col = b.c0 + k % bw;
        const float wx = pixel_x(f, col), wy = pixel_y(f, row);
        const uint32_t layer = body ? render_body_at(wx, wy, x, y, s, c) : (render_goal_at(wx, wy, x, y) ? kLayerGoal : 0u);
        if (layer) put(row * f.W + col, render_id(layer, index));
    }
    // ... and always the pixel containing the point itself: a zoomed-out view of a giant circle still shows every robot
    int col, row;
    if (lane == 0 && pixel_of(f, x, y, &col, &row)) put(row * f.W + col, render_id(body ? kLayerBody : kLayerGoal, index));
}

template <class Put>
MRCA_HD void render_splat_robot(const RenderFrame& f, uint32_t layers, float px, float py, float s, float c, float gx, float gy,
                                uint32_t index, int lane, int lanes, Put& put) {
    if (layers & kRenderGoals) render_splat_disc(f, gx, gy, kGoalReach, false, 0.0f, 0.0f, index, lane, lanes, put);
    if (layers & kRenderBodies) render_splat_disc(f, px, py, kBodyReach, true, s, c, index, lane, lanes, put);
}

// layers 3 / 4: the end of one beam of the newest scan, pose + range * dir with dir formed as the ray cast forms it
// (mrca_raycast_body.h: dx = c * bc - s * bs, dy = s * bc + c * bs); a beam without a return (range 6.0) marks nothing
template <class Put>
MRCA_HD void render_splat_beam(const RenderFrame& f, float px, float py, float s, float c, float bc, float bs, float range,
                               bool hit_robot, uint32_t index, Put& put) {
    if (!(range < kRangeMax)) return;
    const float dx = c * bc - s * bs;
    const float dy = s * bc + c * bs;
    int col, row;
    if (pixel_of(f, px + range * dx, py + range * dy, &col, &row))
        put(row * f.W + col, render_id(hit_robot ? kLayerBeamRobot : kLayerBeamWall, index));
}

// ---- resolve: ID image + trail -> RGB8, packed r | g << 8 | b << 16.  The palette:
constexpr uint32_t kRgbBackground = 0xFFFFFFu;   // white, as Stage's GUI
constexpr uint32_t kRgbMap = 0x202020u;          // near black walls
constexpr uint32_t kRgbTrail = 0xC8C8C8u;        // light grey, only where nothing else is
constexpr uint32_t kRgbBeamWall = 0x00A5FFu;     // (255, 165, 0) orange
constexpr uint32_t kRgbBeamRobot = 0xD300D3u;    // (211, 0, 211) magenta
constexpr uint32_t kRgbCrashed = 0x0000DCu;      // (220, 0, 0) red
constexpr uint32_t kRgbReached = 0x00AA00u;      // (0, 170, 0) green

// the 16 hues of goals and bodies, by local index % 16 (r | g << 8 | b << 16)
MRCA_HD uint32_t render_hue(uint32_t k) {
    switch (k & 15u) {
        case 0: return 0xB4771Fu;    // ( 31, 119, 180)
        case 1: return 0x0E7FFFu;    // (255, 127,  14)
        case 2: return 0x8A5A17u;    // ( 23,  90, 138)
        case 3: return 0xBD6794u;    // (148, 103, 189)
        case 4: return 0x4B568Cu;    // (140,  86,  75)
        case 5: return 0xC277E3u;    // (227, 119, 194)
        case 6: return 0x7F7F7Fu;    // (127, 127, 127)
        case 7: return 0x22BDBCu;    // (188, 189,  34)
        case 8: return 0xCFBE17u;    // ( 23, 190, 207)
        case 9: return 0x9C4A39u;    // ( 57,  74, 156)
        case 10: return 0x31798Cu;   // (140, 121,  49)
        case 11: return 0x6B9E63u;   // ( 99, 158, 107)
        case 12: return 0x94397Bu;   // (123,  57, 148)
        case 13: return 0x4AB5E7u;   // (231, 181,  74)
        case 14: return 0xA55194u;   // (148,  81, 165)
        default: return 0x84845Au;   // ( 90, 132, 132)
    }
}

// per channel (c + 255) / 2: a goal's tint of its robot's hue;  c / 2: the nose's shade;  c / 4 + 144: a robot that is not live
MRCA_HD uint32_t rgb_tint(uint32_t c) { return ((c & 0xFEFEFEu) >> 1) + 0x7F7F7Fu + (c & 0x010101u); }
MRCA_HD uint32_t rgb_shade(uint32_t c) { return (c & 0xFEFEFEu) >> 1; }
MRCA_HD uint32_t rgb_dim(uint32_t c) { return ((c & 0xFCFCFCu) >> 2) + 0x909090u; }

// crashed / first_result / live: the robot's MRCA_F_CRASHED, MRCA_F_FIRST_RESULT, MRCA_F_LIVE (read for layers 5 and 6 only)
MRCA_HD uint32_t render_rgb(uint32_t id, uint32_t trail, uint32_t crashed, uint32_t first_result, uint32_t live) {
    const uint32_t layer = id >> kLayerShift, index = id & kIndexMask;
    switch (layer) {
        case kLayerBackground: return trail ? kRgbTrail : kRgbBackground;
        case kLayerMap: return kRgbMap;
        case kLayerGoal: return rgb_tint(render_hue(index));
        case kLayerBeamWall: return kRgbBeamWall;
        case kLayerBeamRobot: return kRgbBeamRobot;
        default: {
            uint32_t c = render_hue(index);
            if (crashed) c = kRgbCrashed;
            else if (first_result == 1u) c = kRgbReached;     // MRCA_RESULT_REACH
            else if (!live) c = rgb_dim(c);
            return layer == kLayerNose ? rgb_shade(c) : c;
        }
    }
}

}  // namespace mrca
