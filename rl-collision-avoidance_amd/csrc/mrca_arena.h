// mrca_arena.h -- where an env's memory lies: the ONE list of the arena's parts (`parts`), and what is made from it -- the layout
// (make_layout), the binding of a view's pointers to an arena (bind) and the slot of mrca_step_many's run-ahead ring (make_slot,
// bind_slot).  Host-only arithmetic: no HIP call, no allocation; compiles with plain g++ (tests/test_arena_layout_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mrca_env.h"
#include "mrca_kernels.h"

namespace mrca {
namespace arena __attribute__((visibility("hidden"))) {

constexpr size_t kAlign = 256;      // every part begins on a granule of its own
constexpr size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// buckets of a big world's two hashes (robots_per_world > 64, else none): the first powers of two >= 4 N (collision hash: 2 N
// entries -- pose at tick start + provisional pose -- at a load factor <= 0.5) and >= 2 N (lidar hash)
struct Buckets { size_t collide, lidar; };
inline Buckets hash_buckets(const mrca_config& c) {
    Buckets b{0, 0};
    const size_t N = (size_t)c.num_worlds * c.robots_per_world;
    if (c.robots_per_world > 64) {
        for (b.collide = 1; b.collide < 4 * N;) b.collide <<= 1;
        for (b.lidar = 1; b.lidar < 2 * N;) b.lidar <<= 1;
    }
    return b;
}

// The arena's parts in the order they lie in: part(member of EnvView, bytes) for each.  The first MRCA_F_COUNT are the public
// fields in enum order (include/mrca_env.h).  A part that does not exist has 0 bytes: it takes no room, its pointer stays null.
template <class Part> void parts(const mrca_config& c, Part&& part) {
    const size_t R = c.robots_per_world, N = (size_t)c.num_worlds * R, B = c.beams, F = c.frames, mw = c.map_width, mh = c.map_height;
    const Buckets hash = hash_buckets(c);
    auto bw = [&](size_t bytes) { return R > 64 ? bytes : 0; };      // big worlds only
    part(&EnvView::pose, N * 3 * 4);
    part(&EnvView::speed, N * 2 * 4);
    part(&EnvView::speed_gt, N * 2 * 4);
    part(&EnvView::goal, N * 2 * 4);
    part(&EnvView::init_pose, N * 3 * 4);
    part(&EnvView::scan, N * B * 4);
    part(&EnvView::obs, N * F * B * 4);
    part(&EnvView::local_goal, N * 2 * 4);
    part(&EnvView::reward, N * 4);
    part(&EnvView::done, N);
    part(&EnvView::result, N);
    part(&EnvView::first_result, N);
    part(&EnvView::crashed, N);
    part(&EnvView::live, N);
    part(&EnvView::fresh, N);
    part(&EnvView::t, N * 4);
    part(&EnvView::episode, N * 4);
    part(&EnvView::prev_dist, N * 4);
    part(&EnvView::scan_ring, N * F * B * 4);
    part(&EnvView::ring_head, N);
    part(&EnvView::hit_bits, N * F * (B / 64) * 8);
    part(&EnvView::reset_mode, R * 4);
    part(&EnvView::goal_mode, R * 4);
    part(&EnvView::group_id, R * 4);
    part(&EnvView::init_table, R * 3 * 4);
    part(&EnvView::goal_table, R * 2 * 4);
    part(&EnvView::beam_cos, B * 4);
    part(&EnvView::beam_sin, B * 4);
    part(&EnvView::map_bits, mh * c.map_words_per_row * 4);
    part(&EnvView::free_rect, (mw + 2 * kFieldPadX) * (mh + 2 * kFieldPadY) * 4 * sizeof(uint16_t));
    part(&EnvView::cellfield, mw * mh);
    part(&EnvView::head, N * sizeof(float4));
    part(&EnvView::outline, c.collision_raster > 0.0f ? N * sizeof(OutlineBits) : 0);   // fidelity mode only
    part(&EnvView::bw_ticket, bw(4));
    part(&EnvView::bw_prov, bw(N * 2 * sizeof(float4)));
    part(&EnvView::bw_state, bw(N * 4));
    part(&EnvView::bw_chead, bw(hash.collide * 4));
    part(&EnvView::bw_cnext, bw(2 * N * 4));
    part(&EnvView::bw_lstart, bw((hash.lidar + 2) * 4));
    part(&EnvView::bw_lcount, bw((hash.lidar + 1) * 4));
    part(&EnvView::bw_lsorted, bw(N * 4));
    part(&EnvView::bw_lblock, bw((hash.lidar / 1024 + 2) * 4));
    part(&EnvView::bw_lcursor, bw((hash.lidar + 1) * 4));
    part(&EnvView::status, 4);
}

// the bytes of one part (a walk over the list: for construction, not for a launch)
template <class T> size_t part_bytes(const mrca_config& c, T EnvView::*member) {
    size_t found = 0;
    parts(c, [&](auto m, size_t bytes) {
        if constexpr (std::is_same_v<decltype(m), T EnvView::*>)
            if (m == member) found = bytes;
    });
    return found;
}

// offsets and bytes of the public fields (mrca_get_field), and the arena's size
struct Layout { size_t field_off[MRCA_F_COUNT], field_bytes[MRCA_F_COUNT], total; };
inline Layout make_layout(const mrca_config& c) {
    Layout L{};
    int i = 0;
    parts(c, [&](auto, size_t bytes) {
        if (i < MRCA_F_COUNT) L.field_off[i] = L.total, L.field_bytes[i] = bytes;
        ++i;
        L.total += align_up(bytes);
    });
    return L;
}

// v's pointers into the arena at `base` (null for a part that does not exist), and the two hash masks
inline void bind(const mrca_config& c, char* base, EnvView* v) {
    size_t off = 0;
    parts(c, [&](auto m, size_t bytes) {
        v->*m = bytes ? reinterpret_cast<std::remove_reference_t<decltype(v->*m)>>(base + off) : nullptr;
        off += align_up(bytes);
    });
    const Buckets hash = hash_buckets(c);
    v->bw_cmask = hash.collide ? (int32_t)(hash.collide - 1) : 0;
    v->bw_lmask = hash.lidar ? (int32_t)(hash.lidar - 1) : 0;
}

// A slot of mrca_step_many's run-ahead ring: the five parts a ray cast reads of a move launch, sized as the arena sizes them
// (12 + 16 + 8 + 1 = 37 bytes per robot, 53 with outlines), each on a granule of its own.  Slot 0 is the arena's own fields, and
// a ray cast of several ticks reads a slot or the arena with the same strides.
enum SlotPart { kSlotPose, kSlotHead, kSlotGoal, kSlotFresh, kSlotOutline, kSlotParts };
struct Slot { size_t off[kSlotParts], part_bytes[kSlotParts], bytes; };      // (bytes: of a whole slot)
inline Slot make_slot(const mrca_config& c) {
    Slot s{};
    s.part_bytes[kSlotPose] = part_bytes(c, &EnvView::pose);
    s.part_bytes[kSlotHead] = part_bytes(c, &EnvView::head);
    s.part_bytes[kSlotGoal] = part_bytes(c, &EnvView::goal);
    s.part_bytes[kSlotFresh] = part_bytes(c, &EnvView::fresh);
    s.part_bytes[kSlotOutline] = part_bytes(c, &EnvView::outline);
    for (int i = 0; i < kSlotParts; ++i) {
        s.off[i] = s.bytes;
        s.bytes += align_up(s.part_bytes[i]);
    }
    return s;
}

// v's five pointers into the slot at `base` (per launch: five assignments)
inline void bind_slot(const Slot& s, char* base, EnvView* v) {
    v->pose = reinterpret_cast<float*>(base + s.off[kSlotPose]);
    v->head = reinterpret_cast<float4*>(base + s.off[kSlotHead]);
    v->goal = reinterpret_cast<float*>(base + s.off[kSlotGoal]);
    v->fresh = reinterpret_cast<uint8_t*>(base + s.off[kSlotFresh]);
    if (s.part_bytes[kSlotOutline]) v->outline = reinterpret_cast<OutlineBits*>(base + s.off[kSlotOutline]);
}

}  // namespace arena
}  // namespace mrca
