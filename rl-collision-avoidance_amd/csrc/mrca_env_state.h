// mrca_env_state.h -- what an mrca_env is made of, for the translation units that implement include/mrca_env.h on it:
// mrca_abi.hip (creation, reset, stepping, the run-ahead schedule, timing) and mrca_abi_controllers.hip (the renderer, the
// controllers, the noise model, the planner).  Internal: no other file includes it, and those two include it last (`fail` below is a macro).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/mrca_env.h"
#include "mrca_arena.h"
#include "mrca_hostutil.h"
#include "mrca_kernels.h"

#define fail(...) mrca::set_error(__VA_ARGS__)

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return fail(MRCA_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// (hidden: the library's exports are include/mrca_env.h's, not the env's inside)
namespace mrca {
namespace env_state __attribute__((visibility("hidden"))) {

// Owners of what an env holds beside its arena.  A stream is synchronised before it is destroyed.
struct StreamDeleter { void operator()(hipStream_t s) const { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } };
struct EventDeleter { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct DeviceFree { void operator()(void* p) const { (void)hipFree(p); } };
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDeleter>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDeleter>;
template <class T> using DeviceBuffer = std::unique_ptr<T, DeviceFree>;

inline hipError_t make_stream(Stream* s) {
    hipStream_t h = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (e == hipSuccess) s->reset(h);
    return e;
}
inline hipError_t make_event(Event* ev, unsigned flags = hipEventDisableTiming) {
    hipEvent_t h = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e == hipSuccess) ev->reset(h);
    return e;
}
template <class T> hipError_t device_alloc(DeviceBuffer<T>* p, size_t bytes) {
    void* d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) p->reset(static_cast<T*>(d));
    return e;
}

// mrca_step_many's run-ahead schedule: the move launches of a call's ticks run on a stream of their own,
// AHEAD of the ray casts, each tick writing the five things a ray cast reads of a move launch -- pose, head record, goal,
// fresh flag, outline -- into a slot of its own, so that no move launch ever waits for a ray cast.  Slot 0 is the env's
// own fields (where a call starts and where its last tick ends); slots 1 .. slots live in `mem`.
struct AheadRing {
    DeviceBuffer<char> mem;
    mrca::arena::Slot slot{};         // where the five lie inside a slot, and a slot's bytes (mrca_arena.h)
    int slots = 0;                    // 0: the ring could not be allocated -> the chained schedule
    Stream move_stream;
    std::vector<Event> moved;         // [kAheadTicks] "tick k's move launch is through"
    // A range's ray casts go out as launches of up to ticks_per_launch consecutive ticks (mrca_raycast_ticks.hip; 1: a launch
    // per tick).  Such a launch reads the ring heads from one array and leaves them in another -- the env's ring_head field
    // and head_scratch [N] in turns, so that no workgroup reads what another one of its launch writes.
    int ticks_per_launch = 1;
    bool ticks_forced = false;        // MRCA_TICKS_PER_LAUNCH was set: that many wherever such launches are possible at all
    DeviceBuffer<uint8_t> head_scratch;
};

// mrca_step_many with chains > 1: world range c >= 1's stream and the events that order it against the caller's -- `moved`:
// range c - 1's first move launch is through (the chained schedule starts range c behind it), `done`: range c is through
struct WorldRange { Stream stream; Event moved, done; };

// stream choice (mrca_abi.hip: choose_streams)
struct StreamCheck {
    // (at most 8, oldest first) the move stream and the streams of ranges 1 .. ranges - 1 overlap with `caller` and each other
    struct Record { hipStream_t caller; int ranges; };
    std::vector<Record> checked;                 // the caller's streams the env's CURRENT streams were checked against
    DeviceBuffer<unsigned long long> stamps;     // [4] start / end of the two probe kernels
    std::vector<Stream> parked;                  // found to share a hardware queue with another stream: kept until mrca_destroy
    // has the caller's stream `s` been checked against the env's current streams for P ranges or more?
    bool covers(hipStream_t s, int P) const {
        return std::any_of(checked.begin(), checked.end(), [&](const Record& r) { return r.caller == s && r.ranges >= P; });
    }
};

// is `s` being captured?  A query that fails counts as yes: what a capture cannot hold is not tried then
inline bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

}  // namespace env_state
}  // namespace mrca

// Members are destroyed bottom-up: every stream (world ranges, the move stream, parked ones) is synchronised before the memory
// above it that its launches may read (the ring, the probe stamps, the view copy, an owned arena) is freed.
struct mrca_env {
    template <class T> using DeviceBuffer = mrca::env_state::DeviceBuffer<T>;
    using Event = mrca::env_state::Event;
    DeviceBuffer<char> own_arena;         // the arena when the library allocated it
    mrca_config cfg;
    mrca::arena::Layout layout;
    char* arena = nullptr;
    mrca::EnvView view;
    DeviceBuffer<uint16_t> octant_rect;     // the octant free-rectangle array (outside the arena: the arena's size is ABI), or none
    DeviceBuffer<mrca::EnvView> view_dev;   // `view` in device memory (outside the arena): what move_kernel / raycast_kernel read
    DeviceBuffer<uint32_t> plan_counters;   // mrca_goal_fields' per-launch counters, from its first call on (it returns synchronised)
    size_t lds_bytes = 0;
    // timing
    int timing = 0;      // 0 off, n > 0: record events on every n-th step
    int step_count = 0;
    std::vector<Event> ev;       // 4 per recorded step: begin / end of the move launch, begin / end of the ray cast
    int ev_used = 0;
    int last_ray_count = 0;   // workgroups of the last ray-cast launch (profiling build: whose stamps are current)
    // robots_per_world > 64: does the lidar hash (bw_lstart / bw_lsorted) describe the poses as they stand behind everything
    // enqueued so far?  In enqueue order: false after a move phase without its observe phase, true after launch_lidar_grid
    // (mrca_reset, the observe phase).  Who reads the hash outside the tick asks here (mrca_orca_actions_any).
    bool lidar_hash_current = false;
    bool lidar_counts_pending = false;    // a move phase has left the next hash's bucket populations in bw_lcount
    bool reset_seen = false;              // mrca_reset has been enqueued once: the ring holds scans (mrca_scan_noise asks)
    mrca::env_state::StreamCheck check;   // (these four: mrca_step_many)
    mrca::env_state::AheadRing ahead;
    std::vector<mrca::env_state::WorldRange> ranges;       // world ranges 1 .. P - 1
    Event fork;                           // an early exit's join of the move stream
};
