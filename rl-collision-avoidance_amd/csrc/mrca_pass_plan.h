// mrca_pass_plan.h -- the schedule of one run-ahead pass of mrca_step_many as data: which ticks form a block, how a block's
// ray casts are cut into launches, which ring slot every tick writes and reads, and the order in which the host enqueues it
// all.  Integers only, no HIP and no allocation: mrca_abi.hip executes a plan (run_ahead_pass), tests/test_pass_plan_host.py
// compiles this header for the host and checks every plan of K <= kAheadTicks ticks at up to 8 ticks per launch.
#pragma once
#include <stdint.h>

namespace mrca {

constexpr int kAheadTicks = 256;            // most ticks one run-ahead pass covers (a pass ends with every stream joined: ~90 us)
constexpr int kRayTicksGroups = 3 * 2048;   // most workgroups of a ray-cast launch of several ticks: three residency rounds (ticks_per_launch)
constexpr int kMoveLead = 3;                // how many blocks the move launches are enqueued ahead of the ray casts (>= 1)
constexpr int kOwnTicks = 1;                // ticks below this one: move launches on the caller's stream

// Ticks per ray-cast launch of a pass over P world ranges of W worlds x R robots.  ring_ticks: what the env's ring allows
// (min(F, 8), or what MRCA_TICKS_PER_LAUNCH forced: AheadRing::ticks_per_launch).  lazy_obs = 0: the VIEWS epilogue reads the
// rows earlier ticks stored -- a launch per tick.  Otherwise several, where a range's launch then stays within kRayTicksGroups
// workgroups and the mode is the exact-rectangle one: that is where it was measured to pay (Stage-1, 2 x 2048 robots: +5 %).
// Next to launches of more residency rounds the move launches no longer find free CUs between two ray casts and fall behind
// the ray casts they feed: ranges of 4114 robots (the Stage-2 side figure) lost 2 - 5 % at two ticks per launch, fidelity
// mode -- whose move launch is the longer one -- 22 - 27 % with move launches of up to 70 us (profiles/multitick/).
inline int ticks_per_launch(int lazy_obs, int ring_ticks, bool forced, bool raster, int W, int R, int P) {
    if (!lazy_obs) return 1;
    int T = ring_ticks;
    if (!forced) {
        const int most = (W + P - 1) / P * R;             // robots of the largest range
        if (T > kRayTicksGroups / most) T = kRayTicksGroups / most;
        if (T < 1 || raster) T = 1;
    }
    return T;
}

// Ticks of block b, which starts at tick a, at T ticks per ray-cast launch: [0], [1], [2], [3], then fours; with T > 1: [0],
// [1], two, four times T (T = 2: once), then 2 T each: at no length of a pass more waits than with a launch per tick, and small
// blocks while the move launches are not far ahead yet -- a block's ray casts wait for its LAST move launch, and next to
// launches of several residency rounds a move launch takes up to 20 us (launch stamps, profiles/multitick/).
inline int block_ticks(int T, int b, int a) {
    if (T == 1) return a < 4 ? 1 : 4;
    return b < 2 ? 1 : b == 2 ? 2 : b < (T > 2 ? 7 : 4) ? T : 2 * T;
}

// One pass of K ticks (1 .. kAheadTicks) at T ticks per ray-cast launch; the same for every world range.
//
// Ticks are enqueued in BLOCKS (block_ticks): a block's move launches, ONE event behind the last of them, and every range's
// stream waits for that event once before it takes the block's ray casts.  hipStreamWaitEvent is the dearest call of a pass
// (4.6 us of host time against ~3 for a launch: a build with host timers, profiles/r06_ai_*): a wait per tick and range made
// the host 15.8 us per tick against the device's 19.1 -- any hiccup starved the queues.
// The HOST ORDER (ops) matters as much: the host needs ~13 us per tick, the device ~16.5, so the device is never far behind
// the host and what is enqueued late starts late.  The move launches of block b + kMoveLead are therefore enqueued BEFORE the
// ray casts of block b: they have a queue of their own, under load they come ~13 us apart (not 8.5: the launch stamps of the
// profiling build, MRCA_LAUNCH_STAMPS), and a ray cast waits 10 us beyond the end of the move launch it depends on.
// Measured (own ticks on the caller's stream x blocks of lead, profiles/r06_ai_*): lead 1 (round 6's first form) 463 us per
// 20-tick region, lead 2 - 4 with one or two own ticks 436 - 445; tick 0 alone on the caller's stream and lead 3 kept.
// A block's ray casts wait for an event the host has recorded by then -- a wait for an event not yet recorded is no wait at
// all --: Rays(b) stands behind Moves(b) in ops.
struct PassPlan {
    // A ray-cast launch of a range: ticks first .. first + ticks - 1, inside one block.  A launch of several ticks moves the
    // ring heads from one of two arrays to the other (a launch of one tick leaves them where it finds them) -- the env's field
    // and a scratch array; heads_in_scratch: where they are when the launch starts.
    struct Launch { int16_t first, ticks, heads_in_scratch; };
    enum OpKind : int16_t { kMoves, kRays };
    struct Op { int16_t kind, block; };      // "the move launches of `block`" / "every range's ray casts of `block`"

    int K, T;
    int num_blocks, num_launches, num_ops;
    int16_t first_of[kAheadTicks + 1];       // block b: ticks first_of[b] .. first_of[b + 1] - 1
    int16_t launches_of[kAheadTicks + 1];    // block b: launches launches_of[b] .. launches_of[b + 1] - 1
    Launch launch[kAheadTicks + 1];          // (at most one per tick; [num_launches]: the pass's end, where the heads are after it)
    Op ops[2 * kAheadTicks];

    // Tick k's move launch writes write_slot(k) and reads read_slot(k) = what tick k - 1 wrote; its ray cast reads
    // write_slot(k), and a launch of several ticks the slots from there downwards.  Slot 0 is the env's own fields: the pass
    // starts from them and its last tick leaves them current.
    int write_slot(int k) const { return K - 1 - k; }
    int read_slot(int k) const { return k == 0 ? 0 : K - k; }
};

inline void plan_pass(int K, int T, PassPlan* p) {
    p->K = K;
    p->T = T;
    int nb = 0;
    for (int a = 0; a < K; ++nb) {
        p->first_of[nb] = (int16_t)a;
        a += block_ticks(T, nb, a);
    }
    p->first_of[nb] = (int16_t)K;
    p->num_blocks = nb;
    // A block's ray casts of one range: launches of up to T ticks each.  The pass must leave the ring heads in the env's field:
    // an odd number of launches of several ticks is made even by sending the first of them tick by tick.
    int several = 0;
    for (int b = 0; b < nb; ++b)
        for (int k = p->first_of[b]; k < p->first_of[b + 1]; k += T) several += p->first_of[b + 1] - k > 1 && T > 1;
    bool split = several & 1;
    int nl = 0;
    int16_t in_scratch = 0;
    for (int b = 0; b < nb; ++b) {
        p->launches_of[b] = (int16_t)nl;
        for (int k = p->first_of[b]; k < p->first_of[b + 1]; k += T) {
            const int n = p->first_of[b + 1] - k < T ? p->first_of[b + 1] - k : T;
            if (n > 1 && !split) {
                p->launch[nl++] = {(int16_t)k, (int16_t)n, in_scratch};
                in_scratch ^= 1;
                continue;
            }
            for (int q = 0; q < n; ++q) p->launch[nl++] = {(int16_t)(k + q), 1, in_scratch};
            if (n > 1) split = false;
        }
    }
    p->launches_of[nb] = (int16_t)nl;
    p->launch[nl] = {(int16_t)K, 0, in_scratch};
    p->num_launches = nl;
    int no = 0;
    for (int b = 0; b < nb && b < kMoveLead; ++b) p->ops[no++] = {PassPlan::kMoves, (int16_t)b};
    for (int b = 0; b < nb; ++b) {
        if (b + kMoveLead < nb) p->ops[no++] = {PassPlan::kMoves, (int16_t)(b + kMoveLead)};
        p->ops[no++] = {PassPlan::kRays, (int16_t)b};
    }
    p->num_ops = no;
}

}  // namespace mrca
