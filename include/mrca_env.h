/*
 * mrca_env.h -- C ABI of the MI355X-native multi-robot collision-avoidance environment.
 *
 * This is the drop-in boundary for ONE path of Acmece/rl-collision-avoidance: the per-robot
 * ROS/Stage simulation behind the `StageWorld` class.  The reference has no C plugin API for
 * this path; what a caller binds to is (a) the StageWorld method set and (b) the stageros topic
 * contract underneath it.  Every entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - every pointer suffixed _dev is DEVICE memory on the env's GPU, everything else is host;
 *   - all calls are asynchronous on `stream`, there is no hidden synchronisation;
 *   - return value: 0 (MRCA_OK) or a negative mrca_status; mrca_last_error() gives the text
 *     for the calling thread;
 *   - one env per GPU, not thread-safe per handle;
 *   - the env owns one contiguous device arena (either caller-provided or hipMalloc'ed) laid out
 *     structure-of-arrays, every field 256-byte aligned; mrca_get_field() exposes the fields
 *     zero-copy.
 *
 * Robot numbering: robot n lives in world n / robots_per_world with local index
 * n % robots_per_world (the reference's `index` = MPI rank, ppo_stage1.py:168).  Robots only
 * interact (collide, see each other's bodies with the lidar) inside their world.
 */
#ifndef MRCA_ENV_H
#define MRCA_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6, additive: mrca_scatter, mrca_scatter_default_params (a scenario sampler: per world, separated random starts and goals clear
 * of the map, as mrca_reset's poses_dev / goals_dev).
 * 6, additive: mrca_nhorca_actions, mrca_nhorca_default_params (the NH-ORCA baseline: ORCA over the holonomic velocities a
 * unicycle tracks within a bound).
 * 6, additive: mrca_subgoals_los, mrca_los_default_params (the planner's per-tick call with line-of-sight smoothing);
 * mrca_dwa_actions_goal, mrca_hybrid_actions_goal, mrca_hybrid_plan_goal (the sensor-level controllers steered at rows the caller
 * gives, a planner's subgoals for instance, in place of MRCA_F_LOCAL_GOAL).
 * 6, additive: mrca_goal_fields, mrca_subgoals, mrca_planner_grid, mrca_planner_default_params (a global planner: integer goal
 * fields over the map, a subgoal per robot and tick).
 * 6, additive: mrca_hybrid_plan, mrca_hybrid_commit, mrca_safe_policy_default_params, mrca_lidar_features_scaled,
 * mrca_lidar_features_bf16_scaled (hybrid control in the paper's form: the safe policy is the network on a rescaled scan).
 * 6, additive: mrca_hybrid_actions, mrca_hybrid_default_params (hybrid control behind a policy: PID, policy or safe policy per robot).
 * 6, additive: mrca_scan_noise, mrca_scan_noise_default_params (a lidar noise model applied to the ring in place).
 * 6, additive: mrca_dwa_actions,mrca_dwa_default_params (a sensor-level DWA baseline beside ORCA).
 * 6, additive: mrca_orca_actions_any (the ORCA baseline on worlds of any size); mrca_move_worlds / mrca_observe_worlds take the
 * full range of an env with robots_per_world > 64.
 * 6, additive: mrca_lidar_features_bf16 (the bf16 MFMA front end of the opt-in bf16 rollout inference); the opt-in fused bf16
 * update's mrca_lidar_features_bf16_rows, mrca_lidar_features_bf16_backward(_rows, _scratch).
 * 6 (round 6): MRCA_F_HIT_BITS -- what a beam hit is a bit plane of its own, MRCA_F_SCAN_RING holds plain ranges (5: the sign
 * bit of a ring entry); mrca_step_many's run-ahead schedule (chains < 0: the chained one).
 * 5 (round 5): mrca_policy_tail takes fc1_b_dev (may be NULL) after h1_dev; added since 4, all additive: mrca_step_worlds,
 * mrca_move_worlds, mrca_observe_worlds, mrca_step_many, mrca_adam_step, mrca_policy_heads(_backward), mrca_relu_cat(_backward), mrca_rollout_rows +
 * mrca_rollout_store_state / _outcome, status bits for mrca_check.  4: the frame history became a ring of raw scans (MRCA_F_SCAN_RING, MRCA_F_RING_HEAD). */
#define MRCA_ABI_VERSION 6

typedef struct mrca_env mrca_env; /* opaque */

enum mrca_status {
    MRCA_OK = 0,
    MRCA_ERR_INVALID = -1,     /* bad argument / config */
    MRCA_ERR_HIP = -2,         /* a HIP runtime call failed */
    MRCA_ERR_NOMEM = -3,       /* arena too small / allocation failed */
    MRCA_ERR_UNSUPPORTED = -4  /* e.g. robots_per_world > 64 together with group-synchronous episodes */
};

/* episode structure */
enum mrca_auto_reset {
    MRCA_AUTO_NONE = 0,  /* circle_test.py:36-83 : nothing resets, first terminal event latched  */
    MRCA_AUTO_ROBOT = 1, /* ppo_stage1.py:51-58  : each robot starts a new episode when done     */
    MRCA_AUTO_GROUP = 2  /* ppo_stage2.py:72-107 : done robots idle until their whole group done */
};

/* per-local-index rule for reset_pose / generate_goal_point */
enum mrca_reset_mode {
    MRCA_RESET_TABLE = 0, /* model/utils.py:6-63 tables (stage_world2.py:213-214, circle_world.py:205) */
    MRCA_RESET_DISC = 1,  /* stage_world1.py:251-274                                                  */
    MRCA_RESET_REGION = 2 /* stage_world2.py:250-287 (robots 34..43)                                   */
};

/* get_reward_and_terminate's third return value (stage_world1.py:194,201,208) */
enum mrca_result { MRCA_RESULT_NONE = 0, MRCA_RESULT_REACH = 1, MRCA_RESULT_CRASH = 2, MRCA_RESULT_TIMEOUT = 3 };

/* device-resident fields; shapes in [] with N = num_worlds*robots_per_world, B = beams, F = frames */
enum mrca_field {
    MRCA_F_POSE = 0,      /* f32 [N,3]   get_self_stateGT   stage_world1.py:116 ; base_pose_ground_truth stageros.cpp:575 */
    MRCA_F_SPEED,         /* f32 [N,2]   get_self_speed     stage_world1.py:143 ; odom twist stageros.cpp:543-558        */
    MRCA_F_SPEED_GT,      /* f32 [N,2]   get_self_speedGT   stage_world1.py:119 ; stageros.cpp:585-590                   */
    MRCA_F_GOAL,          /* f32 [N,2]   env.goal_point     stage_world1.py:173                                          */
    MRCA_F_INIT_POSE,     /* f32 [N,3]   env.init_pose      stage_world1.py:263                                          */
    MRCA_F_SCAN,          /* f32 [N,B]   base_scan ranges   stageros.cpp:479-516 : the newest scan, a COPY out of
                           *             MRCA_F_SCAN_RING -- current after every call with lazy_obs = 0, otherwise after
                           *             mrca_materialize(MRCA_VIEW_SCAN)                                                    */
    MRCA_F_OBS,           /* f32 [N,F,B] get_laser_observation x frame deque  stage_world1.py:122-140, ppo_stage1.py:59-60,87-89
                           *             x / 6 - 0.5 of the last F scans in deque order (oldest frame first), made from
                           *             MRCA_F_SCAN_RING: current after every call with lazy_obs = 0, otherwise after
                           *             mrca_materialize(MRCA_VIEW_OBS) */
    MRCA_F_LOCAL_GOAL,    /* f32 [N,2]   get_local_goal     stage_world1.py:155-160                                      */
    MRCA_F_REWARD,        /* f32 [N]     get_reward_and_terminate[0]  stage_world1.py:180-211                            */
    MRCA_F_DONE,          /* u8  [N]     get_reward_and_terminate[1]                                                     */
    MRCA_F_RESULT,        /* u8  [N]     get_reward_and_terminate[2] as enum mrca_result                                 */
    MRCA_F_FIRST_RESULT,  /* u8  [N]     first terminal event since reset (success-rate metric)               */
    MRCA_F_CRASHED,       /* u8  [N]     get_crash_state    stage_world1.py:149 ; is_crashed stageros.cpp:562-564        */
    MRCA_F_LIVE,          /* u8  [N]     `liveflag`         ppo_stage2.py:52,85-86                                       */
    MRCA_F_FRESH,         /* u8  [N]     1 where the last call started a new episode for the robot                      */
    MRCA_F_T,             /* i32 [N]     the `step` argument of get_reward_and_terminate (ppo_stage1.py:57,118)          */
    MRCA_F_EPISODE,       /* i32 [N]     episode counter (RNG stream position)                                          */
    MRCA_F_PREV_DIST,     /* f32 [N]     self.distance      stage_world1.py:176-177,185-186                              */
    MRCA_F_SCAN_RING,     /* f32 [N,F,B] the last F scans of every robot (RAW ranges, 0..6 m, never below zero; a zero may be -0.0: a beam
                           *             that enters a wall at boundary time -0, as in the oracle) as a ring (ABI 4): a
                           *             tick writes ONE row per robot -- the tick's only per-beam store -- logical frame f
                           *             (0 = oldest) of robot n is slot (head[n] + 1 + f) mod F.  (ABI 3 kept a ring of
                           *             NORMALISED frames next to MRCA_F_SCAN: every beam was stored twice.  ABI 4-5 kept
                           *             what a beam hit in the SIGN BIT of its entry; since ABI 6 that is MRCA_F_HIT_BITS
                           *             and an entry is the plain range.)                                               */
    MRCA_F_RING_HEAD,     /* u8  [N]     slot of robot n's newest scan in MRCA_F_SCAN_RING                                */
    MRCA_F_HIT_BITS,      /* u64 [N,F,B/64] (ABI 6) what every beam of the ring hit, one bit per beam, slot by slot like the
                           *             ring: bit (b & 63) of word b >> 6 set = beam b returned from ANOTHER ROBOT
                           *             (ranger_return 0.5, stage1.world:95 -- what stageros turns into LaserScan intensity
                           *             0, stageros.cpp:506), clear = the floorplan or nothing (range 6.0)              */
    MRCA_F_COUNT
};

typedef struct mrca_config {
    int32_t abi_version;       /* MRCA_ABI_VERSION */
    int32_t device;            /* HIP device ordinal */
    int32_t num_worlds;
    int32_t robots_per_world;  /* 1..64: one wavefront per world; > 64: per-robot threads + per-tick broad phase */
    int32_t beams;             /* 512 (stage1.world:14); 64..1024, multiple of 64 */
    int32_t frames;            /* 3 (LASER_HIST, ppo_stage1.py:24); 1..8 */
    /* occupancy grid shared by all worlds; cells outside it are free */
    int32_t map_width, map_height, map_words_per_row;   /* cells; at most 16384 per side */
    float map_cell, map_x0, map_y0; /* cell edge [m]; world coords of the lower-left corner */
    const uint32_t* map_bits;       /* host, [map_height][map_words_per_row], bit b of word w = column 32w+b */
    /* reward / episode rules (stage_world1.py:180-211 and the stage2 / circle variants) */
    int32_t timeout;        /* 150 / 200 / 10000 */
    float w_thresh;         /* 1.05 / 1.05 / 0.7 */
    int32_t pre_dist_zero;  /* stage_world2.py:170-171, circle_world.py:166-167 quirk */
    int32_t auto_reset;     /* enum mrca_auto_reset */
    uint64_t seed;          /* Philox key */
    /* per local index (robots_per_world entries each); NULL = all MRCA_RESET_DISC / zeros */
    const int32_t* reset_mode;
    const int32_t* goal_mode;
    const float* init_table;  /* [R,3] */
    const float* goal_table;  /* [R,2] */
    const int32_t* group_id;  /* [R] in 0..15, model/utils.py:83 */
    /* Fidelity mode (ABI 2).  0 = robots collide when their 0.44 x 0.38 rectangles overlap (exact, resolution-free).
     * res > 0 [m] = Stage's rule on a raster of `res` metres (worlds/stage1.world:3: 0.2): robots collide when their
     * OUTLINES SHARE A RASTER CELL, i.e. up to one cell apart.  res >= 0.1; not with robots_per_world > 64. */
    float collision_raster;
    /* ABI 3 / 4.  0: MRCA_F_SCAN and MRCA_F_OBS are brought up to date by every mrca_reset / mrca_step* -- what a caller
     * written against ABI 2 expects; since round 6 the stepping calls' ray cast writes the two views of its robots itself
     * (8 kB per robot beside its 2 kB ring row: 180 instead of 247 M agent-steps/s at 4096 robots; as a pass of its own behind
     * every ray cast it was 131).  1: only mrca_materialize() does that; callers that read MRCA_F_SCAN_RING +
     * MRCA_F_RING_HEAD (mrca_lidar_features does) never pay for it. */
    int32_t lazy_obs;
    /* ABI 3, fidelity.  0: a robot that is not acting any more (MRCA_F_LIVE = 0: finished, waiting for its group,
     * ppo_stage2.py:72-107) is commanded (0, 0), and MRCA_F_SPEED restarts at 0 with every episode.  1: what stageros
     * does -- SetSpeed persists (stageros.cpp:272-280; the watchdog of :466-471 is global and the other robots keep it
     * fed): such a robot keeps driving at the last command it was given, still collides and is still seen, and the odom
     * twist get_self_speed reads (stage_world1.py:106-108,146-147) survives reset_pose's teleport. */
    int32_t hold_velocity;
} mrca_config;

/* Bytes of device arena an env with this config needs (256-byte granules). */
int mrca_arena_bytes(const mrca_config* cfg, size_t* bytes_out);

/* Replaces: StageWorld.__init__ (stage_world1.py:17-84) + the stageros process it talks to
 * (stageros.cpp:311-437).  arena_dev may be NULL (the library allocates) or caller-owned device
 * memory of at least mrca_arena_bytes() (e.g. a torch tensor's data_ptr). */
/* (Beside the arena an env with robots_per_world <= 64 allocates the run-ahead ring of mrca_step_many -- 53 B per robot and
 * slot, at most 255 slots / 256 MB; 55 MB at 4096 robots -- one stream + events for the move launches and one per world range in
 * use.  If that allocation fails the env works without it: mrca_step_many then runs the chained schedule.  Every env also keeps a
 * 560-byte copy of its internal view in device memory: the two kernels of the tick read it there instead of taking it as a
 * kernel argument -- a launch with <= 104 bytes of arguments costs the host 2.6 us, one with more 3.2 - 3.5.) */
int mrca_create(const mrca_config* cfg, void* arena_dev, size_t arena_bytes, mrca_env** env_out);
int mrca_destroy(mrca_env* env);

/* Replaces: reset_world / reset_pose / control_pose / generate_goal_point
 * (stage_world1.py:162-177,213-223,237-249; stageros.cpp:260-296).
 *   mask_dev  u8[N] or NULL (= all robots): which robots begin a new episode
 *   poses_dev f32[N,3] or NULL: teleport targets (control_pose); NULL = sample per reset_mode
 *   goals_dev f32[N,2] or NULL: goal points; NULL = sample per goal_mode
 * Re-casts the lidar for the masked robots and fills all F frames with the fresh scan. */
int mrca_reset(mrca_env* env, const uint8_t* mask_dev, const float* poses_dev, const float* goals_dev, void* stream);

/* Replaces one trip round the loop body of ppo_stage1.py:75-91:
 *   control_vel (cmd_vel -> SetSpeed, stageros.cpp:272-280) for every robot,
 *   one Stage tick (UpdateWorld, stageros.cpp:445-449),
 *   get_reward_and_terminate(step), get_laser_observation, get_local_goal, get_self_speed.
 * actions_dev f32[N,2] = (v, omega) already clipped by the caller (ppo_stage1.py:170, model/ppo.py:75). */
int mrca_step(mrca_env* env, const float* actions_dev, void* stream);

/* The same tick for ONE world sharded over several GPUs (a single circle of 50 000 robots): every
 * rank holds the whole world, feeds the commands of ALL robots (one all-gather of act[N,2] per tick -- the exchange
 * step) and advances all of them -- the ordered collision pass needs every provisional pose, and identical arithmetic
 * keeps the replicas bit-identical -- but casts the lidar only for its own robots
 * [first_robot, first_robot + num_robots): scan / obs / local_goal of the other robots are left untouched.  The
 * replicated move phase bounds the speed-up.  Measured (round 6, one rank's share timed on one GPU,
 * profiles/r06_b_bigworld_shards8.jsonl): the move phase is ~20 % of a tick at every size -- 43.7 of 143 us at
 * 50 000 robots, 98 of 474 at 200 000, 244 of 1190 at 500 000 -- so 8 GPUs project to 2.2x / 3.1x / 3.1x (a jam: 2.5 / 3.8 /
 * 4.3x) and the ceiling, ~3.3x, does not rise with the world: there is no size from which the replicated design alone reaches
 * 6x.  Passing it takes a sharded move phase (spatial slabs + the transitive closure of each slab's lower-indexed neighbours
 * and a second exchange per tick); one GPU does 400 M agent-steps/s at 500 000 robots as it is. */
int mrca_step_slice(mrca_env* env, const float* actions_dev, int32_t first_robot, int32_t num_robots, void* stream);

/* The same tick for the worlds [first_world, first_world + num_worlds) ONLY: their robots advance and are observed, every
 * other world is left exactly as it is.  Worlds never interact (one `stageros` process per world in the reference:
 * stage_world1.py:17-84), so a caller may step disjoint world ranges on DIFFERENT streams -- the latency-bound move launch
 * of one range then runs next to the ray cast of another (bench.py --schedule chained) -- or give the policy of
 * one range the time the simulator spends on the other.  actions_dev is still f32[N,2] indexed by robot; only the rows of the
 * range are read.  Calls on overlapping ranges must be ordered by the caller (same stream, or events).
 * robots_per_world > 64: only the full range (MRCA_ERR_UNSUPPORTED otherwise: one world's move phase is one launch chain). */
int mrca_step_worlds(mrca_env* env, const float* actions_dev, int32_t first_world, int32_t num_worlds, void* stream);
/* ... and its two launches one by one: mrca_move_worlds = control_vel + the Stage tick + get_reward_and_terminate + episode
 * bookkeeping of the range (stage_world1.py:225-234,180-211; stageros.cpp:445-449), mrca_observe_worlds = the ray cast at the
 * poses it left + get_local_goal (stageros.cpp:479-516, stage_world1.py:126-160) (+ the two views with lazy_obs = 0).
 * mrca_step_worlds(r) == mrca_move_worlds(r) then mrca_observe_worlds(r) on one stream.  What the split is for: a caller with
 * two streams and an event can hold two world ranges half a tick apart -- range B's move launch goes out when range A's has
 * finished, i.e. next to A's ray cast, tick after tick (bench.py --chains 2: the schedule, DESIGN.md 5.9: what it buys).
 * robots_per_world > 64: only the full range, and the two must alternate (a second mrca_move_worlds without the
 * mrca_observe_worlds in between is MRCA_ERR_INVALID: the observe phase builds the lidar hash from what the move phase counted).
 * Between the two the lidar hash describes the poses BEFORE the move: mrca_orca_actions_any refuses to read it there. */
int mrca_move_worlds(mrca_env* env, const float* actions_dev, int32_t first_world, int32_t num_worlds, void* stream);
int mrca_observe_worlds(mrca_env* env, int32_t first_world, int32_t num_worlds, void* stream);

/* num_ticks ticks of every world from ONE call, with commands that are already on the device (a scripted scenario, a replayed
 * log, the benchmark's action pool): tick k (k = 0 .. num_ticks - 1) takes actions_dev[(first_tick + k) % num_actions], each
 * f32[N,2] as for mrca_step.  Equal, field for field, to num_ticks calls of mrca_step.
 * Because every command is known up front, tick k + 1's move launch does not depend on tick k's ray cast -- only on what the
 * ray cast READS of a move launch: pose, head record, goal, fresh flag, outline.  The call therefore lets the move launches
 * RUN AHEAD (since round 6): tick 0's goes out on `stream`, the others on a stream the env owns, back to back, each writing
 * those five fields into a slot of its own (a ring of <= 255 slots beside the arena, 53 B per robot and slot, at most 256 MB; the call's last
 * tick writes the env's own fields, so MRCA_F_POSE etc. are current when the call's work is done and never in between); the
 * ray casts of chains = P contiguous world ranges run on P streams (range 0 on `stream`, the others on streams the env created
 * in mrca_create for P <= 2, at first use beyond), tick after tick, each behind the event "tick k's move launch is through".  `stream` waits for
 * all of them before the call's work counts as done, and they for everything queued on `stream` before the call.  What a tick
 * then costs is its ray casts alone.
 * With lazy_obs = 1, exact-rectangle collisions and world ranges of at most 3072 robots, a range's ray casts go out as launches
 * of up to `frames` consecutive ticks each (at most 8, at most 6144 workgroups; their ray casts do not depend on each other,
 * every tick's scan is cast and stored, and the later residency rounds of such a launch start without a launch boundary).  Such a launch reads the ring heads from MRCA_F_RING_HEAD and leaves them in an N-byte
 * array of the env's own, or the other way round; the last one of a call leaves them in MRCA_F_RING_HEAD.  The environment
 * variable MRCA_TICKS_PER_LAUNCH, read once in mrca_create, sets the ticks per launch whatever the env's shape (1: a launch per
 * tick; A/B runs).  The host only enqueues (no synchronisation, nothing spins on the
 * device); the call is capturable into a hipGraph like any other (chains > 2: call it once outside the capture first).
 * Streams: the HIP runtime maps a process's streams onto a few hardware queues, and two streams that share one run their
 * kernels one after the other (tools/queue_alias_probe.hip): the schedule stays correct and silently loses its overlap.  At the
 * FIRST call on a given `stream` (outside a capture) the env therefore warms its streams and checks, with two 40 us probe
 * kernels per pair, that its move stream and its ranges' streams really run next to `stream` and to each other, replacing the
 * ones that do not: ~1 ms, once, and the one place where a call of this library synchronises (`stream` and the env's own
 * streams).  Make that first call before a timed or latency-critical region.
 * chains = -P: round 5's schedule instead -- P chains `move, ray cast, move, ray cast ...` of one world range each, half a tick
 * apart (kept for A/B runs: tools/region_sweep.py --schedule chained).  robots_per_world > 64: one chain, in order. */
int mrca_step_many(mrca_env* env, const float* const* actions_dev, int32_t num_actions, int32_t first_tick, int32_t num_ticks,
                   int32_t chains, void* stream);

/* The reference-shaped views of the ring, for all robots (asynchronous on `stream`; needed only with lazy_obs = 1):
 * what & MRCA_VIEW_SCAN: MRCA_F_SCAN := every robot's newest scan; what & MRCA_VIEW_OBS: MRCA_F_OBS := x / 6 - 0.5
 * (stage_world1.py:140) of the ring in deque order. */
enum mrca_view { MRCA_VIEW_SCAN = 1, MRCA_VIEW_OBS = 2 };
int mrca_materialize(mrca_env* env, int32_t what, void* stream);
/* out_dev f32[N,B] := x / 6 - 0.5 of every robot's newest scan -- the ONE observation row per tick a rollout buffer that
 * stores single frames keeps (ppo_stage1.py:87-89 appends exactly this row to the deque). */
int mrca_newest_obs(mrca_env* env, float* out_dev, void* stream);

/* out_dev[i] := in_dev[i] / 6 - 0.5 (stage_world1.py:140) for `count` floats, rounded exactly as MRCA_F_OBS is -- for a caller
 * that holds rows of MRCA_F_SCAN_RING (several envs concatenated, a slice of a sharded world) and wants observations.
 * count % 4 == 0, both buffers 16-byte aligned; in place allowed. */
int mrca_normalize_scans(const float* in_dev, float* out_dev, size_t count, void* stream);

/* get_laser_observation for a StageWorld constructed with beam_num != the lidar's sample count (stage_world1.py:126-139:
 * the sparse scan is a left half picked ascending and a right half picked descending from the raw one):
 * out_dev f32[N,F,beam_num] := x / 6 - 0.5 of beams index_dev[0..beam_num) of every frame of the stack, deque order.
 * index_dev i32[beam_num], each in [0, beams): the caller's table (the reference advances a float64 index by
 * raw / beam_num per pick and truncates; mrca/vec_env.py:sparse_beam_index restates that loop). */
int mrca_sparse_obs(mrca_env* env, const int32_t* index_dev, int32_t beam_num, float* out_dev, void* stream);

/* Top-down views of worlds, rendered where the state lives (replaces: Stage's GUI window, `stageros` without -g; the
 * reference's GIFs under doc/ are captures of it).  View v shows world views[v].world through an image of width x height pixels
 * centred on (cx, cy) [m] at m_per_px metres per pixel, row 0 = +y, point-sampled at pixel centres (no anti-aliasing):
 *   ids_dev   u32[V,H,W]   out: per pixel the MAXIMUM of layer << 24 | local robot index over everything that covers it --
 *                          layers 0 background, 1 map cell occupied, 2 within 0.25 m of a MRCA_F_GOAL, 3 / 4 end of a beam of
 *                          the newest scan that returned from the floorplan / from a robot (MRCA_F_HIT_BITS), 5 inside a
 *                          robot's 0.44 x 0.38 footprint, 6 its front quarter; the pixels containing a robot's centre and its
 *                          goal are always marked.  Independent of the order in which anything runs.
 *   trail_dev u32[V,H,W]   or NULL; in/out, the caller's and persistent: max(trail, local index + 1) at the pixel containing
 *                          each robot's centre.  Zero it to start over.
 *   rgb_dev   u8[V,H,W,3]  or NULL; out: ids + trail through the fixed palette of DESIGN.md 5.11 (bodies coloured by
 *                          MRCA_F_CRASHED / MRCA_F_FIRST_RESULT / MRCA_F_LIVE); 4-byte aligned.
 * Asynchronous on `stream`; reads the env's fields as they stand at that point of the stream and writes none of them; any
 * robots_per_world, any mode.  Three launches per 128 views (the views travel as kernel arguments: nothing is staged).
 * Everything is validated before the first HIP call (MRCA_ERR_INVALID): num_views 1..256, width / height 1..4096, a finite
 * centre and a finite positive m_per_px, world in range, ids_dev not NULL, no layer bit outside the enum. */
typedef struct mrca_render_view { int32_t world; float cx, cy, m_per_px; } mrca_render_view;
enum mrca_render_layers { MRCA_RENDER_MAP = 1, MRCA_RENDER_GOALS = 2, MRCA_RENDER_BODIES = 4, MRCA_RENDER_BEAMS = 8 };
int mrca_render(mrca_env* env, const mrca_render_view* views /* host */, int32_t num_views, int32_t width, int32_t height,
                uint32_t layers, uint32_t* ids_dev /* [V,H,W] */, uint32_t* trail_dev /* [V,H,W] or NULL */,
                uint8_t* rgb_dev /* [V,H,W,3] or NULL */, void* stream);

/* A classical baseline controller on the device: ORCA (van den Berg, Guy, Lin, Manocha, "Reciprocal n-body collision
 * avoidance") for every robot of the env, from the env's own fields.  It stands in for the NH-ORCA baseline of Long et al. 2018,
 * Sec. V, which the reference does not ship: every success rate of a learned policy can be put next to it, and with `mask_dev`
 * it drives some robots of a world while a policy drives the others (the paper's mixed and non-cooperative scenarios).
 * Per robot: poses, headings and MRCA_F_SPEED_GT of its world's robots give one half plane of permitted velocities per kept
 * neighbour (the max_neighbors nearest within neighbor_dist, crashed and finished ones included: they are still obstacles), the
 * newest row of MRCA_F_SCAN_RING one per sixteenth of the scan (its nearest return below obst_dist whose MRCA_F_HIT_BITS bit is
 * clear, as a static point); the velocity closest to the preferred one (v_pref towards MRCA_F_GOAL, zero within 0.5 m of it,
 * turned by a fixed per-robot angle of at most `jitter` rad) that satisfies them is mapped to a forward-only (v, omega) in
 * [0, max_speed] x [-1, 1].  The rule is csrc/mrca_orca_device.h, separately rounded fp32 steps in a fixed order: the output
 * is reproducible bit for bit (tests/orca_ref.py restates it in NumPy).
 *   params      host; NULL = mrca_orca_default_params: radius 0.35 (the footprint's half diagonal 0.2907 + a margin),
 *               neighbor_dist 6, max_neighbors 10, time_horizon 2, time_horizon_obst 1.5, obst_dist 3, v_pref 1, max_speed 1,
 *               responsibility 0.5, k_omega 6, jitter 0 (time_horizon and k_omega tuned on three closed-loop scenarios,
 *               profiles/orca/defaults.txt)
 *   mask_dev    u8[N] or NULL = all robots
 *   actions_dev f32[N,2] out, 8-byte aligned; rows whose mask byte is 0 are not touched
 *   vel_dev     f32[N,2] or NULL; out: the holonomic velocity chosen (same rows)
 * Asynchronous on `stream`, ONE launch (the params travel as kernel arguments); reads the env as it stands at that point of the
 * stream and writes none of it, so mrca_step with actions_dev can follow on the same stream.  Both lazy_obs values, any beams /
 * frames, exact and raster collision modes.  robots_per_world 1..64: more gives MRCA_ERR_UNSUPPORTED (a world's robots are the
 * lanes of one wavefront); mrca_orca_actions_any below takes worlds of any size.  Everything is validated before the first HIP call (MRCA_ERR_INVALID): every float finite; radius,
 * neighbor_dist, time_horizon, time_horizon_obst, max_speed > 0; 0 <= obst_dist <= 6; 0 <= responsibility <= 1; max_neighbors
 * 0..48; actions_dev not NULL and 8-byte aligned. */
typedef struct mrca_orca_params {
    float radius, neighbor_dist, time_horizon, time_horizon_obst, obst_dist, v_pref, max_speed, responsibility, k_omega, jitter;
    int32_t max_neighbors; /* 0..48 */
} mrca_orca_params;
int mrca_orca_default_params(mrca_orca_params* out);
int mrca_orca_actions(mrca_env* env, const mrca_orca_params* params /* host, NULL = defaults */,
                      const uint8_t* mask_dev /* u8[N] or NULL = all */, float* actions_dev /* f32[N,2] */,
                      float* vel_dev /* f32[N,2] or NULL */, void* stream);

/* The same controller for ANY robots_per_world: same arguments, same validation in the same order (the messages name this
 * call), same asynchronous single launch, same rule -- bit for bit.
 *   robots_per_world <= 64: the launch of mrca_orca_actions; the results are identical.
 *   robots_per_world  > 64: a robot's neighbours are found through the env's lidar hash (the counting sort of the robots by
 *     6.5 m cell that every reset and every observe phase rebuilds for the ray cast): the (2g+1)^2 cells around the robot's
 *     own, g = 1 for neighbor_dist <= 6.3, 2 for <= 12.8, 3 for <= 19.3; a larger neighbor_dist is MRCA_ERR_UNSUPPORTED (on
 *     such worlds only).  One wavefront per robot streams the cells' robots through its lanes 64 at a time and keeps the
 *     max_neighbors nearest by (distance, index), a total order: the result does not depend on the order inside the hash, and
 *     it is the list mrca_orca_actions' rule would choose among all robots of the world.
 *     The hash must describe the current poses.  It does after mrca_reset, mrca_step, mrca_step_slice, mrca_step_worlds,
 *     mrca_step_many and mrca_observe_worlds; it does not between mrca_move_worlds and mrca_observe_worlds (nor before the
 *     first mrca_reset): there the call returns MRCA_ERR_INVALID and names mrca_observe_worlds.  The env keeps that flag on
 *     the host in the order of the calls, so calls on several streams must be issued in the order they are meant to run.
 * Writes nothing of the env: no field, no scratch of the broad phase, no status bit. */
int mrca_orca_actions_any(mrca_env* env, const mrca_orca_params* params /* host, NULL = defaults */,
                          const uint8_t* mask_dev /* u8[N] or NULL = all */, float* actions_dev /* f32[N,2] */,
                          float* vel_dev /* f32[N,2] or NULL */, void* stream);

/* The NH-ORCA baseline (Alonso-Mora, Breitenmoser, Rufli, Beardsley, Siegwart, "Optimal reciprocal collision avoidance for multiple
 * non-holonomic robots"): ORCA that may choose only holonomic velocities the unicycle can track within track_error metres, every
 * disc grown by track_error.  A velocity of speed u at angle th from the heading is tracked by omega = th / track_time and
 * v = u (th/2) / tan(th/2); inside the cone |th| <= min(track_time * 1 rad/s, pi/2) and the disc
 * |v| <= min(max_speed, track_error / (track_time sin(th_max / 2))) the unicycle stays within track_error of the point that moves
 * at that velocity over [0, track_time].  The cone enters ORCA's linear program as two hard lines ahead of the static ones.
 * Two solves per robot: a free one (ORCA with the grown radius) decides whether the tracked one aims at the preferred velocity
 * or at zero, and which way the robot turns in place when the tracked one stands still.  The rule is
 * csrc/mrca_nhorca_device.h, reproducible bit for bit (tests/nhorca_ref.py restates it in NumPy); DESIGN.md 5.19.
 *   params      host; NULL = mrca_nhorca_default_params: ORCA's defaults, then track_error and track_time (chosen by a
 *               closed-loop sweep, profiles/nhorca/defaults.txt).  k_omega is ignored.
 *   vel_dev     f32[N,2] or NULL: the tracked solve's velocity
 *   mode_dev    i32[N] or NULL, 4-byte aligned: MRCA_NHORCA_*
 * mask_dev, actions_dev, the stream, what is read and that nothing of the env is written: as mrca_orca_actions.  Worlds of ANY
 * size: up to 64 robots the small launch, above that the neighbours come from the lidar hash under mrca_orca_actions_any's
 * rules (neighbor_dist <= 19.3 or MRCA_ERR_UNSUPPORTED; the hash must describe the current poses or MRCA_ERR_INVALID).
 * Validated before the first HIP call (MRCA_ERR_INVALID): every float finite; mrca_orca_actions' rules for its fields;
 * track_error in (0, 0.5]; track_time in [0.1, 1.5]; max_neighbors 1..46 (two of the 64 constraints are the heading lines). */
typedef struct mrca_nhorca_params {
    float radius, neighbor_dist, time_horizon, time_horizon_obst, obst_dist, v_pref, max_speed, responsibility, k_omega, jitter;
    int32_t max_neighbors; /* 1..46 */
    float track_error;     /* eps [m] */
    float track_time;      /* T [s] */
} mrca_nhorca_params;
enum {
    MRCA_NHORCA_TRACK = 0, /* drives at the preferred velocity as far as the constraints allow */
    MRCA_NHORCA_TURN = 1,  /* turns in place */
    MRCA_NHORCA_STILL = 2, /* stands still */
    MRCA_NHORCA_EVADE = 3  /* should turn in place but the constraints make it move */
};
int mrca_nhorca_default_params(mrca_nhorca_params* out);
int mrca_nhorca_actions(mrca_env* env, const mrca_nhorca_params* params /* host, NULL = defaults */,
                        const uint8_t* mask_dev /* u8[N] or NULL = all */, float* actions_dev /* f32[N,2] */,
                        float* vel_dev /* f32[N,2] or NULL */, int32_t* mode_dev /* i32[N] or NULL */, void* stream);

/* A second classical baseline on the device, SENSOR-LEVEL where ORCA is agent-level: the dynamic window approach (Fox, Burgard,
 * Thrun, "The dynamic window approach to collision avoidance", 1997).  Per robot it reads what the policy reads and nothing
 * else: MRCA_F_LOCAL_GOAL (the goal in the robot's frame), MRCA_F_SPEED (its own command (v0, w0)) and the newest row of
 * MRCA_F_SCAN_RING (through MRCA_F_RING_HEAD).  MRCA_F_HIT_BITS, poses, MRCA_F_SPEED_GT and the other robots are NOT read: a
 * return from a robot is an obstacle like a wall, and every obstacle is taken as standing still.
 *   Within kGoalRadius (0.5 m) of the goal the command is (0, 0), choice -2.  Otherwise the scan is cut into 64 sectors of
 * beams / 64 beams; a sector's nearest return below min(obst_dist, 6) (the lowest beam among equals, -0.0 counts as 0) is an
 * obstacle point range * (beam_cos, beam_sin).  The window is v in [max(0, v0 - acc_v dt), min(max_speed, v0 + acc_v dt)] and
 * omega in [max(-max_omega, w0 - acc_w dt), min(max_omega, w0 + acc_w dt)], dt = 0.1 s (a command outside the rectangle takes
 * the nearest part of it), sampled nv x nw evenly with both ends (one sample: the upper end); candidate c = i * nw + j.  Each
 * candidate is rolled out from (0, 0), heading 0, in `steps` explicit Euler sub-steps of horizon / steps (position first, with
 * the heading at the start of the sub-step, as the env's own move).  clear = sqrt(least squared distance of any sub-step
 * position to any point) - radius, clear_cap where there is no point; admissible iff clear >= 0.
 *   score = w_goal (|g| - |g - p_end|) / (max_speed horizon) + w_heading cos(angle between the end heading and g - p_end; 1 at
 *           the goal itself) + w_clear min(clear, clear_cap) / clear_cap + w_speed v / max_speed.
 * The admissible candidate of greatest score wins, the lowest c among equals; none admissible: (0, +-max_omega) towards the
 * goal's side (gy >= 0: +), choice -1.  The rule is csrc/mrca_dwa_device.h, separately rounded fp32 steps in a fixed order: the
 * output is reproducible bit for bit (tests/dwa_ref.py restates it in NumPy).
 *   params      host; NULL = mrca_dwa_default_params: radius 0.35, horizon 2, obst_dist 3, clear_cap 1, max_speed 1, max_omega 1,
 *               acc_v 10, acc_w 20 (the env has no acceleration limit: the window is the whole range), w_goal 1, w_heading 0,
 *               w_clear 0.2, w_speed 0.3, steps 10, nv 5, nw 21 (profiles/dwa/defaults.txt)
 *   mask_dev    u8[N] or NULL = all robots
 *   actions_dev f32[N,2] out, 8-byte aligned; rows whose mask byte is 0 are not touched (nor are their choice / score rows)
 *   choice_dev  i32[N] or NULL; out: the candidate chosen, -1 (none admissible) or -2 (at the goal)
 *   score_dev   f32[N] or NULL; out: the chosen candidate's score (0 for choice < 0)
 * Asynchronous on `stream`, ONE launch (one wavefront per robot, the params travel as kernel arguments); reads the env as it
 * stands at that point of the stream and writes none of it, so mrca_step with actions_dev can follow on the same stream.  Any
 * robots_per_world (a robot needs nothing of another: no neighbour search), both lazy_obs values, any beams / frames, exact
 * and raster collision modes.  Everything is validated before the first HIP call (MRCA_ERR_INVALID): every float finite;
 * radius, horizon, clear_cap, max_speed, max_omega > 0; max_speed, max_omega <= 1; 0 <= obst_dist <= 6; acc_v, acc_w and the
 * four weights >= 0; steps 1..64, nv 1..16, nw 1..64; actions_dev not NULL and 8-byte aligned. */
typedef struct mrca_dwa_params {
    float radius, horizon, obst_dist, clear_cap, max_speed, max_omega, acc_v, acc_w, w_goal, w_heading, w_clear, w_speed;
    int32_t steps, nv, nw;
} mrca_dwa_params;
int mrca_dwa_default_params(mrca_dwa_params* out);
int mrca_dwa_actions(mrca_env* env, const mrca_dwa_params* params /* host, NULL = defaults */, const uint8_t* mask_dev,
                     float* actions_dev /* f32[N,2] */, int32_t* choice_dev /* i32[N] or NULL */,
                     float* score_dev /* f32[N] or NULL */, void* stream);
/* mrca_dwa_actions steered at the caller's rows: goal_dev f32[N,2], 8-byte aligned, in each robot's own frame (what mrca_subgoals
 * / mrca_subgoals_los write to local_dev), stands wherever the rule above says "the goal" -- the 0.5 m stop, the progress and
 * heading terms, the side it turns to when nothing is admissible.  NULL = MRCA_F_LOCAL_GOAL: the launch and the bits are
 * mrca_dwa_actions'.  The same kernel, the same validation (the messages name this call).  A SUBGOAL WITHIN 0.5 m STOPS THE ROBOT:
 * feed it subgoals with lookahead * stride * map_cell > 0.5 m.  (mrca_orca_actions steers at MRCA_F_GOAL in the world frame and
 * has no such sibling.) */
int mrca_dwa_actions_goal(mrca_env* env, const mrca_dwa_params* params /* host, NULL = defaults */, const uint8_t* mask_dev,
                          float* actions_dev /* f32[N,2] */, int32_t* choice_dev /* i32[N] or NULL */,
                          float* score_dev /* f32[N] or NULL */, const float* goal_dev /* f32[N,2] or NULL */, void* stream);

/* A lidar noise model on the device: turns the exact ranges the ray cast has just stored into what a real ranger would have
 * reported -- IN PLACE, in MRCA_F_SCAN_RING, so that everything sensor-level (the policy's fused front end, mrca_dwa_actions,
 * ORCA's static points, the renderer's beam layer, mrca_rollout_store_state, mrca_materialize / mrca_newest_obs) reads the
 * noisy row.  For beam b of robot n with clean range r (csrc/mrca_noise_device.h, separately rounded fp32 steps in a fixed
 * order: reproducible bit for bit, tests/noise_ref.py restates it in NumPy):
 *   U = philox4x32_10(n, MRCA_F_EPISODE[n], b, (MRCA_F_T[n] << 2) | 2, seed) -- the reset sampler's robot word and key; its
 *       streams use counter word 3 = 0 and 1, which a word with low bits 2 cannot meet.  The draw hangs on (seed, robot,
 *       episode, T, beam) and on nothing else: not on the launch shape, the mask or the order of calls.
 *   r >= 6: the beam returned nothing -- it stays as it is, its hit bit stays clear.  Otherwise
 *   z  = (((u01(U.x) + u01(U.y)) + u01(U.z)) - 1.5) * 2   (a three-uniform Irwin-Hall deviate: mean 0, variance 1, support
 *        +-3 -- NOT a Gaussian);
 *   r1 = r + (sigma_const + sigma_prop * r) * z if one of the sigmas is > 0, else r;
 *   r2 = quantum * rintf(r1 / quantum) if quantum > 0, else r1;   !(r2 > 0) gives +0.0;   r2 >= 6 gives 6.0 and clears the
 *   beam's bit in MRCA_F_HIT_BITS (a set bit never stands on a 6.0);   u01(U.w) < dropout gives 6.0, bit cleared, whatever
 *   the above produced.
 * Which slots: the newest one (MRCA_F_RING_HEAD[n]); for a robot whose MRCA_F_FRESH flag is set, all `frames` slots and their
 * hit words (the cast has just filled them with one row, as the reference fills its deque).  With lazy_obs = 0 the same launch
 * rewrites MRCA_F_SCAN[n] and the newest frame of MRCA_F_OBS[n] (all frames for a fresh robot) with x / 6 - 0.5 of the row.
 *   ONE CALL PER CAST: the transform is in place and not idempotent -- call it once behind mrca_reset (with that reset's
 * mask) and once behind every mrca_step / mrca_step_slice / mrca_step_worlds / mrca_observe_worlds, with a mask of the
 * robots that call cast.  A second call behind the same cast adds the same draw again.  mrca_step_many casts several ticks
 * per call and cannot be combined with it.
 *   params    host; NULL = mrca_scan_noise_default_params: sigma_const 0.01 m, sigma_prop 0.01, dropout 0.005, quantum 0 -- a
 *             small indoor lidar's order of magnitude, NOT the reference's: Stage is configured without ranger noise
 *   mask_dev  u8[N] or NULL = all robots; rows whose byte is 0 are not touched
 * All four params zero: MRCA_OK without a launch.  Asynchronous on `stream`, ONE launch (one wavefront per robot), capturable;
 * writes the ring, the hit bits and (lazy_obs = 0) the two views of the masked robots and nothing else of the env.  Any
 * robots_per_world, beams, frames, both lazy_obs values, exact and raster modes.  Validated before the first HIP call
 * (MRCA_ERR_INVALID): every float finite; 0 <= sigma_const <= 6; 0 <= sigma_prop <= 1; 0 <= dropout <= 1; 0 <= quantum <= 1;
 * a call before the env's first mrca_reset is refused. */
typedef struct mrca_scan_noise_params {
    float sigma_const;  /* [m], constant part of the range noise */
    float sigma_prop;   /* per metre of range */
    float dropout;      /* probability a returning beam reports nothing */
    float quantum;      /* [m], 0 = none */
} mrca_scan_noise_params;
int mrca_scan_noise_default_params(mrca_scan_noise_params* out);
int mrca_scan_noise(mrca_env* env, const mrca_scan_noise_params* params /* host, NULL = defaults */,
                    const uint8_t* mask_dev /* u8[N] or NULL = all */, void* stream);

/* The scenario sampler: what mrca_reset(env, mask, poses_dev, goals_dev) accepts, produced where the state lives -- per world a
 * DIFFERENT set of starts and goals that keep a stated distance from each other and from the map, the same bits for the same
 * (seed, draw).  The env's own samplers (MRCA_RESET_DISC / _REGION) restate the reference and test neither the map nor the other
 * robots.  The rule (csrc/mrca_scatter_device.h, separately rounded fp32 steps in a fixed order; tests/scatter_ref.py restates
 * it in NumPy), with box[i] = (sx0, sy0, sx1, sy1, gx0, gy0, gx1, gy1) per LOCAL index i, shared by all worlds:
 *   candidate k of robot n:  U = philox4x32_10(n, draw, k, word, seed), word 3 for starts and 7 for goals (the reset sampler
 *       uses the words 0 and 1, the noise model words with low bits 2: a word with low bits 3 meets neither);
 *       x = x0 + (x1 - x0) * u01(U.x), y likewise with U.y; a start's heading is wrap(2 pi * u01(U.z)).  A box with x0 == x1
 *       pins that coordinate: this is how table robots mix with random ones.
 *   clear of the map: the Chebyshev distance (map cells) from the point's cell to the nearest occupied cell must be
 *       > clear_cells.  For a cell outside the map, clamped into it to c', the value is max(that of c', cell distance to c'): a
 *       lower bound of the true distance -- the test may refuse a valid point and never accepts an invalid one.
 *   apart from a point already placed: !(dx * dx + dy * dy < sep * sep); the goal band likewise on the squares.
 *   In each world, for i = 0 .. R-1 in order, start_i is the candidate of the LEAST k < max_tries that is clear and min_sep
 *   apart from start_j for every j < i; then, for i = 0 .. R-1, goal_i is the candidate of the least k that is clear, lies
 *   goal_min .. goal_max from start_i and goal_sep apart from goal_j for every j < i.  If no k qualifies the robot takes
 *   candidate max_tries - 1 as it is, its tries entry is -1, and later robots treat it as placed; otherwise tries = k + 1.
 *   The result hangs on (seed, draw, boxes, params, map) and on nothing else: not on the launch shape or on the other worlds.
 *   params     host; NULL = mrca_scatter_default_params: min_sep 1, goal_sep 1, goal_min 5, goal_max 1e4, clear_cells 4,
 *              max_tries 1024, draw 0
 *   boxes_dev  f32[R,8], device memory and NOT validated on the device: its producer guarantees finite values, x0 <= x1,
 *              y0 <= y1 and |coordinate| <= 1e4 (a value that is not a number fails every test: the robot reports -1)
 *   poses_dev  f32[N,3] out;  goals_dev f32[N,2] out;  tries_dev i32[N,2] out (start, goal) or NULL
 * Asynchronous on `stream`, ONE launch (a workgroup per world, the candidates across its lanes), capturable.  Valid BEFORE the
 * first mrca_reset: it reads the map, the geometry and the seed, and writes its three buffers and nothing of the env.
 * robots_per_world <= 4096 (a world's placed points are held in 32 KB of LDS): more gives MRCA_ERR_UNSUPPORTED.  Validated
 * before the first HIP call (MRCA_ERR_INVALID): every float finite; min_sep >= 0.6 (two 0.44 x 0.38 footprints cannot meet with
 * centres 2 x 0.2907 m apart); goal_sep >= 0; 0 <= goal_min <= goal_max; clear_cells 0..254; max_tries 1..65536; boxes_dev,
 * poses_dev, goals_dev not NULL; poses_dev and tries_dev 4-byte, goals_dev 8-byte aligned. */
typedef struct mrca_scatter_params {
    float min_sep;        /* starts of one world: centre distance >= this [m]                 */
    float goal_sep;       /* goals of one world likewise (0: no test)                          */
    float goal_min, goal_max; /* goal_min <= |goal - own start| <= goal_max                    */
    int32_t clear_cells;  /* starts and goals: Chebyshev distance to an occupied map cell > this (0..254) */
    int32_t max_tries;    /* 1..65536 candidates per start and per goal                        */
    uint32_t draw;        /* scenario number: another draw, another set of scenarios           */
} mrca_scatter_params;
int mrca_scatter_default_params(mrca_scatter_params* out);
int mrca_scatter(mrca_env* env, const mrca_scatter_params* params /* host, NULL = defaults */,
                 const float* boxes_dev /* f32[R,8] */, float* poses_dev /* f32[N,3] out */,
                 float* goals_dev /* f32[N,2] out */, int32_t* tries_dev /* i32[N,2] or NULL */, void* stream);

/* Hybrid control behind a policy, after Fan, Long, Liu, Pan (IJRR 2020, Sec. 5): per robot and tick, which of three drives it --
 * a PID law where nothing stands between it and its goal, the policy's command with v scaled down where something is
 * dangerously close, the policy's command as it is everywhere else.  SENSOR-LEVEL: it reads the newest row of MRCA_F_SCAN_RING
 * (through MRCA_F_RING_HEAD), MRCA_F_LOCAL_GOAL and the incoming command, NOT MRCA_F_HIT_BITS, poses or anything of another
 * robot; behind mrca_scan_noise it sees the noisy row.  In the robot's frame, with goal g, command (vp, wp), ranges r_b
 * (r = r_b + 0: a -0.0 counts as 0) and beam directions (c_b, s_b):
 *   gl = |g| <= 0.5 (kGoalRadius): the command is (0, 0), mode -2.  Otherwise u = g / gl, reach = min(gl, look);
 *   a beam with r < 6 is a return at p = r (c_b, s_b); it BLOCKS iff t = p . u lies in [0, reach] and |px uy - py ux| < corridor;
 *   d_min = least r of all beams, d_front = least r of the beams with c_b >= front_cos (6: none), d_block = least r of the
 *   blocking beams (6: none);
 *   mode 2 (emergent) iff d_min < risk_dist: (vp s, wp), s = clamp((d_front - stop_dist) / (risk_dist - stop_dist), 0, safe_scale)
 *          -- the robot may still turn away at full rate;
 *   mode 1 (simple) iff not emergent and no beam blocks: ORCA's conversion of the velocity v_pid u to (v, omega) at heading 0
 *          (v = min(v_pid ux, max_speed) if ux > 0 else 0; omega = clamp(k_omega uy) if ux > 0 else +-clamp(k_omega));
 *   mode 0 (normal) otherwise: (vp, wp) copied bit for bit, a NaN or a -0.0 included.
 * NOT THE PAPER'S LITERAL FORM: its safe policy runs the network on a rescaled scan; this call sits behind the policy
 * and scales its command only (the literal form is mrca_hybrid_plan / mrca_hybrid_commit below), and the
 * corridor test stands in for the paper's "goal nearer than every obstacle".  The rule is csrc/mrca_hybrid_device.h,
 * separately rounded fp32 steps in a fixed order, minima and a count over the beams: reproducible bit for bit
 * (tests/hybrid_ref.py restates it in NumPy).
 *   params      host; NULL = mrca_hybrid_default_params: risk_dist 0.6, stop_dist 0.3, safe_scale 0.75, corridor 1, look 6,
 *               front_cos 0.5, v_pid 1, k_omega 6, max_speed 1 (profiles/hybrid/defaults.txt)
 *   mask_dev    u8[N] or NULL = all robots
 *   policy_dev  f32[N,2] in: the command to wrap
 *   actions_dev f32[N,2] out, 8-byte aligned, may be policy_dev itself; rows whose mask byte is 0 are not touched (nor are
 *               their mode / clear rows)
 *   mode_dev    i32[N] or NULL; out: 0, 1, 2 or -2
 *   clear_dev   f32[N,3] or NULL; out: d_min, d_front, d_block
 * Asynchronous on `stream`, ONE launch (one wavefront per robot, the params travel as kernel arguments), capturable; reads
 * the env as it stands at that point of the stream and writes none of it, so mrca_step with actions_dev can follow on the same
 * stream.  Any robots_per_world, beams 64 .. 1024, frames 1 .. 8, both lazy_obs values, exact and raster collision modes.
 * Validated before the first HIP call (MRCA_ERR_INVALID): every float finite; 0 <= stop_dist < risk_dist <= 6;
 * 0 <= safe_scale <= 1; corridor > 0; 0 < look <= 6; -1 <= front_cos <= 1; v_pid > 0; 0 < max_speed <= 1; k_omega >= 0;
 * actions_dev not NULL and 8-byte aligned; policy_dev not NULL; a call before the env's first mrca_reset is refused. */
typedef struct mrca_hybrid_params {
    float risk_dist;    /* [m] a return nearer than this makes the robot careful (mode 2) */
    float stop_dist;    /* [m] the nearest return ahead at or below this: v = 0 */
    float safe_scale;   /* the most of the incoming v that mode 2 lets through */
    float corridor;     /* [m] half width of the strip towards the goal that must be free for the PID law */
    float look;         /* [m] its length, at most (and at most the distance to the goal) */
    float front_cos;    /* beams with cos >= this are "ahead" for d_front */
    float v_pid;        /* [m/s] speed of the PID law */
    float k_omega;      /* its turn gain (ORCA's) */
    float max_speed;    /* at most 1 */
} mrca_hybrid_params;
int mrca_hybrid_default_params(mrca_hybrid_params* out);
int mrca_hybrid_actions(mrca_env* env, const mrca_hybrid_params* params /* host, NULL = defaults */,
                        const uint8_t* mask_dev /* u8[N] or NULL */, const float* policy_dev /* f32[N,2] in */,
                        float* actions_dev /* f32[N,2] out; may be policy_dev itself */,
                        int32_t* mode_dev /* i32[N] or NULL */, float* clear_dev /* f32[N,3] or NULL: d_min, d_front, d_block */,
                        void* stream);
/* mrca_hybrid_actions steered at the caller's rows: goal_dev f32[N,2], 8-byte aligned, in each robot's own frame, is g above --
 * the 0.5 m stop, the corridor and the PID law.  NULL = MRCA_F_LOCAL_GOAL: the launch and the bits are mrca_hybrid_actions'.  The
 * same kernel and validation.  A subgoal within 0.5 m stops the robot: lookahead * stride * map_cell must exceed 0.5 m. */
int mrca_hybrid_actions_goal(mrca_env* env, const mrca_hybrid_params* params /* host, NULL = defaults */,
                             const uint8_t* mask_dev /* u8[N] or NULL */, const float* policy_dev /* f32[N,2] in */,
                             float* actions_dev /* f32[N,2] out; may be policy_dev itself */, int32_t* mode_dev /* i32[N] or NULL */,
                             float* clear_dev /* f32[N,3] or NULL */, const float* goal_dev /* f32[N,2] or NULL */, void* stream);

/* Hybrid control in the PAPER'S FORM (Fan, Long, Liu, Pan, IJRR 2020, Sec. 5): the safe policy is the NETWORK run on a scan in
 * which obstacles look nearer, its speed capped.  The mode of mrca_hybrid_actions does not depend on the incoming command, so it
 * is known before the forward runs, and a tick is   plan -> ONE forward with a per-robot scan scale -> commit -> step:
 *   mrca_hybrid_plan     mode_dev[n] = exactly the mode mrca_hybrid_actions reports on the same state (same params);
 *                        scale_dev[n] = scan_scale in mode 2, else 1.0f;  pid_dev[n] = the PID command in mode 1, (0, 0) in the
 *                        other modes;  clear_dev[n] (optional) = d_min, d_front, d_block as mrca_hybrid_actions gives them
 *   the forward          mrca_lidar_features_scaled / mrca_lidar_features_bf16_scaled (below) with scale_dev, then the rest of the
 *                        inference as it is
 *   mrca_hybrid_commit   mode 0: the forward's (vp, wp) bit for bit, a NaN or a -0.0 kept;  modes 1 and -2: pid_dev[n];
 *                        mode 2: (vp > v_cap ? v_cap : vp, wp) -- a NaN vp stays a NaN, wp is kept so that the robot may still
 *                        turn away at full rate;  any other mode value: (vp, wp) copied
 * OUR READING OF THE PAPER'S "SCALED SCAN" (the front ends below): a beam that returned nothing (exactly 6.0, the lidar's range)
 * stays "nothing", a return at r is seen at r s; and the WHOLE stack of three frames is scaled by the CURRENT tick's factor, so
 * that the frames stay mutually consistent (a robot entering the safe mode sees no jump between frames).  The clearance
 * scaling s(d_front) of mrca_hybrid_actions' mode 2 is deliberately NOT applied by the commit: the scaled scan is the paper's
 * mechanism, and stacking ours on top would measure neither.  The rule is csrc/mrca_safe_device.h on top of
 * csrc/mrca_hybrid_device.h (tests/safe_ref.py restates it in NumPy): reproducible bit for bit.
 *
 * mrca_hybrid_plan: ONE launch, one wavefront per robot, the params travel as kernel arguments; reads the newest ring row
 * (MRCA_F_SCAN_RING through MRCA_F_RING_HEAD) and MRCA_F_LOCAL_GOAL, NO command; writes nothing of the env; asynchronous on
 * `stream`, capturable.  Rows whose mask byte is 0 are not touched (pre-fill scale_dev with ones where a mask is used).
 *   hybrid_params  host; NULL = mrca_hybrid_default_params (the classification; safe_scale is not used here)
 *   safe_params    host; NULL = mrca_safe_policy_default_params: scan_scale 0.3, v_cap 0.75 (profiles/safe_policy/defaults.txt)
 *   mask_dev u8[N] or NULL = all;  mode_dev i32[N], scale_dev f32[N], pid_dev f32[N,2] (8-byte aligned): out, not NULL;
 *   clear_dev f32[N,3] or NULL
 * Validated before the first HIP call (MRCA_ERR_INVALID): the table of mrca_hybrid_actions for hybrid_params; scan_scale and
 * v_cap finite, 0 < scan_scale <= 1, 0 < v_cap <= 1; the three outputs not NULL; a call before the env's first mrca_reset is
 * refused.
 *
 * mrca_hybrid_commit: ONE launch, one thread per robot, needs no env.  policy_dev f32[N,2] in; actions_dev f32[N,2] out, 8-byte
 * aligned, may be policy_dev itself; mode_dev, pid_dev as the plan wrote them; rows whose mask byte is 0 are not touched. */
typedef struct mrca_safe_policy_params {
    float scan_scale;   /* what a return's range is multiplied by in mode 2, in (0, 1] */
    float v_cap;        /* the most v that mode 2 lets through, in (0, 1] */
} mrca_safe_policy_params;
int mrca_safe_policy_default_params(mrca_safe_policy_params* out);
int mrca_hybrid_plan(mrca_env* env, const mrca_hybrid_params* hybrid_params /* host, NULL = defaults */,
                     const mrca_safe_policy_params* safe_params /* host, NULL = defaults */,
                     const uint8_t* mask_dev /* u8[N] or NULL */, int32_t* mode_dev /* i32[N] */, float* scale_dev /* f32[N] */,
                     float* pid_dev /* f32[N,2] */, float* clear_dev /* f32[N,3] or NULL */, void* stream);
/* mrca_hybrid_plan steered at the caller's rows (goal_dev f32[N,2], 8-byte aligned, each robot's own frame; NULL =
 * MRCA_F_LOCAL_GOAL, then the launch and the bits are mrca_hybrid_plan's): as mrca_hybrid_actions_goal, the 0.5 m note included. */
int mrca_hybrid_plan_goal(mrca_env* env, const mrca_hybrid_params* hybrid_params /* host, NULL = defaults */,
                          const mrca_safe_policy_params* safe_params /* host, NULL = defaults */,
                          const uint8_t* mask_dev /* u8[N] or NULL */, int32_t* mode_dev /* i32[N] */, float* scale_dev /* f32[N] */,
                          float* pid_dev /* f32[N,2] */, float* clear_dev /* f32[N,3] or NULL */,
                          const float* goal_dev /* f32[N,2] or NULL */, void* stream);
int mrca_hybrid_commit(int32_t n_robots, const mrca_safe_policy_params* safe_params /* host, NULL = defaults */,
                       const uint8_t* mask_dev /* u8[N] or NULL */, const int32_t* mode_dev /* i32[N] */,
                       const float* pid_dev /* f32[N,2] */, const float* policy_dev /* f32[N,2] in */,
                       float* actions_dev /* f32[N,2] out; may be policy_dev itself */, void* stream);

/* A GLOBAL PLANNER under the local controllers: every controller here steers at MRCA_F_LOCAL_GOAL, the straight line to the
 * goal, which is enough on the circle and not on a map with walls.  After Fan, Long, Liu, Pan (IJRR 2020, long-range
 * navigation) the learned policy becomes the LOCAL planner: mrca_goal_fields plans once per goal set, mrca_subgoals gives every
 * robot a SUBGOAL a little way down the shortest path every tick, in the robot's frame, to be handed to the controller in place
 * of MRCA_F_LOCAL_GOAL.  The rule is csrc/mrca_planner_device.h (tests/planner_ref.py restates it in NumPy and heapq):
 *   planning grid  the env's map coarsened by `stride` s: PW = ceil(map_width / s), PH = ceil(map_height / s)
 *                  (mrca_planner_grid); the map cell of a point is floorf((x - map_x0) / map_cell) as everywhere, the planning
 *                  cell that divided by s; a point whose map cell lies outside the map is OFF GRID
 *   blocked        a planning cell is blocked iff an occupied map cell lies within Chebyshev distance `inflate` (map cells) of
 *                  one of its map cells; cells beyond the map are free
 *   field          u32[PH][PW] per goal point: 0 at its planning cell (the SEED, blocked or not; it counts as unblocked from
 *                  there on), 0xFFFFFFFF for every other blocked cell and every cell no path reaches, else the length of the
 *                  shortest 8-connected path to the seed through unblocked cells, a straight step 5, a diagonal step 7, a
 *                  diagonal step only between two unblocked cells (no corner is cut).  A goal off grid: all 0xFFFFFFFF.
 *                  The least solution of D(c) = min D(n) + w: unique, so the words do not depend on the order anything ran in
 *   walk           from the robot's planning cell, up to `lookahead` times: the allowed step of least D(n) + w, ties to the
 *                  lowest direction in the order E, NE, N, NW, W, SW, S, SE, taken only if D(n) < D(c); from a 0xFFFFFFFF
 *                  cell (a robot inside the inflation) every in-grid neighbour with a finite D is a candidate; stops at D = 0
 *   status_dev     1: the walk reached the seed, the subgoal is the slot's goal point bit for bit;  0: the centre of the cell
 *                  reached, map_x0 + ((float)i + 0.5f) * (map_cell * (float)s);  -1: no slot (slot < 0 or >= G);  -2: the robot
 *                  is off grid, or has no candidate at its first step (walled in, or its goal is off grid).  For -1 and -2 the
 *                  subgoal is MRCA_F_GOAL[n] bit for bit
 *   local_dev      the subgoal in the robot's frame, by the expression and from the sine and cosine the ray cast uses for
 *                  MRCA_F_LOCAL_GOAL: wherever the subgoal has the goal's bits, local has MRCA_F_LOCAL_GOAL[n]'s
 *   dist_dev       (float)D(first cell) * ((map_cell * (float)s) / 5.0f) metres; +inf for 0xFFFFFFFF, off grid and no slot
 * WHAT THE NUMBERS ARE NOT.  The chamfer 5 / 7 metric OVER-ESTIMATES the Euclidean length of a path by a few percent (up to 8 %
 * at 26.6 degrees; a pure diagonal is 1 % short), on top of the 8-connected path's own detour.  mrca_subgoals does NO
 * line-of-sight smoothing: its subgoal is a cell centre on the 8-connected path, `lookahead` steps ahead (mrca_subgoals_los
 * below looks further and takes the farthest cell in sight).  One map for all worlds; other robots are not obstacles of the plan.
 *
 * mrca_goal_fields  the PLANNING call: field_dev[g] for goal point goals_dev[g].  One launch initialises the field, then ONE
 *   launch per round relaxes every (goal, tile of 64 x 64 cells) in LDS from the field as it stands; the host reads a counter
 *   every four launches and stops when a launch lowered nothing.  No grid-wide barrier, no cooperative launch, no wait on the
 *   device; every loop has a fixed trip count.  IT SYNCHRONISES `stream` (like mrca_check below) while it looks for convergence,
 *   returns synchronised, and is NOT capturable: inside a stream capture it is refused (MRCA_ERR_INVALID).  Never more than
 *   max_rounds launches; max_rounds 0 = T (64 + 252) + 2 for T tiles per goal (derived at plan_round_bound,
 *   csrc/mrca_planner_device.h; the shipped Stage-2 map takes some tens).  Not converged within that: MRCA_ERR_UNSUPPORTED, the
 *   message names max_rounds, and every word of the field is then >= the true one.  rounds_out (host, may be NULL) = the launches
 *   that lowered something.  Reads the env's map only; writes nothing of the env.
 * mrca_subgoals  the PER-TICK call: asynchronous on `stream`, ONE launch (eight lanes per robot, the params travel as kernel
 *   arguments), capturable; reads MRCA_F_POSE, MRCA_F_GOAL and the head records as they stand at that point of the stream and
 *   writes nothing of the env.  Any robots_per_world, both lazy_obs values, exact and raster collision modes.
 *   params      host; NULL = mrca_planner_default_params: stride 2, inflate 7, lookahead 15, max_rounds 0.  stride must be the
 *               one the field was planned with (inflate and max_rounds are not read here)
 *   field_dev   u32[G,PH,PW] as mrca_goal_fields left it;  goals_dev f32[G,2] the same goal points
 *   slot_dev    i32[N]: which goal point robot n walks to, < 0 or >= G = none;  NULL = n % robots_per_world, needs
 *               G == robots_per_world
 *   mask_dev    u8[N] or NULL = all robots; rows whose mask byte is 0 are not touched in any output
 *   local_dev   f32[N,2] out, 8-byte aligned, not NULL;  subgoal_dev f32[N,2], dist_dev f32[N], status_dev i32[N]: out or NULL
 * Validated before the first HIP call (MRCA_ERR_INVALID): stride 1..8, inflate 0..64, lookahead 1..256, max_rounds >= 0;
 * G 1..4096; goals_dev, field_dev and local_dev not NULL; local_dev 8-byte aligned; slot_dev NULL only with
 * G == robots_per_world; a call before the env's first mrca_reset is refused. */
typedef struct mrca_planner_params {
    int32_t stride;      /* map cells per planning cell and axis, 1..8 */
    int32_t inflate;     /* [map cells] obstacles are grown by this, 0..64 */
    int32_t lookahead;   /* steps of the walk, 1..256 */
    int32_t max_rounds;  /* mrca_goal_fields: at most this many relaxation launches; 0 = the derived bound */
} mrca_planner_params;
int mrca_planner_default_params(mrca_planner_params* out);
int mrca_planner_grid(mrca_env* env, const mrca_planner_params* params /* host, NULL = defaults */, int32_t* pw_out, int32_t* ph_out);
int mrca_goal_fields(mrca_env* env, const mrca_planner_params* params /* host, NULL = defaults */,
                     const float* goals_dev /* f32[G,2] */, int32_t G, uint32_t* field_dev /* u32[G,PH,PW], caller-owned */,
                     int32_t* rounds_out /* host, may be NULL */, void* stream);
int mrca_subgoals(mrca_env* env, const mrca_planner_params* params /* host, NULL = defaults */, const uint32_t* field_dev,
                  const float* goals_dev /* f32[G,2] */, int32_t G, const int32_t* slot_dev /* i32[N] or NULL */,
                  const uint8_t* mask_dev /* u8[N] or NULL */, float* local_dev /* f32[N,2] */, float* subgoal_dev /* f32[N,2] or NULL */,
                  float* dist_dev /* f32[N] or NULL */, int32_t* status_dev /* i32[N] or NULL */, void* stream);

/* mrca_subgoals WITH LINE OF SIGHT: the subgoal is the FARTHEST cell of the path, up to `reach` steps down it, that the robot's
 * planning cell sees -- so the lookahead no longer has to be short to stay on this side of the next corner.  Integers only
 * (csrc/mrca_planner_device.h, LINE OF SIGHT; tests/planner_los_ref.py restates it).  For a robot with a slot and on the grid,
 * L = params.lookahead:
 *   walk      exactly as mrca_subgoals, for up to max(L, reach) steps: the cells c_0 .. c_W (W steps taken)
 *   open      a cell in the planning grid whose field word is not 0xFFFFFFFF
 *   visible   visible(c_0, c_m): the integer supercover line between the two cell centres.  dx = |di|, dy = |dj|, err = dx - dy,
 *             then dx and dy doubled; err > 0: step in x, err -= dy; err < 0: step in y, err += dx; err == 0 (the line passes
 *             exactly through a lattice corner): both side cells (i + sx, j) and (i, j + sy) must be open -- the walk's
 *             no-corner-cut rule -- then step diagonally, err += dx - dy.  Every cell entered must be open, the last one
 *             included; c_0 itself is not tested
 *   choose    m_vis = the LARGEST m in 1..W with visible(c_0, c_m), or 0 (visibility along a path is not monotone: the largest,
 *             not the last before the first failure);  m = max(m_vis, min(L, W)): never nearer than mrca_subgoals' subgoal
 *   outputs   local_dev, subgoal_dev, dist_dev, status_dev exactly as mrca_subgoals gives them for a walk that ended in c_m
 *             (status 1 with the goal point's bits at the seed; -1 / -2 with MRCA_F_GOAL);  ahead_dev[n] = (m, m_vis), (0, 0) for
 *             status -1 / -2 and for W = 0
 * Two consequences: reach <= lookahead gives mrca_subgoals' four outputs bit for bit; and where D(c_0) is finite and W >= 1,
 * m_vis >= 1.  Line of sight is from the CELL CENTRE, not from the robot's exact position (that keeps the rule in integers);
 * other robots are not obstacles; one map for all worlds.
 *   los_params  host; NULL = mrca_los_default_params: reach 60 (6 m on the default 0.1 m planning cells: the lidar's range)
 *   ahead_dev   i32[N,2] out or NULL;  every other argument as mrca_subgoals
 * Asynchronous on `stream`, ONE launch (the walk as mrca_subgoals, its cells kept in LDS, then the robot's lanes test candidates
 * from the far end; a wavefront per robot up to 8192 robots, eight lanes beyond: the same outputs), capturable; writes nothing of
 * the env.  Validated before the first HIP call
 * (MRCA_ERR_INVALID): mrca_subgoals' table, then reach 1..256, then mrca_subgoals' pointers and ahead_dev's alignment. */
typedef struct mrca_los_params {
    int32_t reach;       /* steps of the path the line of sight may skip to, 1..256 */
} mrca_los_params;
int mrca_los_default_params(mrca_los_params* out);
int mrca_subgoals_los(mrca_env* env, const mrca_planner_params* params /* host, NULL = defaults */,
                      const mrca_los_params* los_params /* host, NULL = defaults */, const uint32_t* field_dev,
                      const float* goals_dev /* f32[G,2] */, int32_t G, const int32_t* slot_dev /* i32[N] or NULL */,
                      const uint8_t* mask_dev /* u8[N] or NULL */, float* local_dev /* f32[N,2] */, float* subgoal_dev /* f32[N,2] or NULL */,
                      float* dist_dev /* f32[N] or NULL */, int32_t* status_dev /* i32[N] or NULL */,
                      int32_t* ahead_dev /* i32[N,2] or NULL */, void* stream);

/* (mrca_goal_fields above synchronises its stream too, while it looks for convergence.)
 * Synchronises `stream` and reports (then clears) the env's sticky device-side status word: MRCA_OK, or MRCA_ERR_HIP with
 * mrca_last_error() saying what went wrong on the device since the last check.  Today one condition: the ordered
 * collision pass of a world with more than 64 robots ran out of its (very long) bounded wait and left a robot
 * undecided.  mrca_step itself never synchronises; call this wherever a host round trip is acceptable (end of an
 * evaluation, once per PPO update). */
int mrca_check(mrca_env* env, void* stream);

/* Zero-copy access to a field: device pointer, byte offset inside the arena and byte size. */
int mrca_get_field(mrca_env* env, int field, void** ptr_dev_out, size_t* offset_out, size_t* bytes_out);

/* Replaces: generate_train_data (model/ppo.py:122-139) -- reverse GAE scan, one thread per robot.
 *   rewards_dev f32[T,N], values_dev f32[T,N], last_value_dev f32[N], dones_dev u8[T,N]
 *   targets_dev f32[T,N], advs_dev f32[T,N] */
int mrca_gae(const float* rewards_dev, const float* values_dev, const float* last_value_dev,
             const uint8_t* dones_dev, float gamma, float lam, int32_t T, int32_t N,
             float* targets_dev, float* advs_dev, void* stream);

/* Diagnostics */
int mrca_abi_version(void);
const char* mrca_last_error(void);
/* Per-kernel timing: the move launch and the ray-cast launch of a timed step are stamped with their own BEGIN and END
 * (hipExtLaunchKernel's start / stop events: the dispatch's timestamps, what rocprofv3 reports -- event records AROUND a
 * launch read ~2.5 us longer per kernel), up to 1024 steps between reads.
 * mrca_read_timing synchronises on the last recorded event, returns the summed durations of the
 * recorded launches in milliseconds and clears the ring. */
int mrca_enable_timing(mrca_env* env, int32_t on); /* on = n > 0: time every n-th step; 0: off */
int mrca_read_timing(mrca_env* env, float* move_ms_total, float* ray_ms_total, int32_t* launches);
/* Mean microseconds an event pair on `stream` reads with nothing between its two records (`samples` pairs, each
 * synchronised): the marker time every (event, kernel, event) figure of mrca_read_timing contains once per kernel. */
int mrca_event_pair_overhead(void* stream, int32_t samples, float* us_out);
/* Rollout-path front end of the lidar actor-critic (model/net.py:19-25,37-49,57-69: Conv1d(3,32,k5,s2,p1) -> ReLU ->
 * Conv1d(32,32,k3,s2,p1) -> ReLU for the actor and the critic tower), fused into one kernel: fp32 in, fp32 MFMA
 * accumulate, the 32 x 255 intermediate never leaves the CU.
 *   obs_dev  f32[N,3,512]   the observation stacks: MRCA_F_OBS (deque order) with obs_head_dev = NULL, or a ring with
 *                           obs_head_dev = its head slots (u8[N]): the kernel then reads frame f of robot n from slot
 *                           (head[n] + 1 + f) mod 3 while staging
 *   raw_scans               0: obs_dev holds normalised observations; 1: it holds RAW ranges (MRCA_F_SCAN_RING with
 *                           MRCA_F_RING_HEAD) and the kernel applies x / 6 - 0.5 (stage_world1.py:140) while staging --
 *                           bit-identical to reading the materialised MRCA_F_OBS
 *   w1_dev   f32[2,32,3,5]  b1_dev f32[2,32]    act_fea_cv1 / crt_fea_cv1 weight and bias, tower-major
 *   w2_dev   f32[2,32,32,3] b2_dev f32[2,32]    act_fea_cv2 / crt_fea_cv2
 *   feat_dev f32[2,N,4096]  out: tower-major, each row in the flatten order of [32,128] (what act_fc1 / crt_fc1 eat)
 * frames must be 3 and beams 512 (MRCA_ERR_UNSUPPORTED otherwise). */
int mrca_lidar_features(const float* obs_dev, const uint8_t* obs_head_dev, int32_t raw_scans, int32_t n_robots,
                        int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev,
                        float* feat_dev, void* stream);
/* The same with the stacks addressed THROUGH A ROW TABLE instead of gathered: frames_dev is a matrix of normalised frames
 * f32[*,512] and rows_dev i32[n_samples,3] the row of each sample's three frames, oldest first.  What the PPO update reads of a
 * rollout buffer that stores ONE frame per tick (model/ppo.py:143-194 indexes obs_batch[sampler]; here the stack of (tick t,
 * robot i) is three rows of the frame store, mrca/ppo.py FrameRows): the minibatch's [n,3,512] copy -- 100 MB written and read
 * per 16 384 samples -- is never made.  Same arithmetic, same results bit for bit. */
int mrca_lidar_features_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples, int32_t frames, int32_t beams,
                             const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev, float* feat_dev,
                             void* stream);

/* bf16 form of mrca_lidar_features (same inputs; frames 3, beams 512, else MRCA_ERR_UNSUPPORTED) on bf16 MFMAs
 * (csrc/mrca_policy_bf16.hip), the front end of the opt-in bf16 rollout inference.  Rounding points, each round to nearest
 * even: (1) the observation (raw ranges: x / 6 - 0.5 formed in fp32 as mrca_lidar_features does) to bf16; (2) w1, w2 to bf16,
 * b1, b2 stay fp32 and are added to the fp32 accumulators; (3) h1 = relu(conv1 + b1) to bf16 (never leaves the CU);
 * (4) feat = relu(conv2 + b2) to bf16.  feat_dev = bf16 bit patterns [2][N][4096] (tower-major, the flatten order of
 * [32,128]); obs_dev, w1_dev, w2_dev and feat_dev 16-byte aligned (MRCA_ERR_INVALID otherwise).  Deterministic (no atomics).
 * Arguments are validated before the first HIP call. */
int mrca_lidar_features_bf16(const float* obs_dev, const uint8_t* obs_head_dev, int32_t raw_scans, int32_t n_robots,
                             int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                             const float* b2_dev, uint16_t* feat_dev, void* stream);

/* The two front ends with a PER-ROBOT SCAN SCALE: the safe policy of hybrid control in the paper's form (mrca_hybrid_plan above)
 * in the same single forward as everybody else's -- no second pass, no gathered copy of the stacks, no scaled ring in memory.
 * RAW RING FORM ONLY: obs_dev = MRCA_F_SCAN_RING, obs_head_dev = MRCA_F_RING_HEAD (normalised observations cannot be rescaled
 * without undoing the normalisation; the row-table form belongs to the update).  scale_dev f32[N].  The rule is ONE separately
 * rounded fp32 multiply in front of x / 6 - 0.5, for every beam of ALL THREE frames of robot n; with x = |raw range|:
 *     x' = x < 6.0f ? x * scale[n] : x;      obs = x' / 6 - 0.5
 * Our reading of the paper's "scaled scan": a beam that returned nothing (exactly 6.0, the lidar's range) stays "nothing", a
 * return at r is seen at r s; and the whole stack is scaled by the CURRENT tick's factor, so that the three frames stay mutually
 * consistent (a robot entering the safe mode sees no jump between frames).  With scale[n] == 1.0f every bit of feat equals
 * mrca_lidar_features' / mrca_lidar_features_bf16's on the same ring (x * 1.0f == x for every finite x).  In the bf16 form the
 * multiply happens in fp32 before rounding point (1); the rounding points are otherwise those of mrca_lidar_features_bf16.
 * obs_head_dev == NULL or scale_dev == NULL: MRCA_ERR_INVALID; frames 3 and beams 512, else MRCA_ERR_UNSUPPORTED; alignment as
 * the calls above.  scale_dev is NOT validated on the device: its producer (mrca_hybrid_plan) guarantees 0 < s <= 1. */
int mrca_lidar_features_scaled(const float* obs_dev, const uint8_t* obs_head_dev, const float* scale_dev, int32_t n_robots,
                               int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                               const float* b2_dev, float* feat_dev, void* stream);
int mrca_lidar_features_bf16_scaled(const float* obs_dev, const uint8_t* obs_head_dev, const float* scale_dev, int32_t n_robots,
                                    int32_t frames, int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                    const float* b2_dev, uint16_t* feat_dev, void* stream);

/* The rest of the rollout inference behind fc1 in one kernel (model/net.py:41-55,61-70: ReLU, cat with goal and speed,
 * fc2 + ReLU of both towers, actor1 / actor2 / critic heads with sigmoid / tanh; model/ppo.py:57-82 generate_action:
 * a = mean + exp(logstd) * noise, log-density, clip to the action bounds).  fp32, exact-fp32 MFMA for fc2.
 *   h1_dev    f32[2,N,256]  act_fc1 / crt_fc1 outputs before the ReLU (tower-major)
 *   fc1_b_dev f32[2,256]    act_fc1.bias, crt_fc1.bias: added while h1 is staged -- or NULL when h1 already includes them
 *   goal_dev  f32[N,2]  speed_dev f32[N,2]          MRCA_F_LOCAL_GOAL, MRCA_F_SPEED
 *   fc2_w_dev f32[2,260,128] (input-major: act_fc2.weight^T, crt_fc2.weight^T)   fc2_b_dev f32[2,128]
 *   head_w_dev f32[128,2] (columns actor1.weight, actor2.weight)  head_b_dev f32[2]  critic_w_dev f32[128]  critic_b_dev f32[1]
 *   logstd_dev f32[2]   noise_dev f32[N,2] standard normal draws, or NULL: the deterministic mean action
 *                       (generate_action_no_sampling, model/ppo.py:84-107)
 *   lo_dev, hi_dev f32[2]   the action bounds (ppo_stage1.py:170)
 *   out: value_dev f32[N], action_dev f32[N,2] (UNclipped sample: what the rollout buffer stores), logprob_dev f32[N],
 *        scaled_dev f32[N,2] (clipped: what drives the robot), mean_dev f32[N,2] */
int mrca_policy_tail(const float* h1_dev, const float* fc1_b_dev, const float* goal_dev, const float* speed_dev, int32_t n_robots,
                     const float* fc2_w_dev, const float* fc2_b_dev, const float* head_w_dev, const float* head_b_dev,
                     const float* critic_w_dev, const float* critic_b_dev, const float* logstd_dev, const float* noise_dev,
                     const float* lo_dev, const float* hi_dev, float* value_dev, float* action_dev, float* logprob_dev,
                     float* scaled_dev, float* mean_dev, void* stream);

/* Backward pass of the same front end for the PPO update (model/ppo.py:158-192 back-propagates the loss through
 * act_fea_cv1/2 and crt_fea_cv1/2 of model/net.py:19-25 for every minibatch): given the gradient with respect to the
 * forward kernel's output it returns the gradients of both towers' convolution weights and biases; h1 is recomputed,
 * g1 never leaves the registers, per-wave partial sums are added in a fixed order (deterministic).
 *   obs_dev   f32[N,3,512]   the minibatch's observation stacks (no gradient: data)
 *   w1_dev f32[2,32,3,5]  b1_dev f32[2,32]  w2_dev f32[2,32,32,3]      the weights the forward ran with
 *   feat_dev  f32[2,N,4096]  the forward's output (its sign pattern is the second ReLU's mask)
 *   gfeat_act_dev, gfeat_crt_dev  f32[N,4096] each: dLoss / dfeat of the actor and of the critic tower (two buffers:
 *                            they are the outputs of two independent fc1 backward GEMMs)
 *   dw1_dev f32[2,32,3,5]  db1_dev f32[2,32]  dw2_dev f32[2,32,32,3]  db2_dev f32[2,32]   out (overwritten)
 *   scratch_dev              caller-owned device scratch of at least mrca_lidar_features_backward_scratch() bytes
 *                            on the CURRENT device */
int mrca_lidar_features_backward_scratch(size_t* bytes_out);
int mrca_lidar_features_backward(const float* obs_dev, int32_t n_robots, int32_t frames, int32_t beams,
                                 const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* feat_dev,
                                 const float* gfeat_act_dev, const float* gfeat_crt_dev, float* dw1_dev, float* db1_dev,
                                 float* dw2_dev, float* db2_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
/* ... and its row-table form (see mrca_lidar_features_rows): frames_dev f32[*,512], rows_dev i32[n_samples,3]. */
int mrca_lidar_features_backward_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples, int32_t frames,
                                      int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                      const float* feat_dev, const float* gfeat_act_dev, const float* gfeat_crt_dev, float* dw1_dev,
                                      float* db1_dev, float* dw2_dev, float* db2_dev, void* scratch_dev, size_t scratch_bytes,
                                      void* stream);

/* The bf16 front end of the opt-in fused bf16 PPO UPDATE (not the reference's precision; fp32 is the default).
 * Forward: mrca_lidar_features_bf16 with the scans addressed through a row table (see mrca_lidar_features_rows; frames_dev
 * f32[*,512] NORMALISED, rows_dev i32[n_samples,3]) -- the rounding points (1)-(4) of mrca_lidar_features_bf16 and the same
 * device code, so with both bf16 flags on the update re-evaluates the policy at the precision the rollout acted with.
 * Same results bit for bit as mrca_lidar_features_bf16 on the gathered stacks. */
int mrca_lidar_features_bf16_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples, int32_t frames,
                                  int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                  const float* b2_dev, uint16_t* feat_dev, void* stream);
/* Backward of the bf16 front end on v_mfma_f32_32x32x16_bf16 (csrc/mrca_policy_bf16_bwd.hip).  Numerical contract -- every
 * rounding is to nearest even by a plain cast, every accumulation fp32, parameters and gradients fp32, roundings are
 * straight-through (no gradient term for a rounding):
 *   in   feat_dev bf16[2,N,4096] the forward's output; gfeat_act_dev / gfeat_crt_dev bf16[N,4096]: fc1's dgrad g * W, formed
 *        from bf16 operands with fp32 accumulation and STORED as bf16 (the caller's rounding point)
 *   (1)  g2 = gfeat * (feat > 0): exact
 *   (2)  h1 is recomputed exactly as the forward forms it (bf16 observation and w1, fp32 b1, relu, rounded to bf16)
 *   (3)  dw2 = sum g2 * h1 and db2 = sum g2: fp32 sums of exact products
 *   (4)  dh1 = sum w2 * g2 with w2 rounded to bf16: fp32; g1 = dh1 * (h1 > 0) is rounded to bf16
 *   (5)  dw1 = sum g1 * x (the bf16 observation) and db1 = sum g1: fp32 sums of exact products
 *   per-wave partial sums are added in a fixed order in float64: run-to-run bit-identical, no atomics.
 * obs_dev f32[N,3,512] NORMALISED observations (or frames_dev / rows_dev: the row-table form); w1_dev, b1_dev, w2_dev the fp32
 * weights the forward ran with; outputs and scratch as mrca_lidar_features_backward (the scratch size is this kernel's own:
 * mrca_lidar_features_bf16_backward_scratch).  obs, w1, w2, feat and the two gfeat 16-byte aligned, everything else 4-byte
 * (MRCA_ERR_INVALID); frames 3, beams 512 (MRCA_ERR_UNSUPPORTED).  Arguments are validated before the first HIP call. */
int mrca_lidar_features_bf16_backward_scratch(size_t* bytes_out);
int mrca_lidar_features_bf16_backward(const float* obs_dev, int32_t n_robots, int32_t frames, int32_t beams, const float* w1_dev,
                                      const float* b1_dev, const float* w2_dev, const uint16_t* feat_dev,
                                      const uint16_t* gfeat_act_dev, const uint16_t* gfeat_crt_dev, float* dw1_dev, float* db1_dev,
                                      float* dw2_dev, float* db2_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
int mrca_lidar_features_bf16_backward_rows(const float* frames_dev, const int32_t* rows_dev, int32_t n_samples, int32_t frames,
                                           int32_t beams, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                                           const uint16_t* feat_dev, const uint16_t* gfeat_act_dev, const uint16_t* gfeat_crt_dev,
                                           float* dw1_dev, float* db1_dev, float* dw2_dev, float* db2_dev, void* scratch_dev,
                                           size_t scratch_bytes, void* stream);

/* The loss tail of the PPO update, values AND gradients, in one launch (model/ppo.py:172-185 / :238-251: importance ratio,
 * clipped surrogate, value loss x value_coef, entropy bonus; log-density of model/utils.py:90-97) -- what PyTorch runs as
 * ~30 element-wise launches forward and as many backward per minibatch.
 *   mean_dev f32[n,2]  value_dev f32[n]  logstd_dev f32[2]      the network's outputs for the minibatch
 *   action_dev f32[n,2]  old_logprob_dev f32[n]  adv_dev f32[n]  target_dev f32[n]      the minibatch's stored rows
 *   out_dev f32[8]:  loss, policy loss, value loss, entropy, k3 estimate of KL(old || new), dloss/dlogstd[0], [1], 0
 *   gmean_dev f32[n,2] = dloss/dmean,  gvalue_dev f32[n] = dloss/dvalue      (autograd's tie rules for min / clamp)
 *   scratch_dev: caller-owned, at least mrca_ppo_loss_scratch() bytes, ZEROED ONCE before its first use (a launch leaves
 *   it ready for the next); sums are combined in a fixed order: bit-identical from run to run. */
int mrca_ppo_loss_scratch(size_t* bytes_out);
int mrca_ppo_loss(const float* mean_dev, const float* value_dev, const float* logstd_dev, const float* action_dev,
                  const float* old_logprob_dev, const float* adv_dev, const float* target_dev, int32_t n, float clip_value,
                  float value_coef, float coeff_entropy, float* out_dev, float* gmean_dev, float* gvalue_dev,
                  void* scratch_dev, size_t scratch_bytes, void* stream);

/* One optimiser step of the PPO update on flat buffers, one launch: torch.optim.Adam's rule (ppo_stage1.py:176 Adam(lr);
 * one step per minibatch, model/ppo.py:187-189) with no weight decay and no amsgrad --
 *     m <- m + (g - m)(1 - beta1),  v <- v beta2 + (1 - beta2) g g,
 *     p <- p - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * in fp32, the bias corrections formed in double.
 *   param_dev, exp_avg_dev, exp_avg_sq_dev  f32[n]  updated in place;  grad_dev f32[n];  all four 16-byte aligned
 *   step  the number of THIS step, starting at 1 */
int mrca_adam_step(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                   double lr, double beta1, double beta2, double eps, int32_t step, void* stream);

/* The three output heads of the actor-critic in the PPO update (model/net.py:47-55,61-63: mean = [sigmoid(actor1(a)),
 * tanh(actor2(a))], value = critic(c); three Linear(128, 1)), forward and backward, as row operations instead of ~25 library
 * launches per minibatch.
 *   a_dev, c_dev  f32[n,128]  the actor / critic tower's features (act_fc2 / crt_fc2 outputs after their ReLU), 16-byte aligned
 *   w_*_dev f32[128], b_*_dev f32[1]   actor1 / actor2 / critic weight rows and biases (any 4-byte alignment)
 *   relu_inputs   1: a_dev / c_dev are fc2's outputs BEFORE their ReLU -- it is applied as they are loaded, and its mask to
 *                 da_dev / dc_dev on the way back (which are then the gradients of those pre-activations); 0: as given
 *   out: mean_dev f32[n,2], value_dev f32[n] */
int mrca_policy_heads(const float* a_dev, const float* c_dev, int32_t n, const float* w_actor1_dev, const float* b_actor1_dev,
                      const float* w_actor2_dev, const float* b_actor2_dev, const float* w_critic_dev, const float* b_critic_dev,
                      int32_t relu_inputs, float* mean_dev, float* value_dev, void* stream);
/* ... and its backward pass: given dLoss/dmean (gmean_dev f32[n,2] or NULL = zero) and dLoss/dvalue (gvalue_dev f32[n] or
 * NULL) and the forward's mean_dev, the feature gradients da_dev, dc_dev f32[n,128] and dw_dev f32[387] = dW actor1[128],
 * dW actor2[128], dW critic[128], db actor1, db actor2, db critic (per-wave partial sums added in a fixed order in float64:
 * deterministic).  scratch_dev: caller-owned, at least mrca_policy_heads_backward_scratch() bytes, 16-byte aligned. */
int mrca_policy_heads_backward_scratch(size_t* bytes_out);
int mrca_policy_heads_backward(const float* a_dev, const float* c_dev, const float* mean_dev, const float* gmean_dev,
                               const float* gvalue_dev, int32_t n, const float* w_actor1_dev, const float* w_actor2_dev,
                               const float* w_critic_dev, int32_t relu_inputs, float* da_dev, float* dc_dev, float* dw_dev,
                               void* scratch_dev, size_t scratch_bytes, void* stream);
/* The same, and dz_bias_dev f32[256] = the column sums of da_dev [0,128) and dc_dev [128,256): with relu_inputs = 1 the gradients
 * of act_fc2.bias / crt_fc2.bias, the layers whose outputs a_dev / c_dev are (model/net.py:45,59) -- summed where da / dc are
 * formed, in the same fixed order, instead of by a reduction over the two matrices just written. */
int mrca_policy_heads_backward_bias(const float* a_dev, const float* c_dev, const float* mean_dev, const float* gmean_dev,
                                    const float* gvalue_dev, int32_t n, const float* w_actor1_dev, const float* w_actor2_dev,
                                    const float* w_critic_dev, int32_t relu_inputs, float* da_dev, float* dc_dev, float* dw_dev,
                                    float* dz_bias_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* out[n,260] = [relu(h1[n,256]), goal[n,2], speed[n,2]]: F.relu(act_fc1(a)) and torch.cat((a, goal, speed), dim=-1) of
 * model/net.py:43-45 (the critic tower alike, :57-59) in one launch, and its backward dh1[n,256] = gout[:, :256] where h1 > 0
 * (goal and speed are data).  h1 / out / gout / dh1 16-byte aligned, goal / speed 8-byte. */
int mrca_relu_cat(const float* h1_dev, const float* goal_dev, const float* speed_dev, int32_t n, float* out_dev, void* stream);
int mrca_relu_cat_backward(const float* h1_dev, const float* gout_dev, int32_t n, float* dh1_dev, void* stream);
/* ... with db_dev f32[256] = the column sums of dh1: the gradient of the bias of the fc1 layer that produced h1 (model/net.py:41,57),
 * per-workgroup sums added in a fixed order in float64 (deterministic).  scratch_dev: caller-owned, at least
 * mrca_relu_cat_backward_bias_scratch() bytes, 16-byte aligned. */
int mrca_relu_cat_backward_bias_scratch(size_t* bytes_out);
int mrca_relu_cat_backward_bias(const float* h1_dev, const float* gout_dev, int32_t n, float* dh1_dev, float* db_dev,
                                void* scratch_dev, size_t scratch_bytes, void* stream);

/* The learner's rollout buffer, written by the library: what the reference appends to `buff` every step and turns into arrays
 * before the update (ppo_stage1.py:102-103; model/ppo.py:22-54 transform_buffer), kept on the device with ONE lidar frame per
 * tick (the stack at tick t shares F - 1 frames with the stack at t - 1) plus, per tick and robot, the rows of `frames` that
 * make up its stack (a robot that restarted: F times its fresh scan, ppo_stage1.py:59-60).  All pointers are device memory of
 * the caller (mrca/ppo.py RolloutBuffer); T = horizon, N / F / B = the env's robots / frames / beams. */
typedef struct mrca_rollout_rows {
    float* frames;     /* f32[T + F - 1][N][B]   rows 0 .. F-2: the older frames of the first tick's stacks (the caller's) */
    int64_t* fidx;     /* i64[T][N][F]           rows of `frames` that are the stack of (tick, robot), oldest first */
    int64_t* cur;      /* i64[N][F]              the same for the tick being stored (carried from tick to tick) */
    float* goal;       /* f32[T][N][2]  MRCA_F_LOCAL_GOAL */
    float* speed;      /* f32[T][N][2]  MRCA_F_SPEED */
    float* action;     /* f32[T][N][2]  the UNclipped sample (model/ppo.py:75) */
    float* logprob;    /* f32[T][N] */
    float* value;      /* f32[T][N] */
    float* reward;     /* f32[T][N] */
    uint8_t* done;     /* u8[T][N] */
    int32_t horizon;   /* T */
} mrca_rollout_rows;

/* Row *tick_dev of the buffer BEFORE the env steps, one launch: the newest observation frame x / 6 - 0.5 from the env's scan
 * ring into frames[t + F - 1], the stack's row indices (tick 0: rows 0 .. F-1), the env's local goal and speed, and the
 * policy's action_dev f32[N,2] / logprob_dev f32[N] / value_dev f32[N].  The row comes from DEVICE memory (int64[1]): no host
 * value enters the launch, a captured tick replays for every row of the horizon.  A counter outside [0, T) stores nothing and
 * sets a sticky status bit (mrca_check). */
int mrca_rollout_store_state(mrca_env* env, const mrca_rollout_rows* rows, const int64_t* tick_dev, const float* action_dev,
                             const float* logprob_dev, const float* value_dev, void* stream);
/* ... and AFTER the env stepped, one launch: MRCA_F_REWARD / MRCA_F_DONE into row *tick_dev, then *tick_dev += 1 (by the last
 * workgroup to finish).  ticket_dev: uint32[1] of the caller, zero before the first call (every call leaves it at zero). */
int mrca_rollout_store_outcome(mrca_env* env, const mrca_rollout_rows* rows, int64_t* tick_dev, uint32_t* ticket_dev,
                               void* stream);

#ifdef MRCA_PROFILING
/* PROFILING BUILD ONLY (csrc/build.sh --profiling -> libmrca_env_prof.so, used by tools/ablate.py); the product
 * library neither exports this symbol nor contains the switches.  Results are WRONG while any of bits 0-5 is
 * set: 1 = skip robot-robot lidar tests, 2 = skip the grid march, 8 / 16 / 32 = move kernel without its outline
 * test / collision loop / resets.  Launch-shape knobs (results unchanged):
 * bits 8-10 = k > 0: 1 << (k-1) beams per marching thread; bit 11: a dedicated preparation wave; bit 12: the beams of a
 * thread marched in lock step.  64 (results unchanged): the ray cast's phase stamps drain the memory queues first.
 * 0 restores the product path. */
int mrca_set_debug_flags(mrca_env* env, int32_t flags);
/* s_memtime ticks between the move kernel's phase stamps of the last launch, averaged over worlds: [0..7] = state loaded
 * and integrated | clearance + broad phase | patches in LDS | outline walks | ordered collision pass | reward / ballots
 * | restarts | stores drained; [8] = entry to end.  Every stamp drains the memory queues first. */
int mrca_debug_move_stamps(mrca_env* env, double* avg_ticks_out);
/* s_memtime stamps of the last ray-cast launch, lane 0 of wave 0 (builds the neighbour list, then marches) and of wave 1
 * (marches only): out[w * 7 + k] = mean over workgroups of stamp k - the workgroup's entry, k = entry | loads requested |
 * neighbour list built | beams marched | through the barrier | slab tests done | stores issued; out[14..16] = 0 (reserved:
 * s_memtime counters have unrelated origins across the chip, stamps of different workgroups cannot be compared). */
int mrca_debug_ray_stamps(mrca_env* env, double* out /* [17] */);
/* s_memtime ticks per robot a wave of the last mrca_lidar_features launch spent in conv1's tile pairs 0..3 (out[0..3]) and
 * conv2's tile pairs 0 / 1 (out[4], out[5]); out[6] = robots per wave; out[7] = shader clock during the loop [GHz].  See
 * tools/fwd_phases.py. */
int mrca_debug_fwd_stamps(double* out /* [8] */);
/* the same for the last mrca_lidar_features_backward launch: out[0..6] = ticks per item in: scan staged | gradient rows staged |
 * conv1 recompute | conv2 wgrad | conv2 dgrad | ReLU mask | conv1 wgrad; out[8] = items per wave; out[9] = shader clock [GHz].
 * See tools/bwd_phases.py. */
int mrca_debug_bwd_stamps(double* out /* [10] */);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MRCA_ENV_H */
