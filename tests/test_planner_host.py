"""The global planner's rule (csrc/mrca_planner_device.h) compiled for the host with g++ -ffp-contract=off: the very functions the
gfx950 kernels call, held EQUAL to the NumPy / heapq restatement of tests/planner_ref.py -- the blocked mask, the field word for
word under tile relaxation in several orders and with stale halos, the walk and its four outputs bit for bit on random and
crafted poses -- the library's validation table, and the closed loop on the doorway scenario in the C oracle.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import planner_cases as PC
import planner_ref as R
import util as U
from util import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl-collision-avoidance_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "mrca_host.h"
#include "mrca_planner_device.h"
using namespace mrca;
extern "C" void shim_cellfield(const uint32_t* bits, const GridGeom* g, uint8_t* out) {
    std::vector<uint8_t> cf;
    build_cell_field(bits, g->width, g->height, g->wpr, &cf);
    memcpy(out, cf.data(), cf.size());
}
extern "C" void shim_blocked(const uint8_t* cf, const GridGeom* g, int s, int inflate, uint8_t* out) {
    const int pw = plan_cells(g->width, s), ph = plan_cells(g->height, s);
    for (int j = 0; j < ph; ++j)
        for (int i = 0; i < pw; ++i) out[j * pw + i] = plan_blocked(cf, *g, s, inflate, i, j);
}
// the field as mrca_goal_fields' first launch leaves it
extern "C" void shim_init(const uint8_t* cf, const GridGeom* g, int s, int inflate, const float* goal, uint32_t* f) {
    const int pw = plan_cells(g->width, s), ph = plan_cells(g->height, s);
    int ix, iy;
    const bool on = plan_map_cell(*g, goal[0], goal[1], &ix, &iy);
    for (int j = 0; j < ph; ++j)
        for (int i = 0; i < pw; ++i)
            f[j * pw + i] = plan_field_init(on && i == ix / s && j == iy / s, plan_blocked(cf, *g, s, inflate, i, j));
}
extern "C" int shim_tile_round(uint32_t* f, const uint32_t* halo, int pw, int ph, int ti, int tj, int sweeps) {
    std::vector<uint32_t> scratch((kPlanTile + 2) * (kPlanTile + 2));
    return plan_tile_round(f, halo, pw, ph, ti, tj, sweeps, scratch.data());
}
extern "C" long long shim_round_bound(int pw, int ph) { return plan_round_bound(pw, ph); }
extern "C" void shim_robots(const GridGeom* g, const PlannerParams* q, const uint32_t* fields, int G, const float* goals,
                            const int32_t* slot, int N, const float* pose, const float* head_sc, const float* env_goal, float* local,
                            float* sub, float* dist, int32_t* status) {
    const size_t cells = (size_t)plan_cells(g->width, q->stride) * plan_cells(g->height, q->stride);
    for (int n = 0; n < N; ++n) {
        const bool has = slot[n] >= 0 && slot[n] < G;
        const PlanResult r = plan_robot(*g, *q, has ? fields + slot[n] * cells : nullptr, has ? goals + 2 * slot[n] : nullptr,
                                        env_goal + 2 * n, pose[3 * n], pose[3 * n + 1], head_sc[2 * n], head_sc[2 * n + 1]);
        local[2 * n] = r.lx; local[2 * n + 1] = r.ly; sub[2 * n] = r.sx; sub[2 * n + 1] = r.sy; dist[n] = r.dist; status[n] = r.status;
    }
}
"""


class Geom(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("x0", "y0", "cell", "inv_cell")] + [(k, C.c_int32) for k in ("width", "height", "wpr")]


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in R.FIELDS]


def geom(grid):
    return Geom(f32(grid.x0), f32(grid.y0), f32(grid.cell), f32(1.0) / f32(grid.cell), grid.width, grid.height, grid.words_per_row)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("planner_host")
    src, so = d / "shim.cpp", d / "libplanner_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-pthread", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    lib.shim_round_bound.restype = C.c_longlong
    return lib


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def host_cellfield(shim, grid):
    cf = np.zeros((grid.height, grid.width), np.uint8)
    bits = np.ascontiguousarray(grid.bits, np.uint32)
    g = geom(grid)
    shim.shim_cellfield(ptr(bits), C.byref(g), ptr(cf))
    return cf


def host_blocked(shim, grid, s, inflate):
    pw, ph = R.grid_shape(grid, s)
    out = np.zeros((ph, pw), np.uint8)
    cf, g = host_cellfield(shim, grid), geom(grid)
    shim.shim_blocked(ptr(cf), C.byref(g), s, inflate, ptr(out))
    return out.astype(bool)


def host_field(shim, grid, p, goal, order="rows", halo_age=0, sweeps=64, rng=None, max_rounds=500):
    """mrca_goal_fields emulated on the host: rounds over all tiles in `order`, a tile's halo taken from the field as it stood
    `halo_age` rounds ago (0: as it stands now) -> (field with the walls finished, rounds that changed something)"""
    s = p["stride"]
    pw, ph = R.grid_shape(grid, s)
    cf, g = host_cellfield(shim, grid), geom(grid)
    f = np.zeros((ph, pw), np.uint32)
    goal = np.ascontiguousarray(goal, f32)
    shim.shim_init(ptr(cf), C.byref(g), s, p["inflate"], ptr(goal), ptr(f))
    tiles = [(ti, tj) for tj in range(-(-ph // 64)) for ti in range(-(-pw // 64))]
    history = [f.copy()]
    quiet = 0
    for rnd in range(max_rounds):
        todo = list(tiles)
        if order == "reversed":
            todo.reverse()
        elif order == "random":
            rng.shuffle(todo)
        halo = f if halo_age == 0 else history[max(0, len(history) - halo_age)]
        changed = 0
        for ti, tj in todo:
            changed += shim.shim_tile_round(ptr(f), ptr(halo), pw, ph, ti, tj, sweeps)
        history.append(f.copy())
        quiet = 0 if changed else quiet + 1
        if quiet >= max(1, halo_age):        # (a halo older than a launch -- older than the GPU's -- has to catch up first)
            f[f == 0xFFFFFFFE] = R.INF
            return f, rnd + 1 - quiet
    raise AssertionError("no fixed point")


def host_subgoals(shim, grid, p, fields, goals, slot, pose, head_sc, env_goal):
    N = len(pose)
    local, sub = np.full((N, 2), 7.0, f32), np.full((N, 2), 7.0, f32)
    dist, status = np.full(N, 7.0, f32), np.full(N, 7, np.int32)
    g, q = geom(grid), Params(**{k: int(p[k]) for k in R.FIELDS})
    fields, goals, slot = np.ascontiguousarray(fields, np.uint32), np.ascontiguousarray(goals, f32), np.ascontiguousarray(slot, np.int32)
    pose, head_sc, env_goal = (np.ascontiguousarray(t, f32) for t in (pose, head_sc, env_goal))
    shim.shim_robots(C.byref(g), C.byref(q), ptr(fields), len(goals), ptr(goals), ptr(slot), N, ptr(pose), ptr(head_sc), ptr(env_goal),
                     ptr(local), ptr(sub), ptr(dist), ptr(status))
    return local, sub, dist, status


def assert_outputs_equal(want, got):
    for name, w, g in zip(("local", "subgoal", "dist"), want, got):
        bad = np.argwhere(np.ascontiguousarray(w, f32).view(np.uint32) != np.ascontiguousarray(g, f32).view(np.uint32))
        assert len(bad) == 0, (name, bad[:5], w[tuple(bad[0])], g[tuple(bad[0])])
    assert np.array_equal(want[3], got[3]), np.argwhere(want[3] != got[3])[:5]


# ------------------------------------------------------------------------------------------------ the blocked mask
@pytest.mark.parametrize("which,s,inflate", [("crafted", 2, 1), ("crafted", 1, 0), ("odd", 3, 0), ("odd", 3, 4), ("odd", 8, 64),
                                             ("serpentine", 1, 1), ("doorway", 1, 4)])
def test_blocked_mask_equals_the_restatement(shim, which, s, inflate):
    grid = {"crafted": PC.crafted_grid, "odd": PC.odd_grid, "serpentine": PC.serpentine_grid,
            "doorway": lambda: S.doorway().grid}[which]()
    want = R.blocked_mask(grid, s, inflate)
    assert want.any() and (which == "odd" and inflate == 64 or not want.all())
    assert np.array_equal(host_blocked(shim, grid, s, inflate), want)


# ------------------------------------------------------------------------------------------------ the field
def test_tile_relaxation_ends_in_dijkstras_field_in_any_order_and_with_stale_halos(shim):
    rng = np.random.default_rng(11)
    grid = PC.serpentine_grid()
    p = R.params(stride=1, inflate=1)
    goal = (grid.x0 + 2.0, grid.y0 + 0.8)                       # below the lowest wall
    want = R.goal_field(grid, p, goal)
    assert (want == R.INF).any() and want[69, 35] != R.INF and want[69, 35] > 5 * 64 * 8      # many crossings of the tile border
    rounds = {}
    for order, age, sweeps in [("rows", 0, 64), ("reversed", 0, 64), ("random", 0, 64), ("rows", 1, 64), ("random", 1, 64),
                               ("random", 3, 64), ("reversed", 2, 5), ("random", 0, 1)]:
        got, rounds[(order, age, sweeps)] = host_field(shim, grid, p, goal, order, age, sweeps, rng)
        assert np.array_equal(got, want), (order, age, sweeps, np.argwhere(got != want)[:5])
    assert rounds[("rows", 1, 64)] > 1            # halos as old as the launch: what the GPU does in the worst case
    pw, ph = R.grid_shape(grid, 1)
    assert max(rounds.values()) < shim.shim_round_bound(pw, ph) == 4 * (64 + 252) + 2


@pytest.mark.parametrize("s,inflate", [(3, 0), (3, 4), (2, 1)])
def test_fields_of_the_odd_and_the_crafted_map(shim, s, inflate):
    rng = np.random.default_rng(s * 10 + inflate)
    grid = PC.odd_grid()
    p = R.params(stride=s, inflate=inflate)
    for goal in [(grid.x0 + 0.25, grid.y0 + 0.25), (grid.x0 + 12.9, grid.y0 + 6.6), (0.0, 0.0)]:
        want = R.goal_field(grid, p, goal)
        got, _r = host_field(shim, grid, p, goal, "random", 1, 64, rng)
        assert np.array_equal(got, want)
    grid, p, _blocked, fields = PC.crafted_fields()
    for k, goal in enumerate(PC.CRAFTED_GOALS):
        got, _r = host_field(shim, grid, p, goal, "reversed", 1, 64, rng)
        assert np.array_equal(got, fields[k]), k
    pcx, pcy = 45 // 2, 10 // 2
    assert fields[0][pcy, pcx] == R.INF and fields[4][pcy, pcx] == 0 and fields[4][2, 2] == R.INF      # the box cuts both ways
    assert (fields[3] == R.INF).all()                                                                # a goal off grid: no seed
    assert fields[2][39 // 2, 11 // 2] == 0 and (fields[2] != R.INF).sum() > 100                       # a blocked seed is walked to


# ------------------------------------------------------------------------------------------------ the walk and its outputs
def test_walk_and_outputs_on_crafted_poses(shim):
    grid, p, blocked, fields = PC.crafted_fields()
    names, pose, slot = PC.crafted_poses()
    env_goal = np.ascontiguousarray(PC.CRAFTED_GOALS[np.clip(slot, 0, len(PC.CRAFTED_GOALS) - 1)] + f32(0.125))
    head = PC.head_of(pose)
    want = R.subgoals(grid, p, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal, blocked)
    PC.crafted_expectations(names, want[3], want[1], want[2])
    assert_outputs_equal(want, host_subgoals(shim, grid, p, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal))
    # wherever there is no walk the subgoal is the robot's own goal
    for k in ("in_pocket", "off_grid_left", "no_slot", "slot_too_large", "to_off_grid_goal"):
        i = names.index(k)
        assert np.array_equal(want[1][i].view(np.uint32), env_goal[i].view(np.uint32))
    # lookahead 1: one step, and on the tie between E (then NE) and NE (then E) the lower direction index, E
    p1 = dict(p, lookahead=1)
    want1 = R.subgoals(grid, p1, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal, blocked)
    assert_outputs_equal(want1, host_subgoals(shim, grid, p1, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal))
    i = names.index("tie_straight_diagonal")
    gx, gy = 56 // 2, 30 // 2
    assert want1[3][i] == R.ON_PATH and tuple(want1[1][i]) == tuple(f32(v) for v in PC.centre(2 * (gx - 1) + 0.5, 2 * (gy - 1) + 0.5))
    assert want1[3][names.index("on_the_seed")] == R.ON_GOAL and want1[3][names.index("seed_within_lookahead")] == R.ON_PATH


@pytest.mark.parametrize("lookahead", [1, 6, 40])
def test_walk_and_outputs_on_random_poses(shim, lookahead):
    rng = np.random.default_rng(100 + lookahead)
    grid, p, blocked, fields = PC.crafted_fields()
    p = dict(p, lookahead=lookahead)
    pose, slot = PC.random_poses(rng, 400, grid)
    env_goal = rng.uniform(-5, 5, (400, 2)).astype(f32)
    head = PC.head_of(pose)
    want = R.subgoals(grid, p, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal, blocked)
    assert lookahead != 6 or all((want[3] == v).sum() > 5 for v in (1, 0, -1, -2))
    assert_outputs_equal(want, host_subgoals(shim, grid, p, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal))


# ------------------------------------------------------------------------------------------------ the library's own table
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.planner import PlannerParams
    assert built_lib.mrca_planner_default_params(None) == -1 and b"out is NULL" in built_lib.mrca_last_error()
    st = _lib.PlannerParamsStruct()
    assert built_lib.mrca_planner_default_params(C.byref(st)) == 0
    assert {k: getattr(st, k) for k in R.FIELDS} == R.DEFAULTS
    assert [n for n, _t in _lib.PlannerParamsStruct._fields_] == R.FIELDS and C.sizeof(st) == 16
    assert PlannerParams(stride=1).as_dict() == dict(R.DEFAULTS, stride=1)
    assert PlannerParams.from_assignments(["lookahead=20"]).lookahead == 20
    with pytest.raises(ValueError):
        PlannerParams.from_assignments(["nonsense=1"])
    pg = PlannerParams.for_grid(S.doorway().grid)
    assert (pg.stride, pg.inflate, pg.lookahead) == (1, 4, 15)
    pg = PlannerParams.for_grid(S.stage2().grid)
    assert (pg.stride, pg.inflate, pg.lookahead) == (2, 7, 15)
    # a rejected call touches nothing: `out` stands where the device buffers would (host memory -- no call gets as far as a launch)
    out = np.full(64, 7.0, f32)
    buf = C.c_void_p(out.ctypes.data)
    assert out.ctypes.data % 8 == 0

    def fields(params=None, goals=buf, G=4, field=buf):
        return built_lib.mrca_goal_fields(None, None if params is None else C.byref(params), goals, G, field, None, None)

    def subgoals(params=None, field=buf, goals=buf, G=4, local=buf):
        return built_lib.mrca_subgoals(None, None if params is None else C.byref(params), field, goals, G, None, None, local, None, None,
                                       None, None)
    err = built_lib.mrca_last_error
    for call in (fields, subgoals):
        assert call() == -1 and b"env is NULL" in err()
        assert call(goals=None) == -1 and b"goals_dev is NULL" in err()
        assert call(field=None) == -1 and b"field_dev is NULL" in err()
        for G in (0, -1, 4097):
            assert call(G=G) == -1 and b"G " in err() and b"1..4096" in err()
        assert call(G=4096) == -1 and b"env is NULL" in err()
        for k, bad, good in [("stride", (0, 9, -1), (1, 8)), ("inflate", (-1, 65), (0, 64)), ("lookahead", (0, 257), (1, 256)),
                             ("max_rounds", (-1,), (0, 1, 1 << 30))]:
            for v in bad:
                st = _lib.PlannerParamsStruct(**dict(R.DEFAULTS, **{k: v}))
                assert call(st) == -1 and k.encode() in err() and b"env is NULL" not in err(), (k, v, err())
            for v in good:
                st = _lib.PlannerParamsStruct(**dict(R.DEFAULTS, **{k: v}))
                assert call(st) == -1 and b"env is NULL" in err(), (k, v, err())
    assert subgoals(local=None) == -1 and b"local_dev is NULL" in err()
    assert subgoals(local=C.c_void_p(out.ctypes.data + 4)) == -1 and b"8-byte aligned" in err()
    pw, ph = C.c_int32(), C.c_int32()
    assert built_lib.mrca_planner_grid(None, None, C.byref(pw), C.byref(ph)) == -1 and b"env is NULL" in err()
    assert built_lib.mrca_planner_grid(None, None, None, C.byref(ph)) == -1 and b"NULL" in err()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ the closed loop
DOORWAY_PLAN = dict(radius=0.5, lookahead_m=1.0)
DOORWAY_TICKS = 900


def doorway_run(env, local_goal_fn, ticks=DOORWAY_TICKS):
    """`env` (the VecStageWorld surface on numpy arrays or tensors) driven by go_to_goal_policy at local_goal_fn(env) until every
    robot has a first result -> first_result"""
    import torch
    from mrca.evaluate import go_to_goal_policy
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    for k in range(ticks):
        a = go_to_goal_policy(as_t(env.obs), as_t(local_goal_fn(env)), as_t(env.speed)).float()
        a[:, 0] = torch.where(as_t(env.done).bool(), torch.zeros_like(a[:, 0]), a[:, 0])
        env.step(a.contiguous() if isinstance(env.obs, torch.Tensor) else a.numpy())
        if k % 25 == 24 and bool((as_t(env.first_result) != 0).all()):
            break
    return as_t(env.first_result).cpu().numpy()


def test_doorway_closed_loop_in_the_oracle():
    """One robot in the doorway scenario, in the C oracle: steered at the restatement's subgoals it goes through the door and
    reaches its goal; steered at the goal itself, as every controller was before, it does not."""
    from mrca.planner import PlannerParams
    sc = S.doorway(num_worlds=1, robots=1)
    p = R.params(**{k: v for k, v in PlannerParams.for_grid(sc.grid, **DOORWAY_PLAN).as_dict().items()})
    blocked = R.blocked_mask(sc.grid, p["stride"], p["inflate"])
    goals = np.ascontiguousarray(sc.goal_table, f32)
    fields = np.stack([R.goal_field(sc.grid, p, g, blocked) for g in goals])
    slot = np.zeros(1, np.int32)

    def planned(env):
        return R.subgoals(sc.grid, p, fields, goals, slot, env.pose, PC.head_of(env.pose), env.goal, blocked)[0]
    env = U.COracleEnv(sc)
    env.reset()
    assert doorway_run(env, planned)[0] == 1
    env = U.COracleEnv(sc)
    env.reset()
    assert doorway_run(env, lambda e: e.local_goal)[0] != 1
