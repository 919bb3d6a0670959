"""The planner's line-of-sight rule (csrc/mrca_planner_device.h: plan_visible, plan_robot_los -- what mrca_subgoals_los runs)
compiled for the host with g++ -ffp-contract=off and held EQUAL, on all five outputs, to the NumPy restatement of
tests/planner_los_ref.py: hand-made fields for the supercover line and its lattice corners, the crafted poses, random finite
cells on three maps with every branch of the choice counted, the list of reaches; the two stated consequences; the validation
table of the five new entry points; and the closed loop on the doorway scenario in the C oracle for the stand-in, DWA and hybrid
control steered at the subgoals.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import dwa_ref
import hybrid_ref
import planner_cases as PC
import planner_los_ref as LR
import planner_ref as R
import util as U
from test_planner_host import CSRC, DOORWAY_PLAN, Params, geom, ptr
from util import S

f32 = np.float32
REACHES = lambda L: [1, L - 1, L, L + 1, 16, 64, 256]

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "mrca_host.h"
#include "mrca_planner_device.h"
using namespace mrca;
extern "C" int shim_visible(const uint32_t* f, int pw, int ph, int i0, int j0, int i1, int j1) {
    return plan_visible(f, pw, ph, i0, j0, i1, j1) ? 1 : 0;
}
extern "C" void shim_robots_los(const GridGeom* g, const PlannerParams* q, int reach, const uint32_t* fields, int G, const float* goals,
                                const int32_t* slot, int N, const float* pose, const float* head_sc, const float* env_goal, float* local,
                                float* sub, float* dist, int32_t* status, int32_t* ahead) {
    const size_t cells = (size_t)plan_cells(g->width, q->stride) * plan_cells(g->height, q->stride);
    std::vector<int> path(2 * kLosMaxPath);
    const LosParams lq = {reach};
    for (int n = 0; n < N; ++n) {
        const bool has = slot[n] >= 0 && slot[n] < G;
        const LosResult o = plan_robot_los(*g, *q, lq, has ? fields + slot[n] * cells : nullptr, has ? goals + 2 * slot[n] : nullptr,
                                           env_goal + 2 * n, pose[3 * n], pose[3 * n + 1], head_sc[2 * n], head_sc[2 * n + 1], path.data());
        const PlanResult& r = o.r;
        local[2 * n] = r.lx; local[2 * n + 1] = r.ly; sub[2 * n] = r.sx; sub[2 * n + 1] = r.sy; dist[n] = r.dist; status[n] = r.status;
        ahead[2 * n] = o.m; ahead[2 * n + 1] = o.m_vis;
    }
}
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


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("planner_los_host")
    src, so = d / "shim.cpp", d / "libplanner_los_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-pthread", "-Wno-unknown-pragmas",
                    "-I", CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    return C.CDLL(str(so))


def host_subgoals_los(shim, grid, p, reach, fields, goals, slot, pose, head_sc, env_goal):
    N = len(pose)
    local, sub = np.full((N, 2), 7.0, f32), np.full((N, 2), 7.0, f32)
    dist, status, ahead = np.full(N, 7.0, f32), np.full(N, 7, np.int32), np.full((N, 2), 7, np.int32)
    g, q = geom(grid), Params(**{k: int(p[k]) for k in R.FIELDS})
    fields, goals, slot = np.ascontiguousarray(fields, np.uint32), np.ascontiguousarray(goals, f32), np.ascontiguousarray(slot, np.int32)
    pose, head_sc, env_goal = (np.ascontiguousarray(t, f32) for t in (pose, head_sc, env_goal))
    shim.shim_robots_los(C.byref(g), C.byref(q), int(reach), ptr(fields), len(goals), ptr(goals), ptr(slot), N, ptr(pose), ptr(head_sc),
                         ptr(env_goal), ptr(local), ptr(sub), ptr(dist), ptr(status), ptr(ahead))
    return local, sub, dist, status, ahead


def host_subgoals_plain(shim, grid, p, fields, goals, slot, pose, head_sc, env_goal):
    N = len(pose)
    local, sub = np.full((N, 2), 7.0, f32), np.full((N, 2), 7.0, f32)
    dist, status = np.full(N, 7.0, f32), np.full(N, 7, np.int32)
    g, q = geom(grid), Params(**{k: int(p[k]) for k in R.FIELDS})
    fields, goals, slot = np.ascontiguousarray(fields, np.uint32), np.ascontiguousarray(goals, f32), np.ascontiguousarray(slot, np.int32)
    pose, head_sc, env_goal = (np.ascontiguousarray(t, f32) for t in (pose, head_sc, env_goal))
    shim.shim_robots(C.byref(g), C.byref(q), ptr(fields), len(goals), ptr(goals), ptr(slot), N, ptr(pose), ptr(head_sc), ptr(env_goal),
                     ptr(local), ptr(sub), ptr(dist), ptr(status))
    return local, sub, dist, status


def assert_los_equal(want, got, what=""):
    """all five outputs, the floats by their bits"""
    for name, w, g in zip(("local", "subgoal", "dist"), want, got):
        bad = np.argwhere(np.ascontiguousarray(w, f32).view(np.uint32) != np.ascontiguousarray(g, f32).view(np.uint32))
        assert len(bad) == 0, (what, name, bad[:5], w[tuple(bad[0])], g[tuple(bad[0])])
    assert np.array_equal(want[3], got[3]), (what, "status", np.argwhere(want[3] != got[3])[:5])
    if len(want) > 4:
        assert np.array_equal(want[4], got[4]), (what, "ahead", np.argwhere(want[4] != got[4])[:5], want[4][:8], got[4][:8])


def cell_poses(grid, s, cells, rng):
    """poses inside the planning cells `cells` ((i, j) rows), anywhere in the cell's first map cell, any heading"""
    cells = np.asarray(cells)
    off = rng.uniform(0.05, 0.95, (len(cells), 2))
    xy = np.array([grid.x0, grid.y0]) + (cells * s + off) * grid.cell
    return np.concatenate([xy, rng.uniform(-np.pi, np.pi, (len(cells), 1))], 1).astype(f32)


# ------------------------------------------------------------------------------------------------ the line itself
def corner_field(block):
    """an empty 8 x 8 grid of 1 m cells, the cells of `block` blocked, the seed at (5, 5)"""
    grid = S.empty_grid(8, 1.0)
    p = R.params(stride=1, inflate=0, lookahead=2)
    blocked = np.zeros((8, 8), bool)
    for i, j in block:
        blocked[j, i] = True
    goal = (grid.x0 + 5.5, grid.y0 + 5.5)
    return grid, p, blocked, goal, R.goal_field(grid, p, goal, blocked)


def test_a_line_through_a_lattice_corner_needs_both_side_cells(shim):
    """(1, 1) -> (5, 5) passes exactly through four lattice corners.  With (1, 2) blocked the seed is not visible from (1, 1) --
    and the walk, which may not cut that corner either, goes round by (2, 1); with both side cells open it is."""
    rng = np.random.default_rng(3)
    for block, sees in (([(1, 2)], False), ([(2, 1)], False), ([(3, 4)], False), ([], True), ([(0, 3), (6, 2)], True)):
        grid, p, blocked, goal, D = corner_field(block)
        assert LR.visible(D, (1, 1), (5, 5)) is sees
        assert bool(shim.shim_visible(ptr(np.ascontiguousarray(D)), 8, 8, 1, 1, 5, 5)) is sees
        pose = cell_poses(grid, 1, [(1, 1)], rng)
        args = (D[None], np.array([goal], f32), np.zeros(1, np.int32), pose, PC.head_of(pose), np.array([goal], f32))
        want = LR.subgoals_los(grid, p, 8, *args, blocked)
        assert_los_equal(want, host_subgoals_los(shim, grid, p, 8, *args), block)
        m, m_vis = want[4][0]
        if sees:
            assert (m, m_vis) == (4, 4) and want[3][0] == R.ON_GOAL and np.array_equal(want[1][0].view(np.uint32), f32(goal).view(np.uint32))
        else:
            assert m_vis >= 1 and m == max(m_vis, 2) and want[3][0] == R.ON_PATH          # the seed, c_W, is not the subgoal


def test_visible_equals_the_restatement_on_every_pair_of_a_cluttered_field(shim):
    rng = np.random.default_rng(4)
    grid = S.empty_grid(12, 1.0)
    blocked = rng.random((12, 12)) < 0.2
    blocked[6, 6] = False
    D = R.goal_field(grid, R.params(stride=1, inflate=0), (grid.x0 + 6.5, grid.y0 + 6.5), blocked)
    Dc = np.ascontiguousarray(D)
    seen = [0, 0]
    for j0 in range(12):
        for i0 in range(12):
            for j1 in range(12):
                for i1 in range(12):
                    want = LR.visible(D, (i0, j0), (i1, j1))
                    seen[want] += 1
                    assert bool(shim.shim_visible(ptr(Dc), 12, 12, i0, j0, i1, j1)) is want, (i0, j0, i1, j1)
    assert min(seen) > 2000
    # c_0 itself is not tested, the last cell is
    bi, bj = [(i, j) for j in range(1, 11) for i in range(1, 11) if D[j, i] == R.INF and D[j, i + 1] != R.INF][0]
    assert LR.visible(D, (bi, bj), (bi + 1, bj)) and not LR.visible(D, (bi + 1, bj), (bi, bj))


# ------------------------------------------------------------------------------------------------ crafted poses
LOS_EXTRA = [("floor_decides", (22, 0), 0), ("sees_past_lookahead", (11, 4), 0), ("straight_to_the_end", (20, 22), 0)]


def crafted_case(rng):
    grid, p, blocked, fields = PC.crafted_fields()
    names, pose, slot = PC.crafted_poses()
    extra = cell_poses(grid, p["stride"], [c for _n, c, _s in LOS_EXTRA], rng)
    names = names + [n for n, _c, _s in LOS_EXTRA]
    pose = np.concatenate([pose, extra])
    slot = np.concatenate([slot, np.array([s for _n, _c, s in LOS_EXTRA], np.int32)])
    env_goal = np.ascontiguousarray(PC.CRAFTED_GOALS[np.clip(slot, 0, len(PC.CRAFTED_GOALS) - 1)] + f32(0.125))
    return grid, p, blocked, fields, names, pose, slot, env_goal


def crafted_los_expectations(names, want, env_goal, L, reach=64):
    """what the restatement must say about the crafted poses at lookahead 6 and reach 64: the branch each one takes"""
    _local, sub, dist, status, ahead = want
    ix = {k: i for i, k in enumerate(names)}
    row = lambda k: (int(status[ix[k]]), int(ahead[ix[k]][0]), int(ahead[ix[k]][1]))
    same = lambda a, b: np.array_equal(a.view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))
    assert row("straight_to_the_end") == (R.ON_GOAL, 8, 8)                       # an open straight run: m = W, the seed's bits
    assert same(sub[ix["straight_to_the_end"]], PC.CRAFTED_GOALS[0])
    st, m, m_vis = row("floor_decides")                                          # an inflated corner ahead: m_vis < min(L, W)
    assert st == R.ON_PATH and m_vis < L and m == L
    st, m, m_vis = row("sees_past_lookahead")
    assert st == R.ON_PATH and L < m == m_vis < reach
    assert row("seed_beyond_lookahead") == (R.ON_GOAL, 7, 7)                     # the plain walk stops a step short of it
    assert row("seed_at_lookahead") == (R.ON_GOAL, 6, 6) and row("seed_within_lookahead") == (R.ON_GOAL, 3, 3)
    assert row("on_the_seed") == (R.ON_GOAL, 0, 0) and dist[ix["on_the_seed"]] == 0.0        # W = 0
    st, m, m_vis = row("in_inflation")                                           # inside the inflation: c_0 is not tested
    assert st == R.ON_PATH and np.isinf(dist[ix["in_inflation"]]) and m >= L
    assert row("in_pocket") == (R.NO_PATH, 0, 0)                                 # no finite neighbour
    assert row("to_off_grid_goal") == (R.NO_PATH, 0, 0)
    assert row("off_grid_left") == (R.NO_PATH, 0, 0) and row("off_grid_above") == (R.NO_PATH, 0, 0)
    assert row("no_slot") == (R.NO_SLOT, 0, 0) and row("slot_too_large") == (R.NO_SLOT, 0, 0)
    for k in ("in_pocket", "off_grid_left", "no_slot", "slot_too_large", "to_off_grid_goal"):
        assert same(sub[ix[k]], env_goal[ix[k]])


def test_crafted_poses(shim):
    grid, p, blocked, fields, names, pose, slot, env_goal = crafted_case(np.random.default_rng(5))
    head = PC.head_of(pose)
    want = LR.subgoals_los(grid, p, 64, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal, blocked)
    crafted_los_expectations(names, want, env_goal, p["lookahead"])
    assert_los_equal(want, host_subgoals_los(shim, grid, p, 64, fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal))


@pytest.mark.parametrize("reach", REACHES(PC.CRAFTED_PARAMS["lookahead"]))
def test_reaches_on_crafted_and_random_poses(shim, reach):
    """every reach of the list; reach <= lookahead gives mrca_subgoals' four outputs bit for bit -- by the restatement of
    tests/planner_ref.py and by plan_robot itself"""
    rng = np.random.default_rng(200 + reach)
    grid, p, blocked, fields, _names, pose, slot, env_goal = crafted_case(rng)
    rp, rs = PC.random_poses(rng, 150, grid)
    pose, slot = np.concatenate([pose, rp]), np.concatenate([slot, rs])
    env_goal = np.concatenate([env_goal, rng.uniform(-5, 5, (150, 2)).astype(f32)])
    head = PC.head_of(pose)
    args = (fields, PC.CRAFTED_GOALS, slot, pose, head, env_goal)
    want = LR.subgoals_los(grid, p, reach, *args, blocked)
    got = host_subgoals_los(shim, grid, p, reach, *args)
    assert_los_equal(want, got, reach)
    assert all((want[3] == v).sum() > 5 for v in (1, 0, -1, -2))
    plain = R.subgoals(grid, p, *args, blocked)
    if reach <= p["lookahead"]:
        assert_los_equal(plain, got[:4], "the plain walk")
        assert_los_equal(plain, host_subgoals_plain(shim, grid, p, *args), "plan_robot")
    else:
        assert (got[4][:, 0] > p["lookahead"]).any() and not np.array_equal(plain[1], got[1])


# ------------------------------------------------------------------------------------------------ random finite cells
MAPS = {
    "crafted": lambda: (PC.crafted_grid(), R.params(**PC.CRAFTED_PARAMS), [PC.CRAFTED_GOALS[0], PC.CRAFTED_GOALS[2]]),
    "serpentine": lambda: (PC.serpentine_grid(), R.params(stride=1, inflate=1, lookahead=6), [(-8.75 + 2.0, -8.75 + 0.8)]),
    "odd": lambda: (PC.odd_grid(), R.params(stride=1, inflate=2, lookahead=15), [(-5.5, -2.5)]),
    "odd_stride3": lambda: (PC.odd_grid(), R.params(stride=3, inflate=0, lookahead=6), [(-6.55 + 12.9, -3.35 + 6.6)]),
}
_cases = {}


def random_case(which, n=400, reach=64):
    """-> (grid, p, blocked, fields, goals, pose, slot, env_goal, the restatement's outputs, per-robot (W, first failure)):
    robots in `n` random cells with a finite D, computed once per map"""
    if which not in _cases:
        rng = np.random.default_rng(sorted(MAPS).index(which) + 40)
        grid, p, goals = MAPS[which]()
        goals = np.ascontiguousarray(goals, f32)
        blocked = R.blocked_mask(grid, p["stride"], p["inflate"])
        fields = np.stack([R.goal_field(grid, p, g, blocked) for g in goals])
        slot = rng.integers(0, len(goals), n).astype(np.int32)
        cells = np.zeros((n, 2), np.int64)
        for g in range(len(goals)):
            fin = np.argwhere(fields[g] != R.INF)[:, ::-1]
            sel = np.flatnonzero(slot == g)
            cells[sel] = fin[rng.choice(len(fin), len(sel), replace=len(fin) < len(sel))]
        pose = cell_poses(grid, p["stride"], cells, rng)
        env_goal = rng.uniform(-5, 5, (n, 2)).astype(f32)
        want = LR.subgoals_los(grid, p, reach, fields, goals, slot, pose, PC.head_of(pose), env_goal, blocked)
        walks = []
        for n_, (i, j) in enumerate(cells):
            D = fields[slot[n_]]
            path, _nocand = LR.walk_cells(D, blocked, R.plan_cell(grid, p["stride"], *goals[slot[n_]]), int(i), int(j), max(p["lookahead"], reach))
            vis = [LR.visible(D, path[0], c) for c in path[1:]]
            walks.append((len(path) - 1, vis.index(False) if False in vis else len(vis)))
        _cases[which] = (grid, p, blocked, fields, goals, pose, slot, env_goal, want, np.array(walks))
    return _cases[which]


@pytest.mark.parametrize("which", sorted(MAPS))
def test_random_finite_cells_take_every_branch(shim, which):
    grid, p, blocked, fields, goals, pose, slot, env_goal, want, walks = random_case(which)
    got = host_subgoals_los(shim, grid, p, 64, fields, goals, slot, pose, PC.head_of(pose), env_goal)
    assert_los_equal(want, got, which)
    L = p["lookahead"]
    W, first_fail = walks[:, 0], walks[:, 1]
    m, m_vis = want[4][:, 0], want[4][:, 1]
    assert np.isfinite(want[2]).all() and (want[3] >= 0).all()
    # the invariant: a finite start that walks at all sees its first step
    assert (m_vis[W >= 1] >= 1).all() and (W >= 1).sum() > 390
    assert np.array_equal(m, np.maximum(m_vis, np.minimum(L, W)))
    counts = {"m_vis < W": int((m_vis < W).sum()), "the floor decides": int((m_vis < np.minimum(L, W)).sum()),
              "m_vis <= 1": int(((m_vis <= 1) & (W >= 1)).sum()), "visible after invisible": int((m_vis > first_fail + 1).sum()),
              "m = W beyond L": int(((m == W) & (W > L)).sum())}
    assert counts["m_vis < W"] >= 100 and counts["the floor decides"] >= 20 and counts["m_vis <= 1"] >= 3, counts
    assert counts["m = W beyond L"] >= 3, counts
    if which.startswith("odd"):
        assert counts["visible after invisible"] >= 10 and counts["the floor decides"] > 200, counts


# ------------------------------------------------------------------------------------------------ the library's own table
def test_default_params_and_the_validation_table(built_lib):
    from mrca import _lib
    from mrca.planner import LosParams
    err = built_lib.mrca_last_error
    assert built_lib.mrca_los_default_params(None) == -1 and b"out is NULL" in err()
    st = _lib.LosParamsStruct()
    assert built_lib.mrca_los_default_params(C.byref(st)) == 0 and st.reach == 60
    assert [n for n, _t in _lib.LosParamsStruct._fields_] == LR.LOS_FIELDS and C.sizeof(st) == 4
    assert LosParams().as_dict() == LR.LOS_DEFAULTS and LosParams(reach=7).as_dict() == {"reach": 7}
    assert LosParams.from_assignments(["reach=20"]).reach == 20
    with pytest.raises(ValueError):
        LosParams.from_assignments(["nonsense=1"])
    assert LosParams.for_grid(S.doorway().grid).reach == 60 and LosParams.for_grid(S.stage2().grid).reach == 60
    assert LosParams.for_grid(S.doorway().grid, reach_m=2.0).reach == 20 and LosParams.for_grid(PC.crafted_grid(), reach_m=100.0).reach == 256
    # a rejected call touches nothing: `out` stands where the device buffers would (host memory -- no call gets as far as a launch)
    out = np.full(64, 7.0, f32)
    buf, odd = C.c_void_p(out.ctypes.data), C.c_void_p(out.ctypes.data + 4)
    byte = C.c_void_p(out.ctypes.data + 1)
    assert out.ctypes.data % 8 == 0

    def los(params=None, lp=None, field=buf, goals=buf, G=4, local=buf, ahead=None, slot=None):
        return built_lib.mrca_subgoals_los(None, None if params is None else C.byref(params), None if lp is None else C.byref(lp), field,
                                           goals, G, slot, None, local, None, None, None, ahead, None)
    assert los() == -1 and b"env is NULL" in err()
    assert los(goals=None) == -1 and b"mrca_subgoals_los: goals_dev is NULL" in err()
    assert los(field=None) == -1 and b"field_dev is NULL" in err()
    assert los(local=None) == -1 and b"local_dev is NULL" in err()
    assert los(local=odd) == -1 and b"local_dev must be 8-byte aligned" in err()
    assert los(ahead=byte) == -1 and b"ahead_dev must be 4-byte aligned" in err()
    assert los(slot=byte) == -1 and b"slot_dev must be 4-byte aligned" in err()
    assert los(ahead=odd) == -1 and b"env is NULL" in err()
    for G in (0, -1, 4097):
        assert los(G=G) == -1 and b"G " in err() and b"1..4096" in err()
    for bad in (0, -1, 257, 1 << 20):
        assert los(lp=_lib.LosParamsStruct(reach=bad)) == -1 and b"mrca_subgoals_los: reach" in err() and b"1..256" in err(), err()
    for good in (1, 60, 256):
        assert los(lp=_lib.LosParamsStruct(reach=good)) == -1 and b"env is NULL" in err()
    for k, bad in [("stride", 9), ("inflate", 65), ("lookahead", 257), ("max_rounds", -1)]:
        stp = _lib.PlannerParamsStruct(**dict(R.DEFAULTS, **{k: bad}))
        assert los(stp) == -1 and k.encode() in err() and b"env is NULL" not in err()
        # the planner's table is read before the reach
        assert los(stp, _lib.LosParamsStruct(reach=0)) == -1 and k.encode() in err()

    # the three controllers steered at the caller's rows: their siblings' tables, and the goal's alignment
    def dwa(params=None, actions=buf, goal=buf):
        return built_lib.mrca_dwa_actions_goal(None, None if params is None else C.byref(params), None, actions, None, None, goal, None)

    def hyb(params=None, policy=buf, actions=buf, goal=buf):
        return built_lib.mrca_hybrid_actions_goal(None, None if params is None else C.byref(params), None, policy, actions, None, None, goal,
                                                  None)

    def plan(params=None, safe=None, mode=buf, scale=buf, pid=buf, goal=buf):
        return built_lib.mrca_hybrid_plan_goal(None, None if params is None else C.byref(params), None if safe is None else C.byref(safe),
                                               None, mode, scale, pid, None, goal, None)
    for call, name in ((dwa, b"mrca_dwa_actions_goal"), (hyb, b"mrca_hybrid_actions_goal"), (plan, b"mrca_hybrid_plan_goal")):
        assert call() == -1 and b"env is NULL" in err()
        assert call(goal=None) == -1 and b"env is NULL" in err()                     # NULL: MRCA_F_LOCAL_GOAL
        assert call(goal=odd) == -1 and name + b": goal_dev must be 8-byte aligned" in err()
    assert dwa(actions=None) == -1 and b"mrca_dwa_actions_goal: actions_dev is NULL" in err()
    assert dwa(actions=odd) == -1 and b"8-byte aligned" in err()
    d = _lib.DwaParamsStruct()
    assert built_lib.mrca_dwa_default_params(C.byref(d)) == 0
    d.nv = 0
    assert dwa(d) == -1 and b"mrca_dwa_actions_goal: nv" in err()
    assert hyb(policy=None) == -1 and b"mrca_hybrid_actions_goal: policy_dev is NULL" in err()
    assert hyb(actions=None) == -1 and b"actions_dev is NULL" in err()
    h = _lib.HybridParamsStruct()
    assert built_lib.mrca_hybrid_default_params(C.byref(h)) == 0
    h.stop_dist = 0.7
    assert hyb(h) == -1 and b"mrca_hybrid_actions_goal: risk_dist must be > stop_dist" in err()
    assert plan(h) == -1 and b"mrca_hybrid_plan_goal: risk_dist must be > stop_dist" in err()
    for k in ("mode", "scale", "pid"):
        assert plan(**{k: None}) == -1 and (k + "_dev is NULL").encode() in err()
    sp = _lib.SafePolicyParamsStruct(scan_scale=0.0, v_cap=0.5)
    assert plan(safe=sp) == -1 and b"mrca_hybrid_plan_goal: scan_scale" in err()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ the closed loop
DOORWAY_REACH = 60


class DoorwayPlan:
    """the doorway scenario's fields by the restatement, and per tick the subgoals of an env's robots"""

    def __init__(self, sc, lookahead=None, goals=None, slot=None):
        """goals / slot: the goal points and which one each robot walks to (default: the scenario's table, robot n to row
        n % robots_per_world)"""
        from mrca.planner import PlannerParams
        self.sc = sc
        self.p = R.params(**PlannerParams.for_grid(sc.grid, **DOORWAY_PLAN).as_dict())
        if lookahead is not None:
            self.p["lookahead"] = lookahead
        self.blocked = R.blocked_mask(sc.grid, self.p["stride"], self.p["inflate"])
        self.goals = np.ascontiguousarray(sc.goal_table if goals is None else goals, f32)
        self.fields = np.stack([R.goal_field(sc.grid, self.p, g, self.blocked) for g in self.goals])
        self.slot = (np.arange(sc.num_robots) % sc.robots_per_world).astype(np.int32) if slot is None else np.asarray(slot, np.int32)

    def plain(self, env):
        return R.subgoals(self.sc.grid, self.p, self.fields, self.goals, self.slot, env.pose, PC.head_of(env.pose), env.goal, self.blocked)[0]

    def los(self, env, reach=DOORWAY_REACH):
        return LR.subgoals_los(self.sc.grid, self.p, reach, self.fields, self.goals, self.slot, env.pose, PC.head_of(env.pose), env.goal,
                               self.blocked)[0]


def stand_in(obs, local, speed):
    import torch
    from mrca.evaluate import go_to_goal_policy
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return go_to_goal_policy(t(obs), t(local), t(speed)).float().numpy()


def cpu_controller(kind):
    """-> f(env fields, local goal) -> actions f32[N, 2]: the stand-in, DWA, or hybrid control around the stand-in, each steered
    at `local` through its restatement's goal argument, at the restatements' defaults"""
    if kind == "stand_in":
        return lambda obs, local, speed, scan: stand_in(obs, local, speed)
    if kind == "dwa":
        p = dwa_ref.params()
        return lambda obs, local, speed, scan: dwa_ref.env_actions(p, local, speed, scan)[0]
    p = hybrid_ref.params()
    return lambda obs, local, speed, scan: hybrid_ref.env_actions(p, local, stand_in(obs, local, speed), scan)[0]


def closed_loop(env, act, local_goal_fn, ticks=900):
    """drive `env` (numpy fields) until every robot has a first result -> (first_result, ticks run); a robot that is done gets
    v = 0, as the evaluator gives it"""
    for k in range(ticks):
        a = np.ascontiguousarray(act(env.obs, local_goal_fn(env), env.speed, env.scan), f32).copy()
        a[:, 0] = np.where(np.asarray(env.done).astype(bool), f32(0.0), a[:, 0])
        env.step(a)
        if (np.asarray(env.first_result) != 0).all():
            return np.asarray(env.first_result).copy(), k + 1
    return np.asarray(env.first_result).copy(), ticks


@pytest.mark.parametrize("kind", ["stand_in", "dwa", "hybrid"])
def test_doorway_closed_loop_in_the_oracle(kind):
    """One robot in the doorway scenario, in the C oracle, steered at the line-of-sight subgoals (reach 60): it goes through the
    door and reaches its goal, and sooner than at the plain subgoals."""
    sc = S.doorway(num_worlds=1, robots=1)
    plan = DoorwayPlan(sc)
    env = U.COracleEnv(sc)
    env.reset()
    result, ticks_los = closed_loop(env, cpu_controller(kind), plan.los)
    assert result[0] == 1, (kind, result, ticks_los)
    env = U.COracleEnv(sc)
    env.reset()
    result, ticks_plain = closed_loop(env, cpu_controller(kind), plan.plain)
    print(kind, "ticks: line of sight", ticks_los, "plain", ticks_plain)
    assert result[0] == 1 and ticks_los < ticks_plain, (kind, result, ticks_los, ticks_plain)


def test_a_plain_lookahead_of_60_ends_at_the_wall():
    """what the reach does is not what a longer lookahead does: 60 plain steps put the subgoal behind the wall"""
    sc = S.doorway(num_worlds=1, robots=1)
    plan = DoorwayPlan(sc, lookahead=60)
    env = U.COracleEnv(sc)
    env.reset()
    result, _ticks = closed_loop(env, cpu_controller("stand_in"), plan.plain)
    assert result[0] != 1
