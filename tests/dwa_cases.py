"""Crafted inputs of the DWA rule that the host test (tests/test_dwa_host.py) and the GPU test (tests/test_gpu_dwa.py) share:
robots that each take one special path through csrc/mrca_dwa_device.h, the grids on which ties decide, scan rows with a stated
number of occupied sectors, commands and goals that are no numbers -- data only -- and ``expectations`` / ``tie_expectations``,
which assert from the restatement's outputs and diagnostics (tests/dwa_ref.py) that each case stands on the edge it is named
for.  Both tests call them: the host test on what the restatement gives for the arrays below, the GPU test on what it gives for
the env's fields read back from the device.  Every case here goes onto the device as it stands (the rule reads the env's own
beam table in both)."""
import numpy as np

import dwa_ref as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, f32)), bits(np.asarray(b, f32)))


def crafted(B=192):
    """(goal, speed, rows) of robots that each take one special path; -> also their names in order"""
    per = B // 64
    open_row = np.full(B, 6.0, f32)
    names, goals, speeds, rows = [], [], [], []

    def add(name, goal, row, speed=(0.5, 0.0)):
        names.append(name)
        goals.append(goal)
        speeds.append(speed)
        rows.append(row)
    add("all_ranges_6", (4.0, 1.0), open_row.copy())
    r = open_row.copy()
    r[3 * per], r[10 * per + 1 if per > 1 else 10] = f32(-0.0), f32(0.0)
    add("ranges_0_and_minus_0", (4.0, 1.0), r)
    r = open_row.copy()
    r[20 * per:21 * per] = f32(3.0)                                      # exactly obst_dist: does not count
    r[21 * per + (1 if per > 1 else 0)] = np.nextafter(f32(3.0), f32(0.0))          # one ulp below: counts
    add("return_at_obst_dist", (4.0, -1.0), r)
    r = open_row.copy()
    r[30 * per:31 * per] = f32(2.0)
    r[30 * per] = r[30 * per + (2 if per > 1 else 0)] = f32(1.5)         # equal minima in sector 30 (one beam a sector at 64: no tie)
    add("equal_minima", (3.0, 2.0), r)
    add("goal_half_a_metre_ahead", (0.5, 0.0), open_row.copy())
    add("goal_half_a_metre_right", (0.0, -0.5), open_row.copy())
    add("goal_just_outside", (float(np.nextafter(f32(0.5), f32(1.0))), 0.0), open_row.copy())
    add("goal_dead_ahead_open", (5.0, 0.0), open_row.copy(), speed=(1.0, 0.0))
    add("boxed_in", (3.0, 1.0), np.full(B, 0.3, f32))
    add("boxed_in_goal_right", (3.0, -1.0), np.full(B, 0.3, f32))
    r = open_row.copy()
    r[32 * per] = f32(0.8)                                               # one return ahead, 0.8 m: some arcs pass, some do not
    add("post_ahead", (4.0, 0.0), r)
    r = open_row.copy()
    r[0] = f32(1.6)                                                      # 1.6 m to the right: clearance above and below the cap
    add("far_point", (4.0, 0.0), r)
    return names, np.array(goals, f32), np.array(speeds, f32), np.stack(rows)


def expectations(names, p, B, act, choice, score, d):
    """What ``crafted(B)`` is made for, asserted on the restatement's outputs (act, choice, score) and diagnostics ``d`` under the
    default params ``p``; the rows of ``crafted`` stand at the front of the arrays in the order of ``names``."""
    per = B // 64
    ix = {k: i for i, k in enumerate(names)}
    cap, nw = p["clear_cap"], p["nw"]
    # no point at all: every clearance IS the cap, everybody admissible
    i = ix["all_ranges_6"]
    assert not d["any_point"][i] and (d["beam"][i] == -1).all() and (d["clear"][i] == cap).all() and d["admissible"][i].all()
    assert np.isinf(d["px"][i]).all() and choice[i] >= 0
    # 0 and -0.0 are points AT the robot, both +0 after the rule's + 0: everything is blocked, the robot turns to the goal's side
    i = ix["ranges_0_and_minus_0"]
    assert d["beam"][i][3] == 3 * per and d["beam"][i][10] == (10 * per + 1 if per > 1 else 10)
    assert (d["px"][i][[3, 10]] == 0).all() and (d["py"][i][[3, 10]] == 0).all()
    assert not np.signbit(d["px"][i][3])                 # (the beam's cosine is positive: the range -0.0 became +0 first)
    assert not d["admissible"][i].any() and choice[i] == R.BLOCKED and same_bits(act[i], [0.0, 1.0]) and score[i] == 0
    # exactly obst_dist does not count, one ulp below does
    i = ix["return_at_obst_dist"]
    assert d["beam"][i][20] == -1 and d["beam"][i][21] == 21 * per + (1 if per > 1 else 0)
    # equal minima: the lower beam
    i = ix["equal_minima"]
    assert d["beam"][i][30] == 30 * per and int((d["beam"][i] >= 0).sum()) == 1
    # 0.5 m is AT the goal (<=), the next float is not
    for k in ("goal_half_a_metre_ahead", "goal_half_a_metre_right"):
        assert d["at_goal"][ix[k]] and choice[ix[k]] == R.AT_GOAL and same_bits(act[ix[k]], [0.0, 0.0])
    assert not d["at_goal"][ix["goal_just_outside"]] and choice[ix["goal_just_outside"]] >= 0
    # dead ahead in the open: mirror arcs have EQUAL scores, and straight on at full speed wins
    i = ix["goal_dead_ahead_open"]
    sc = d["score"][i].reshape(p["nv"], nw)
    assert same_bits(sc, sc[:, ::-1])
    assert choice[i] == (p["nv"] - 1) * nw + nw // 2 and same_bits(act[i], [1.0, 0.0])
    # boxed in: nobody admissible, the turn follows the sign of gy
    for k, turn in (("boxed_in", 1.0), ("boxed_in_goal_right", -1.0)):
        assert not d["admissible"][ix[k]].any() and choice[ix[k]] == R.BLOCKED and same_bits(act[ix[k]], [0.0, turn])
    # a post ahead: some candidates pass and some do not, and the chosen one passes
    i = ix["post_ahead"]
    assert d["admissible"][i].any() and not d["admissible"][i].all() and d["admissible"][i][choice[i]]
    # a far point: clearances on both sides of the cap among the admissible candidates
    i = ix["far_point"]
    assert (d["clear"][i] > cap).any() and ((d["clear"][i] < cap) & d["admissible"][i]).any()


# ------------------------------------------------------------------------------------------------ ties
TIE_ROW = 7                 # goal_dead_ahead_open
# grids on which ties decide (what is changed of the defaults): two mirror arcs; and, with only the clearance weighted and no
# point anywhere, ALL candidates -- of the default grid (105: a partial second round) and of 16 x 64 (16 full rounds)
TIE_GRIDS = {
    "mirror_pair": dict(nv=1, nw=2),
    "all_tie_default_grid": dict(w_goal=0.0, w_heading=0.0, w_speed=0.0),
    "all_tie_16_x_64": dict(w_goal=0.0, w_heading=0.0, w_speed=0.0, nv=16, nw=64),
}


def tie_expectations(name, act, choice, d, i=0):
    """Row ``i`` of the outputs is ``crafted()``'s row TIE_ROW under R.params(**TIE_GRIDS[name]): the lowest candidate wins."""
    if name == "mirror_pair":
        assert bits(d["score"][i])[0] == bits(d["score"][i])[1] and d["admissible"][i].all()
        assert choice[i] == 0 and same_bits(act[i], [1.0, -1.0])
    else:
        assert len(set(bits(d["score"][i]).tolist())) == 1 and d["admissible"][i].all()
        assert choice[i] == 0 and same_bits(act[i], [0.0, -1.0])


# ------------------------------------------------------------------------------------------------ sectors with a point
SECTOR_COUNTS = (0, 1, 3, 4, 5, 63, 64)    # both sides of the groups of four the kernel rolls the points in, none and all
SECTOR_GOAL = (-2.0, 2.0)                  # behind and to the left: the winner turns past the highest sectors' points, the last
#                                            to be packed, and its clearance is to them (checked with the restatement: without the
#                                            last n mod 4 packed points command or score differ at 1, 3, 5 and 63)


def sector_rows(B):
    """One row per entry of SECTOR_COUNTS with exactly that many sectors holding a return below obst_dist: the sectors are taken
    from the LEFT end (the highest lanes: their points stand last among the packed ones), the return is the sector's last beam
    in odd sectors and its first in even ones, 0.9 m in the highest sector taken and 1.4 m in the others -- near enough that the
    clearances lie below the cap and decide."""
    per = B // 64
    rows = np.full((len(SECTOR_COUNTS), B), 6.0, f32)
    for i, k in enumerate(SECTOR_COUNTS):
        taken = [63 - (j * 64) // k for j in range(k)] if 0 < k < 64 else list(range(k))
        assert len(set(taken)) == k
        for s in taken:
            rows[i, s * per + (per - 1 if s & 1 else 0)] = f32(0.9) if s == max(taken) else f32(1.4)
    return rows


def sector_expectations(d, first=0):
    for i, k in enumerate(SECTOR_COUNTS):
        assert int((d["beam"][first + i] >= 0).sum()) == k, (k, d["beam"][first + i])


# ------------------------------------------------------------------------------------------------ where the winner sits
# (what is changed of the defaults, goal): between them the winning candidate c sits in lane 0 and in lane 63 (c mod 64), in the
# first round (c < 64 of more than 64) and in the last, partial round
WINNER_SETS = [
    (dict(nv=1, nw=64), (0.0, -4.0)),                    # hard right: the lowest omega, c = 0
    (dict(nv=1, nw=64), (0.0, 4.0)),                     # hard left: the highest omega, c = 63
    (dict(), (4.0, 1.0)),                                # the default grid, 105: full speed, the last (partial) round
    (dict(), (0.6, 0.0)),                                # ... and a goal so near that a slow candidate wins: the first round
    (dict(nv=2, nw=64), (-1.0, -4.0)),
    (dict(nv=2, nw=64), (-1.0, 4.0)),
]


def winner_kinds(p, choice):
    """-> the places a robot's winning candidate takes in the kernel's deal of candidates to lanes"""
    nc = p["nv"] * p["nw"]
    kinds = set()
    if choice >= 0:
        if choice % 64 == 0:
            kinds.add("lane_0")
        if choice % 64 == 63:
            kinds.add("lane_63")
        if nc > 64 and choice < 64:
            kinds.add("first_round")
        if nc % 64 and choice >= nc - nc % 64:
            kinds.add("last_partial_round")
    return kinds


WINNER_KINDS = {"lane_0", "lane_63", "first_round", "last_partial_round"}

# ------------------------------------------------------------------------------------------------ goals and speeds that are no numbers
NAN, INF = float("nan"), float("inf")
# (name, goal, speed): a NaN in the goal makes every score a NaN (nobody admissible; the turn's side is `gy >= 0`, false for a
# NaN); a NaN speed is clamped to the window's lower end; an infinite goal gives inf - inf = NaN progress
SPECIAL = [
    ("goal_nan_x", (NAN, 1.0), (0.5, 0.0)),
    ("goal_nan_y", (1.0, NAN), (0.5, 0.0)),
    ("goal_inf", (INF, 0.0), (0.5, 0.0)),
    ("goal_minus_inf_y", (2.0, -INF), (0.5, 0.0)),
    ("speed_nan_v", (4.0, 1.0), (NAN, 0.0)),
    ("speed_nan_w", (4.0, 1.0), (0.5, NAN)),
    ("speed_inf", (4.0, 1.0), (INF, -INF)),
    ("speed_minus_0", (4.0, 1.0), (-0.0, -0.0)),
]


def special(B):
    """-> (names, goal, speed, rows): SPECIAL in the open (every range 6)"""
    return ([k for k, _g, _s in SPECIAL], np.array([g for _k, g, _s in SPECIAL], f32), np.array([s for _k, _g, s in SPECIAL], f32),
            np.full((len(SPECIAL), B), 6.0, f32))


def special_expectations(p, act, choice, d, first=0):
    ix = {k: first + i for i, (k, _g, _s) in enumerate(SPECIAL)}
    for k in ("goal_nan_x", "goal_nan_y", "goal_inf", "goal_minus_inf_y"):
        i = ix[k]
        assert not d["at_goal"][i] and np.isnan(d["score"][i]).all() and not d["admissible"][i].any() and choice[i] == R.BLOCKED, k
        assert act[i][0] == 0.0 and abs(act[i][1]) == p["max_omega"]
    assert act[ix["goal_nan_y"]][1] == -p["max_omega"] and act[ix["goal_minus_inf_y"]][1] == -p["max_omega"]
    for k in ("speed_nan_v", "speed_nan_w", "speed_inf", "speed_minus_0"):
        i = ix[k]
        assert choice[i] >= 0 and np.isfinite(act[i]).all() and np.isfinite(d["v"][i]).all() and np.isfinite(d["w"][i]).all(), k


# ------------------------------------------------------------------------------------------------ all of it, one case per robot
# where each group stands when the cases are dealt to the robots of one env (tests/test_gpu_dwa.py); a workgroup of the kernel is
# four robots, and QUAD fills one: masked out by the test, at the goal, blocked, choosing
CRAFTED_AT, SECTORS_AT, SPECIAL_AT, WINNERS_AT, QUAD_AT, N_CASES = 0, 12, 19, 27, 36, 40
QUAD = ["all_ranges_6", "goal_half_a_metre_ahead", "boxed_in", "post_ahead"]


def layout(B):
    """-> (names of ``crafted``, goal[N_CASES,2], speed[N_CASES,2], rows[N_CASES,B]); robots between the groups stand in the open"""
    names, cg, cs, cr = crafted(B)
    goal, speed, rows = np.tile(f32([4.0, 1.0]), (N_CASES, 1)), np.tile(f32([0.5, 0.0]), (N_CASES, 1)), np.full((N_CASES, B), 6.0, f32)
    assert len(names) == SECTORS_AT - CRAFTED_AT and QUAD_AT % 4 == 0 and QUAD_AT + len(QUAD) == N_CASES

    def put(at, g=None, s=None, r=None):
        for dst, src in ((goal, g), (speed, s), (rows, r)):
            if src is not None:
                dst[at:at + len(src)] = src
    put(CRAFTED_AT, cg, cs, cr)
    put(SECTORS_AT, np.tile(f32(SECTOR_GOAL), (len(SECTOR_COUNTS), 1)), None, sector_rows(B))
    _n, sg, ss, sr = special(B)
    assert SPECIAL_AT + len(sg) <= WINNERS_AT and WINNERS_AT + len(WINNER_SETS) <= QUAD_AT
    put(SPECIAL_AT, sg, ss, sr)
    put(WINNERS_AT, f32([g for _p, g in WINNER_SETS]))
    q = [names.index(k) for k in QUAD]
    put(QUAD_AT, cg[q], cs[q], cr[q])
    return names, goal, speed, rows
