"""Crafted inputs of the ORCA and NH-ORCA rules (csrc/mrca_orca_device.h, csrc/mrca_nhorca_device.h) that the host tests
(tests/test_orca_host.py, tests/test_nhorca_host.py) and the GPU tests (tests/test_gpu_orca.py, tests/test_gpu_nhorca.py,
tests/test_gpu_orca_big.py) share -- data only -- and the ``*_expectations`` that assert what each is made for.

The host tests feed single functions of the headers: the sector reduction (``sector_rows``), the neighbour ranking
(``place_ties``), the command mapping (``COMMAND_CASES``) and NH-ORCA's two solves (``crafted_solves``: sets of LINES).  A
kernel takes none of these as they stand: it reads an env.  ``device_world`` therefore rebuilds them as ONE world -- poses and
goals that go in through reset, ``speed_gt`` values, scan rows and hit flags that are written into the env
(tests/controller_inject.py) -- in which every robot of CASES stands on one of those edges; ``crafted_solves`` cannot go onto
the device as lines, so robots whose pose, goal, scan row or neighbour produce its situations (free, at its goal, facing away,
goal to the left / right, a wall ahead; pushed at its goal, pushed forward while it should turn, pushed sideways at its goal
and a wall ahead with a push: each with a pusher robot that drives at it) stand in for all ten of them and their modes are
asserted.  A pusher's line is not the host set's line (its normal follows from ORCA's leg, not from a stated vector), so where
the host set says TRACK for the robot pushed at its goal the world's robot evades under the narrow default cone and tracks under
the wide one: ``nh_device_expectations`` states the mode per cone.  ``device_expectations``
/ ``nh_device_expectations`` assert from the restatements' diagnostics (tests/orca_ref.py, tests/nhorca_ref.py) on the fields
read back from the device that each edge occurred."""
import numpy as np

import nhorca_ref as NR
import orca_ref as R

f32 = np.float32
RADIUS = f32(R.DEFAULTS["radius"])
TOUCH = f32(2.0) * RADIUS                    # centres at exactly 2 * radius: dist2 == R2, the overlap branch (<=)
OBST = f32(R.DEFAULTS["obst_dist"])
GROWN = f32(NR.derive(NR.params())[3])     # the radius NH-ORCA's defaults grow a robot to
NH_TOUCH = f32(2.0) * GROWN
HALF_PI = f32(np.pi / 2)


def below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def above(x):
    return np.nextafter(f32(x), f32(np.inf))


# ------------------------------------------------------------------------------------------------ the host tests' inputs
def sector_rows(rng, B):
    """six (ranges, hit flags) rows of B beams: random, nothing anywhere, all equal, only robots, a tie inside sector 1, random"""
    rows = []
    for kind in range(6):
        r = rng.uniform(0.1, 6.0, B).astype(f32)
        r[rng.random(B) < 0.3] = 6.0
        hit = rng.random(B) < 0.3
        if kind == 1:
            r[:] = 6.0                                # nothing anywhere
        if kind == 2:
            r[:] = f32(1.25)                          # all equal: the lowest beam of every sector
        if kind == 3:
            hit[:] = True                             # only robots
        if kind == 4:
            per = B // 16
            r[per:2 * per] = f32(2.0)
            r[per + per // 2] = r[2 * per - 1] = f32(0.5)     # a tie inside sector 1
            hit[per:2 * per] = False
        rows.append((r, hit))
    return rows


def sector_expectations(rows, B):
    """``rows``: ``sector_rows`` of B beams"""
    r, hit = rows[4]
    assert R.sectors(r, hit, f32(3.0))[1][1] == B // 16 + B // 32          # the tie went to the lower beam
    assert all(b < 0 for _r, b in R.sectors(rows[1][0], rows[1][1], f32(6.0)))      # a row of 6.0 gives nothing, even at 6


def place_ties(xy):
    """robots 1 and 3 on one spot; 4, 5, 6 and 2 at ONE distance from robot 0, four ways (in place; len(xy) >= 7)"""
    xy[3] = xy[1]                                 # two on one spot
    xy[4] = (xy[0][0] + f32(1.0), xy[0][1])       # equal distances from robot 0, four ways
    xy[5] = (xy[0][0] - f32(1.0), xy[0][1])
    xy[6] = (xy[0][0], xy[0][1] + f32(1.0))
    xy[2] = (xy[0][0], xy[0][1] - f32(1.0))
    return xy


def tie_expectations(xy):
    order = [j for j in R.neighbours(xy, 0, 6.0, 48) if j in (2, 4, 5, 6)]
    assert order == [2, 4, 5, 6]                          # equal distances: by index


# (vx, vy, sin, cos) of the heading: still, barely still, ahead, behind, behind a little left / right, left, right, too fast, turned
COMMAND_CASES = [(0.0, 0.0, 0.0, 1.0), (5e-5, 5e-5, 0.0, 1.0), (0.5, 0.0, 0.0, 1.0), (-0.5, 0.0, 0.0, 1.0), (-0.5, 1e-3, 0.0, 1.0),
                 (-0.5, -1e-3, 0.0, 1.0), (0.0, 0.7, 0.0, 1.0), (0.0, -0.7, 0.0, 1.0), (2.0, 0.1, 0.0, 1.0), (0.3, 0.3, 1.0, 0.0)]
COMMAND_KINDS = {"still", "back", "straight", "turn"}


def crafted_solves():
    """(what, lines without the heading lines, n_static, heading angle, o, mode expected or None)"""
    vx_le_0 = (0.0, 0.0, 0.0, 1.0)                       # a static line: vx <= 0
    vx_ge_02 = (0.2, 0.0, 0.0, -1.0)                     # a robot line: vx >= 0.2
    return [
        ("free", [], 0, 0.0, (1.0, 0.0), NR.TRACK),
        ("at its goal", [], 0, 0.7, (0.0, 0.0), NR.STILL),
        ("facing away", [], 0, np.pi, (1.0, 0.0), NR.TURN),
        ("goal to the left", [], 0, 0.0, (0.0, 1.0), NR.TURN),
        ("goal to the right", [], 0, 0.0, (0.3, -1.0), NR.TURN),
        ("boxed in by a wall ahead", [vx_le_0], 1, 0.0, (1.0, 0.0), NR.STILL),
        ("pushed forward while it should turn", [vx_ge_02], 0, 0.0, (0.0, 1.0), NR.EVADE),
        ("pushed at its goal", [vx_ge_02], 0, 0.0, (0.0, 0.0), NR.TRACK),
        ("pushed sideways at its goal", [(0.0, 0.2, 1.0, 0.0)], 0, 0.0, (0.0, 0.0), NR.EVADE),
        ("wall ahead and a push", [vx_le_0, vx_ge_02], 1, 0.0, (1.0, 0.0), None),
    ]


def solve_expectations(what, want, T, mode, s2, diag, lines):
    """one of ``crafted_solves`` under track_time ``T``: the mode it is made for"""
    if want is None or T == 1.5:                 # (a cone of 1.5 rad holds some of the velocities that are outside the others)
        return
    assert mode == want, (what, T, mode, s2)
    if what == "goal to the left":
        assert diag["turn"] == 1.0
    if what == "goal to the right":
        assert diag["turn"] == -1.0
    if what == "boxed in by a wall ahead":
        assert R.violation(tuple(f32(v) for v in lines[0]), s2[0], s2[1]) <= 1e-5


def equal_distance_poses(init_table):
    """Seven robots: four of them at ONE distance from robot 0 and two on one spot (test_nhorca_host's open world)"""
    poses = np.asarray(init_table, f32).copy()
    poses[0, :2] = 0.0
    poses[4, :2], poses[5, :2], poses[6, :2], poses[2, :2] = (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)
    poses[3, :2] = poses[1, :2]
    return poses


# ------------------------------------------------------------------------------------------------ one world for the device
# Every number below is a float32 and every difference the rule takes of two of them is exact, so the distances ARE what the
# names say.  The robot behind each name (index in the world):
CASES = {
    "tie_centre": 0,         # 2, 4, 5, 6 stand 1 m from it, four ways: max_neighbors 2 cuts through the tie (2 and 4 stay)
    "tie_south": 2, "tie_east": 4, "tie_west": 5, "tie_north": 6,
    "one_spot_a": 1, "one_spot_b": 3,                                      # two robots on one spot
    "touch_a": 7, "touch_b": 8,                                            # centres exactly 2 * radius apart: overlap (<=)
    "inside_a": 9, "inside_b": 10,                                         # one ulp nearer: overlap
    "outside_a": 11, "outside_b": 12,                                      # one ulp further: no overlap
    "on_its_goal": 13,       # exactly: the preferred velocity is zero                 (crafted_solves: at its goal)
    "free": 14,              # alone, facing its goal                                  (free)
    "facing_away": 15,       #                                                         (facing away)
    "goal_left": 16, "goal_right": 17,                                     #           (goal to the left / right)
    "wall_ahead": 18,        # one return ahead at the grown radius, the goal behind it    (boxed in by a wall ahead)
    "pushed_at_goal": 19, "pusher": 20,      # on its goal, a robot drives at it from behind    (pushed at its goal)
    # the three pairs once more at twice the radius NH-ORCA's defaults grow a robot to
    "nh_touch_a": 21, "nh_touch_b": 22, "nh_inside_a": 23, "nh_inside_b": 24, "nh_outside_a": 25, "nh_outside_b": 26,
    "pushed_while_turning": 27, "pusher_behind": 28,     # its goal to the left, a robot drives at it from behind
    #                                                                                  (pushed forward while it should turn)
    "pushed_sideways_at_goal": 29, "pusher_beside": 30,  # on its goal, a robot drives at it from its right side
    #                                                                                  (pushed sideways at its goal)
    "wall_and_push": 31, "pusher_at_wall": 32,           # wall_ahead's return and goal, and a robot drives at it from behind
    #                                                                                  (wall ahead and a push)
}
N_CASES = 33
FAR = 40.0                   # the ring the other robots of the world stand on, out of everybody's neighbor_dist


def device_world(robots, beams):
    """-> dict(poses[R,3], goals[R,2], speed_gt {robot: (v, w)}, rows {robot: f32[B]}, hit {robot: bool[B]}) of ONE world"""
    assert robots >= N_CASES + 1 and beams % 16 == 0
    ang = 2.0 * np.pi * np.arange(robots) / robots
    poses = np.stack([FAR * np.cos(ang), FAR * np.sin(ang), ang + np.pi], 1).astype(f32)
    goals = (-poses[:, :2]).astype(f32)
    c = CASES

    def put(k, x, y, th, goal):
        poses[c[k]] = (x, y, th)
        goals[c[k]] = goal
    put("tie_centre", 0.0, 0.0, 0.0, (5.0, 0.0))
    put("tie_south", 0.0, -1.0, 1.5, (0.0, 5.0))
    put("tie_east", 1.0, 0.0, 3.0, (-5.0, 0.0))
    put("tie_west", -1.0, 0.0, 0.25, (5.0, 1.0))
    put("tie_north", 0.0, 1.0, -1.5, (0.0, -5.0))
    put("one_spot_a", 3.0, 12.0, 0.5, (8.0, 12.0))
    put("one_spot_b", 3.0, 12.0, -2.0, (-2.0, 12.0))
    for y, (a, b), d in ((24.0, ("touch_a", "touch_b"), TOUCH), (28.0, ("inside_a", "inside_b"), below(TOUCH)),
                         (32.0, ("outside_a", "outside_b"), above(TOUCH)), (-24.0, ("nh_touch_a", "nh_touch_b"), NH_TOUCH),
                         (-28.0, ("nh_inside_a", "nh_inside_b"), below(NH_TOUCH)),
                         (-32.0, ("nh_outside_a", "nh_outside_b"), above(NH_TOUCH))):
        put(a, 0.0, y, 0.0, (6.0, y))
        put(b, float(d), y, 3.0, (-6.0, y))
    put("on_its_goal", 16.0, 0.0, 0.75, (16.0, 0.0))
    put("free", 16.0, 8.0, 0.0, (22.0, 8.0))
    put("facing_away", 16.0, 16.0, 3.0, (22.0, 16.0))
    put("goal_left", 16.0, -8.0, 0.0, (16.0, -2.0))
    put("goal_right", 16.0, -16.0, 0.0, (16.5, -22.0))
    put("wall_ahead", -16.0, 0.0, 0.0, (-10.0, 0.0))
    put("pushed_at_goal", -16.0, 12.0, 0.0, (-16.0, 12.0))
    put("pusher", -17.0, 12.0, 0.0, (-10.0, 12.0))
    put("pushed_while_turning", 16.0, -30.0, 0.0, (16.0, -24.0))
    put("pusher_behind", 15.0, -30.0, 0.0, (22.0, -30.0))
    put("pushed_sideways_at_goal", -16.0, 24.0, 0.0, (-16.0, 24.0))
    put("pusher_beside", -16.0, 23.0, HALF_PI, (-16.0, 30.0))
    put("wall_and_push", -16.0, -12.0, 0.0, (-10.0, -12.0))
    put("pusher_at_wall", -17.0, -12.0, 0.0, (-10.0, -12.0))
    # speed_gt as it is written (v, omega): 0, -0.0 and the speed limit among the tied and the touching robots
    speed_gt = {c["tie_centre"]: (0.0, 0.0), c["tie_south"]: (-0.0, -0.0), c["tie_east"]: (1.0, 0.0), c["tie_west"]: (1.0, -1.0),
                c["tie_north"]: (0.5, 0.25), c["touch_a"]: (1.0, 0.0), c["touch_b"]: (-0.0, 0.0), c["inside_a"]: (0.0, 0.0),
                c["outside_a"]: (1.0, 0.0), c["outside_b"]: (1.0, 0.0), c["pusher"]: (1.0, 0.0), c["pushed_at_goal"]: (0.0, 0.0),
                c["pusher_behind"]: (1.0, 0.0), c["pusher_beside"]: (1.0, 0.0), c["pusher_at_wall"]: (1.0, 0.0),
                c["one_spot_a"]: (1.0, 0.0), c["one_spot_b"]: (-0.0, 0.0)}
    # scan rows: every case robot gets one (the others keep what the ray cast saw), all 6.0 but for
    per = beams // 16
    rows = {n: np.full(beams, 6.0, f32) for n in c.values()}
    hit = {n: np.zeros(beams, bool) for n in c.values()}
    r, h = rows[c["tie_centre"]], hit[c["tie_centre"]]
    r[per:2 * per] = f32(2.0)
    r[per + per // 2] = r[2 * per - 1] = f32(0.5)                         # sector 1: minima that tie -- the lower beam
    r[3 * per], r[3 * per + 1] = f32(1.0), f32(1.5)                       # sector 3: its minimum beam is a robot's: the next one
    h[3 * per] = True
    r[5 * per:6 * per] = OBST                                             # sector 5: exactly obst_dist: no constraint
    r[6 * per + per - 1] = below(OBST)                                    # sector 6: one ulp below: a constraint
    r[8 * per:9 * per] = f32(1.0)                                         # sector 8: only robots: no constraint
    h[8 * per:9 * per] = True
    rows[c["tie_east"]][:] = f32(1.25)                                    # all equal: the lowest beam of every sector, 16 lines
    hit[c["tie_west"]][:] = True                                          # only robots, all near: nothing
    rows[c["tie_west"]][:] = f32(0.75)
    # one return on the beam nearest to straight ahead, at exactly the radius NH-ORCA's defaults grow the robot to: the line
    # goes through the origin with the beam as its normal (v . beam <= 0), and the goal lies along that very beam
    rows[c["wall_ahead"]][beams // 2] = rows[c["wall_and_push"]][beams // 2] = GROWN
    bc, bs = (np.asarray(t, f32) for t in R.O.beam_table(f32, beams))
    for k in ("wall_ahead", "wall_and_push"):
        goals[c[k]] = poses[c[k], :2] + f32(4.0) * np.array([bc[beams // 2], bs[beams // 2]], f32)
    return dict(poses=poses, goals=goals, speed_gt=speed_gt, rows=rows, hit=hit)


def device_params():
    """the parameter sets the world is run under: ORCA's defaults (jitter 0), max_neighbors cutting through the tie, and a full
    list with every return counting"""
    return [R.params(), R.params(max_neighbors=2), R.params(max_neighbors=1, jitter=0.3), R.params(obst_dist=6.0, neighbor_dist=3.0)]


def _dist2(pose, a, b):
    dx, dy = f32(pose[b][0]) - f32(pose[a][0]), f32(pose[b][1]) - f32(pose[a][1])
    return R.dot(dx, dy, dx, dy)


def device_expectations(p, first, beams, pose, speed_gt, goal, rows, hit, diags, robots=None):
    """Each edge of ``device_world`` occurred: from host copies of an env's fields, for the world of ``robots`` robots (default:
    all there are) that starts at robot ``first``, and the restatement's diagnostics ``diags`` ({robot: diag}) under ``p`` (any
    of ``device_params``)."""
    c = {k: first + v for k, v in CASES.items()}
    n_cases = first + N_CASES
    xy = pose[first:first + (robots or len(pose)), :2]
    per = beams // 16
    R2 = (f32(2.0) * p["radius"]) * (f32(2.0) * p["radius"])
    # four neighbours at ONE distance, and the list cut among them by index
    d2 = [_dist2(pose, c["tie_centre"], c[k]) for k in ("tie_south", "tie_east", "tie_west", "tie_north")]
    assert len({float(v) for v in d2}) == 1 and d2[0] == 1.0
    near = R.neighbours(xy, 0, p["neighbor_dist"], p["max_neighbors"])
    assert near == [2, 4, 5, 6][:p["max_neighbors"]], near
    d = diags[c["tie_centre"]]
    assert len(d["branches"]) - d["n_static"] == min(4, p["max_neighbors"])
    # two robots on one spot; centres at 2 * radius and one ulp either side (the pairs made for the radius ``p`` has)
    assert _dist2(pose, c["one_spot_a"], c["one_spot_b"]) == 0.0
    pre = {float(TOUCH): "", float(NH_TOUCH): "nh_"}.get(float(f32(2.0) * p["radius"]))
    assert pre is not None or p["radius"] not in (RADIUS, GROWN)
    overlapping = ["one_spot_a", "one_spot_b"]
    if pre is not None:
        assert _dist2(pose, c[pre + "touch_a"], c[pre + "touch_b"]) == R2
        assert _dist2(pose, c[pre + "inside_a"], c[pre + "inside_b"]) < R2 < _dist2(pose, c[pre + "outside_a"], c[pre + "outside_b"])
        overlapping += [pre + k for k in ("touch_a", "touch_b", "inside_a", "inside_b")]
        for k in (pre + "outside_a", pre + "outside_b"):
            d = diags[c[k]]
            assert d["branches"][d["n_static"]] != R.OVERLAP and R.OVERLAP not in d["branches"], k
    for k in overlapping:
        d = diags[c[k]]
        assert d["branches"][d["n_static"]] == R.OVERLAP, k                # (the partner is the nearest: the first robot line)
    # a robot exactly on its goal: the preferred velocity is zero
    n = c["on_its_goal"]
    assert (pose[n, :2] == goal[n]).all()
    assert R.pref_velocity(p, n, 0, 0, pose[n, 0], pose[n, 1], goal[n, 0], goal[n, 1]) == (0.0, 0.0)
    # speed_gt: 0, -0.0 and the speed limit are there
    sp = speed_gt[first:n_cases, 0]
    assert (sp == p["max_speed"]).any() and (np.signbit(sp) & (sp == 0)).any() and (~np.signbit(sp) & (sp == 0)).any()
    # the scan row of the tie's centre: the sector minima
    n = c["tie_centre"]
    sec = R.sectors(rows[n], hit[n], p["obst_dist"])
    assert sec[1][1] == per + per // 2 and rows[n][2 * per - 1] == rows[n][per + per // 2]          # equal minima: the lower beam
    assert hit[n][3 * per] and rows[n][3 * per] < rows[n][3 * per + 1] and sec[3][1] == 3 * per + 1    # the minimum is a robot's
    assert sec[8][1] == -1 and sec[0][1] == -1                              # only robots; nothing
    assert rows[n][6 * per + per - 1] == below(OBST) and (rows[n][5 * per:6 * per] == OBST).all()
    if p["obst_dist"] == OBST:
        assert sec[5][1] == -1 and sec[6][1] == 6 * per + per - 1           # exactly obst_dist does not count, one ulp below does
        assert diags[n]["n_static"] == 3
    else:
        assert sec[5][1] == 5 * per and diags[n]["n_static"] == 4
    assert diags[c["tie_east"]]["n_static"] == (16 if p["obst_dist"] > 1.25 else 0)
    assert [b for _r, b in R.sectors(rows[c["tie_east"]], hit[c["tie_east"]], p["obst_dist"])] == [s * per for s in range(16)]
    assert diags[c["tie_west"]]["n_static"] == 0 and diags[c["tie_south"]]["n_static"] == 0
    assert diags[c["wall_ahead"]]["n_static"] == 1


def nh_device_params():
    return [NR.params(jitter=0.0), NR.params(jitter=0.0, max_neighbors=2), NR.params(max_neighbors=1),
            NR.params(jitter=0.0, obst_dist=6.0, neighbor_dist=3.0, track_error=0.2, track_time=1.0)]


def nh_device_expectations(p, first, mode, diags):
    """the situations of ``crafted_solves`` that the world rebuilds, under a ``p`` without jitter: the modes they are made for"""
    c = {k: first + v for k, v in CASES.items()}
    assert p["jitter"] == 0.0
    assert mode[c["on_its_goal"]] == NR.STILL and diags[c["on_its_goal"]]["o"] == (0.0, 0.0)
    assert mode[c["free"]] == NR.TRACK
    assert mode[c["facing_away"]] == NR.TURN
    assert mode[c["goal_left"]] == NR.TURN and diags[c["goal_left"]]["turn"] == 1.0
    assert mode[c["goal_right"]] == NR.TURN and diags[c["goal_right"]]["turn"] == -1.0
    if NR.derive(p)[3] == GROWN:
        assert mode[c["wall_ahead"]] == NR.STILL and diags[c["wall_ahead"]]["n_static"] == 1
    # the pushed robots.  The free solve's velocity points where the pusher's line lets it; whether that lies in the cone of
    # headings the unicycle can track decides between TRACK and EVADE, so the mode is stated per cone: track_time 0.3 (the
    # defaults: 0.3 rad either side) and track_time 1.0 (the last of ``nh_device_params``: 1 rad either side)
    narrow = p["track_time"] == NR.params()["track_time"]
    assert narrow or p["track_time"] == 1.0
    for k in ("pushed_at_goal", "pushed_sideways_at_goal"):
        assert diags[c[k]]["o"] == (0.0, 0.0), k                         # (they move although they are at their goals)
    assert mode[c["pushed_at_goal"]] == (NR.EVADE if narrow else NR.TRACK)
    assert mode[c["pushed_while_turning"]] == (NR.EVADE if narrow else NR.TRACK)
    assert mode[c["pushed_sideways_at_goal"]] == NR.EVADE
    for k in ("pushed_at_goal", "pushed_while_turning", "pushed_sideways_at_goal", "wall_and_push"):
        d = diags[c[k]]
        assert len(d["branches"]) - d["n_static"] == 1, k                  # (one robot line: the pusher's)
    assert diags[c["wall_and_push"]]["n_static"] == 1                      # (no mode is expected of it, on the host either)


def world_arrays(robots, beams):
    """``device_world`` as the fields of an env whose other robots see nothing and stand still -> (pose, speed_gt, goal, rows, hit):
    what the host tests feed the host build with"""
    w = device_world(robots, beams)
    speed_gt, rows, hit = np.zeros((robots, 2), f32), np.full((robots, beams), 6.0, f32), np.zeros((robots, beams), bool)
    for dst, src in ((speed_gt, w["speed_gt"]), (rows, w["rows"]), (hit, w["hit"])):
        for n, v in src.items():
            dst[n] = v
    return w["poses"], speed_gt, w["goals"], rows, hit
