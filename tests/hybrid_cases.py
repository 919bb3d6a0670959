"""Crafted inputs of the hybrid control rule (csrc/mrca_hybrid_device.h) that the host tests (tests/test_hybrid_host.py,
tests/test_safe_host.py) and the GPU tests (tests/test_gpu_hybrid.py, tests/test_gpu_safe_policy.py) share: rows that stand
exactly on each of the rule's edges, commands that are no numbers in every mode -- data only -- and ``expectations``, which
asserts from the restatement's outputs and its blocking count (tests/hybrid_ref.py) that each row took the branch it is named
for.

Two sets.  ``crafted`` is the host test's: it needs a hand-made beam table (``crafted_table``: beams 0, 1 and 2 point exactly
left, ahead and right), so that a range IS the lateral or the forward distance -- the device reads the env's own table, which
has no beam straight ahead, so the set cannot go onto the device as it stands.  ``device_cases`` rebuilds every one of its rows
on the env's table: beam 0 and beam B - 1 have a sine of exactly -1 and +1 (the corridor's edge is a range again); for any other
beam ``edge_range`` searches the floats around threshold / |component| for a range whose float32 product with the component
lands exactly on the threshold.  Its lone returns stand on beams 0, 63, 64 and B - 1 -- the first and the last lane of the
kernel's first and last round -- wherever the edge allows it (reach and look need a beam within the corridor ahead), and it adds
a row in which all B beams block."""
import numpy as np

import hybrid_ref as R

f32 = np.float32
NAN, INF = float("nan"), float("inf")

# (its own corridor, look and scale; risk_dist 0.4 so that a return on the corridor's edge, 0.45 m away, is not a risk)
PARAMS = dict(risk_dist=0.4, stop_dist=0.3, safe_scale=0.5, corridor=0.45, look=4.0)
COMMAND = (0.75, -0.25)
SPECIAL_COMMANDS = (("nan", (NAN, 0.5)), ("inf", (INF, -INF)), ("minus_0", (-0.0, -0.0)), ("nan_w", (0.5, NAN)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, f32)), bits(np.asarray(b, f32)))


def below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def above(x):
    return np.nextafter(f32(x), f32(np.inf))


def beam_table(B):
    return tuple(np.ascontiguousarray(t, f32) for t in R.O.beam_table(f32, B))


def crafted_table(B=64):
    """beam directions with three exact ones: beam 0 = (0, 1) (left), beam 1 = (1, 0) (ahead), beam 2 = (0, -1) (right); the rest
    the env's own"""
    bc, bs = beam_table(B)
    bc, bs = bc.copy(), bs.copy()
    bc[:3] = [0.0, 1.0, 0.0]
    bs[:3] = [1.0, 0.0, -1.0]
    return bc, bs


class _Rows:
    def __init__(self, B):
        self.B, self.names, self.goals, self.cmds, self.rows = B, [], [], [], []

    def open_row(self):
        return np.full(self.B, 6.0, f32)

    def lone(self, beam, r):
        row = self.open_row()
        row[beam] = f32(r)
        return row

    def add(self, name, goal, row, cmd=COMMAND):
        assert name not in self.names
        self.names.append(name)
        self.goals.append(goal)
        self.cmds.append(cmd)
        self.rows.append(row)

    def arrays(self):
        return self.names, np.array(self.goals, f32), np.array(self.cmds, f32), np.stack(self.rows)


def crafted(B=64):
    """The host set, on ``crafted_table(B)`` -> (names, goal, policy, rows)"""
    c = _Rows(B)
    cor, risk, stop = (f32(PARAMS[k]) for k in ("corridor", "risk_dist", "stop_dist"))
    c.add("goal_half_a_metre_ahead", (0.5, 0.0), c.lone(1, 0.2))
    c.add("goal_just_outside", (float(above(0.5)), 0.0), c.open_row())
    c.add("all_ranges_6", (3.0, 1.0), c.open_row())
    c.add("edge_of_corridor_t0", (4.0, 0.0), c.lone(0, cor))                 # t = 0, |l| = corridor exactly: does not block
    c.add("inside_corridor_t0", (4.0, 0.0), c.lone(0, below(cor)))           # t = 0, one ulp inside: blocks
    c.add("inside_corridor_right_t0", (4.0, 0.0), c.lone(2, below(cor)))
    c.add("at_reach", (2.0, 0.0), c.lone(1, 2.0))                            # t = reach = gl exactly: blocks
    c.add("beyond_reach", (2.0, 0.0), c.lone(1, above(2.0)))
    c.add("at_look", (5.5, 0.0), c.lone(1, 4.0))                             # t = reach = look exactly: blocks
    c.add("beyond_look", (5.5, 0.0), c.lone(1, above(4.0)))
    c.add("d_min_is_risk", (0.0, 3.0), c.lone(2, risk))                      # exactly risk_dist: not emergent
    c.add("d_min_below_risk", (0.0, 3.0), c.lone(2, below(risk)))
    c.add("d_front_at_stop", (3.0, 0.0), c.lone(1, stop))                    # s = 0
    c.add("d_front_below_stop", (3.0, 0.0), c.lone(1, 0.1))                  # s would be negative: 0
    c.add("d_front_between", (3.0, 0.0), c.lone(1, 0.325))                   # s = 0.25 (about)
    c.add("risk_beside_front_open", (3.0, 0.0), c.lone(0, 0.35))             # d_front 6: s = safe_scale
    row = c.open_row()
    row[1], row[5] = f32(-0.0), f32(0.0)
    c.add("range_minus_0", (3.0, 0.0), row)
    _goals_and_commands(c, blocked=c.lone(1, 1.0), risky=c.lone(1, 0.35))
    return c.arrays()


def _goals_and_commands(c, blocked, risky):
    """the rows that need no exact beam: goals behind and beside, and the special commands in every mode"""
    c.add("goal_straight_behind", (-3.0, 0.0), c.open_row())
    c.add("goal_behind_left", (-3.0, 1.0), c.open_row())
    c.add("goal_behind_right", (-3.0, -1.0), c.open_row())
    c.add("goal_ahead_left", (1.0, 0.05), c.open_row())
    for k, cmd in SPECIAL_COMMANDS:
        c.add("normal_" + k, (3.0, 0.0), blocked, cmd)
        c.add("simple_" + k, (3.0, 0.0), c.open_row(), cmd)
        c.add("emergent_" + k, (3.0, 0.0), risky, cmd)
        c.add("at_goal_" + k, (0.1, 0.1), c.open_row(), cmd)


def edge_range(threshold, component):
    """The floats around threshold / |component| whose float32 product with |component| IS the threshold -> (the smallest, the
    largest) of them, or None where the product steps over the threshold."""
    comp, thr = np.abs(f32(component)), f32(threshold)
    r = f32(thr / comp)
    for _ in range(8):
        r = below(r)
    hits = []
    for _ in range(17):
        if f32(r * comp) == thr:
            hits.append(r)
        r = above(r)
    return (hits[0], hits[-1]) if hits else None


def edge_beams(B):
    """the first and the last lane of the kernel's first and of its last round"""
    return sorted({0, 63, min(64, B - 1), B - 1})


def device_cases(B):
    """``crafted`` rebuilt on the env's own beam table -> (names, goal, policy, rows); a name ends in _b<beam> where the row is a
    lone return on that beam"""
    c = _Rows(B)
    bc, bs = beam_table(B)
    cor, risk, stop, look = (f32(PARAMS[k]) for k in ("corridor", "risk_dist", "stop_dist", "look"))
    mid = B // 2                                                             # the beam nearest to straight ahead (a little to the left)
    assert bs[0] == -1.0 and bs[B - 1] == 1.0 and (bc >= 0).all() and bc[mid] > 0.999
    c.add("goal_half_a_metre_ahead", (0.5, 0.0), c.lone(mid, 0.2))
    c.add("goal_just_outside", (float(above(0.5)), 0.0), c.open_row())
    c.add("all_ranges_6", (3.0, 1.0), c.open_row())
    # the corridor's edge, goal ahead on the x axis (u = (1, 0) exactly): t = r cos >= 0, |l| = |r sin|
    for b in edge_beams(B):
        hit = edge_range(cor, bs[b])
        if hit is None:                                                      # (the product steps over 0.45 on this beam: none at
            continue                                                         # 64, 192 and 1024 beams -- asserted below)
        c.add(f"edge_of_corridor_b{b}", (4.0, 0.0), c.lone(b, hit[0]))      # |l| = corridor exactly: does not block
        c.add(f"inside_corridor_b{b}", (4.0, 0.0), c.lone(b, below(hit[0])))               # one ulp inside: blocks
    assert sum(k.startswith("edge_of_corridor") for k in c.names) == len(edge_beams(B))
    # reach and look: t = r cos on a beam inside the corridor ahead, the nearest to the middle on either side that has such a range
    for what, goal, thr in (("reach", (2.0, 0.0), f32(2.0)), ("look", (5.5, 0.0), look)):
        found = 0
        for b in sorted(range(B), key=lambda b: abs(b - mid + 0.5)):
            hit = edge_range(thr, bc[b])
            if hit is None or not above(hit[1]) * np.abs(bs[b]) < cor:
                continue
            c.add(f"at_{what}_b{b}", goal, c.lone(b, hit[1]))               # t = reach exactly: blocks
            c.add(f"beyond_{what}_b{b}", goal, c.lone(b, above(hit[1])))
            found += 1
            if found == 2:
                break
        assert found == 2, what
    # the risk: the range itself, on every edge beam, with the goal on the other side (the return is behind the way to it)
    for b in edge_beams(B):
        goal = (0.0, 3.0) if bs[b] < 0 else (0.0, -3.0)
        c.add(f"d_min_is_risk_b{b}", goal, c.lone(b, risk))                 # exactly risk_dist: not emergent
        c.add(f"d_min_below_risk_b{b}", goal, c.lone(b, below(risk)))
    c.add("d_front_at_stop", (3.0, 0.0), c.lone(mid, stop))
    c.add("d_front_below_stop", (3.0, 0.0), c.lone(mid, 0.1))
    c.add("d_front_between", (3.0, 0.0), c.lone(mid, 0.325))
    c.add("risk_beside_front_open", (3.0, 0.0), c.lone(0, 0.35))            # beam 0 is not ahead (front_cos 0.5): d_front 6
    row = c.open_row()
    row[mid], row[5] = f32(-0.0), f32(0.0)
    c.add("range_minus_0", (3.0, 0.0), row)
    c.add("all_beams_block", (4.0, 0.0), np.full(B, 0.44, f32))             # every |r sin| < 0.45, every t in [0, 4]: the count is B
    _goals_and_commands(c, blocked=c.lone(mid, 1.0), risky=c.lone(mid, 0.35))
    return c.arrays()


def expectations(names, p, policy, rows, act, mode, clear, nb):
    """What the rows of ``crafted`` / ``device_cases`` are made for, asserted on the restatement's outputs under
    R.params(**PARAMS); the rows stand at the front of the arrays in the order of ``names``."""
    ix = {k: i for i, k in enumerate(names)}
    cor = p["corridor"]

    def m(k):
        return int(mode[ix[k]])

    def named(prefix):
        got = [k for k in names if k == prefix or k.startswith(prefix + "_b") or k.startswith(prefix + "_t0") or
               k.startswith(prefix + "_right_t0")]
        assert got, prefix
        return got
    # 0.5 m is AT the goal (<=): (0, 0) whatever is near; the next float is not
    assert m("goal_half_a_metre_ahead") == R.AT_GOAL and same_bits(act[ix["goal_half_a_metre_ahead"]], [0.0, 0.0])
    assert same_bits(clear[ix["goal_half_a_metre_ahead"]], [0.2, 0.2, 6.0])
    assert m("goal_just_outside") == R.SIMPLE
    # nothing anywhere: the PID law, and every clearance is 6
    i = ix["all_ranges_6"]
    assert m("all_ranges_6") == R.SIMPLE and same_bits(clear[i], [6.0, 6.0, 6.0]) and act[i][0] > 0.9 and act[i][1] == 1.0
    # the corridor's edge is outside it (strict), one ulp inside blocks; t = 0 is inside (>=)
    for k in named("edge_of_corridor"):
        assert nb[ix[k]] == 0 and m(k) == R.SIMPLE, k
    for k in named("inside_corridor"):
        assert nb[ix[k]] == 1 and m(k) == R.NORMAL and same_bits(act[ix[k]], policy[ix[k]]) and clear[ix[k]][2] == rows[ix[k]].min(), k
    if "inside_corridor_t0" in ix:
        assert all(clear[ix[k]][2] == below(cor) for k in ("inside_corridor_t0", "inside_corridor_right_t0"))
    # t = reach is inside (<=), whether the goal's distance or `look` ends the corridor
    for what in ("reach", "look"):
        for k in named("at_" + what):
            assert nb[ix[k]] == 1 and m(k) == R.NORMAL, k
        for k in named("beyond_" + what):
            assert nb[ix[k]] == 0 and m(k) == R.SIMPLE, k
    # d_min == risk_dist is not a risk (strict)
    assert all(m(k) == R.SIMPLE for k in named("d_min_is_risk")) and all(m(k) == R.EMERGENT for k in named("d_min_below_risk"))
    # the scale: 0 at and below stop_dist, in between in between, safe_scale where nothing is ahead; omega goes through
    for k in ("d_front_at_stop", "d_front_below_stop"):
        assert m(k) == R.EMERGENT and same_bits(act[ix[k]], [0.0, -0.25])
    i = ix["d_front_between"]
    assert m("d_front_between") == R.EMERGENT and 0.0 < act[i][0] < 0.75 * 0.5 and same_bits(act[i][1], -0.25)
    i = ix["risk_beside_front_open"]
    assert m("risk_beside_front_open") == R.EMERGENT and same_bits(act[i], [0.75 * 0.5, -0.25]) and same_bits(clear[i], [0.35, 6.0, 0.35])
    # -0.0 is a 0: d_min is +0, the robot is in danger and stops
    i = ix["range_minus_0"]
    assert m("range_minus_0") == R.EMERGENT and same_bits(clear[i], [0.0, 0.0, 0.0]) and same_bits(act[i], [0.0, -0.25])
    # a goal behind (fwd <= 0): stand and turn at full rate, to the left when the goal is straight behind or to the left
    assert same_bits(act[ix["goal_straight_behind"]], [0.0, 1.0]) and same_bits(act[ix["goal_behind_left"]], [0.0, 1.0])
    assert same_bits(act[ix["goal_behind_right"]], [0.0, -1.0])
    assert all(m(k) == R.SIMPLE for k in ("goal_straight_behind", "goal_behind_left", "goal_behind_right", "goal_ahead_left"))
    i = ix["goal_ahead_left"]
    assert 0.99 < act[i][0] < 1.0 and 0.29 < act[i][1] < 0.31           # k_omega * uy = 6 * 0.05 (about)
    # a NaN, an Inf or a -0.0 coming in: normal copies the bits, simple and at-goal do not look at them, emergent scales v
    for k, _cmd in SPECIAL_COMMANDS:
        i = ix["normal_" + k]
        assert m("normal_" + k) == R.NORMAL and np.array_equal(bits(act[i]), bits(policy[i]))
        assert m("simple_" + k) == R.SIMPLE and same_bits(act[ix["simple_" + k]], [1.0, 0.0])
        assert m("at_goal_" + k) == R.AT_GOAL and same_bits(act[ix["at_goal_" + k]], [0.0, 0.0])
        i = ix["emergent_" + k]
        assert m("emergent_" + k) == R.EMERGENT and np.array_equal(bits(act[i][1]), bits(policy[i][1]))
    assert np.isnan(act[ix["emergent_nan"]][0]) and np.isinf(act[ix["emergent_inf"]][0])
    assert same_bits(act[ix["emergent_minus_0"]], [-0.0, -0.0])
    # all B beams block (the device set)
    if "all_beams_block" in ix:
        i = ix["all_beams_block"]
        assert nb[i] == rows.shape[1] and m("all_beams_block") == R.NORMAL and same_bits(clear[i], [0.44, 0.44, 0.44])
