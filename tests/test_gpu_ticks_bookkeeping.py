"""The bookkeeping of the ray cast of several ticks (csrc/mrca_raycast_ticks.hip, raycast_body<..., TICKS>): the closed-form
ring rule, the fresh flags through one base and a 32-bit offset, the loads through the kernel's pointer arguments (run with
-m gpu on an MI355X).

Two envs of one seeded scenario in one process, one created under MRCA_TICKS_PER_LAUNCH=3 and one under =1 (a launch per tick:
the single-tick kernel), take the same actions through ``step_many`` in calls of 1, 2, 3, 4, 6, 7 and 13 ticks.  After every
call pose, goal, fresh flags, scan ring, ring heads, hit bits and local goal -- and every other field a caller reads -- must be
equal bit for bit, and after the last call both must agree with the C oracle (tests/util.COracleEnv).

At three ticks per launch those calls cut into launches of one, two and three ticks, and the call's last launch -- the one whose
last tick reads the env's own fields instead of a ring slot -- comes at each of the three lengths (6: two ticks, 7 and 13:
three); ``test_the_calls_end_in_launches_of_every_length`` holds that against the plan's restatement.  The shapes: robot counts
per range that are and are not multiples of 8 (both arms of block_to_robot), one robot per world, 64 beams (one wave, one beam
per thread) as well as 512, with one world range and with two (a range that does not begin at robot 0).

Restarts are placed by the episode time-out: every robot's episode ends after ``timeout`` + 1 ticks, which walks the restart
through a launch's first, middle and last tick as the calls go by.  The last shape restarts one robot twice inside one launch:
with a time-out of one tick every robot restarts every other tick (fresh, stale, fresh), and two robots of every world have
their goal on their start pose and restart in every tick.  Each shape names the patterns of restarts (launch length, flags of
one robot over the launch's ticks) it must produce, and the test counts them in the fresh flags of the =1 env stepped tick by
tick -- a sequence that lost its restarts would fail, not pass."""
import numpy as np
import pytest
import torch

import util as U
from pass_plan_ref import launch_plan
from util import S

pytestmark = pytest.mark.gpu

CALLS = (1, 2, 3, 4, 6, 7, 13)
T = 3                                    # MRCA_TICKS_PER_LAUNCH of the env under test (the ring has three frames)
FIELDS = ("pose", "goal", "fresh", "scan_ring", "ring_head", "hit_bits", "local_goal")


def _stage1(worlds, robots, seed, timeout, beams=512):
    sc = S.stage1(num_worlds=worlds, robots_per_world=robots, seed=seed)
    sc.timeout = timeout
    sc.beams = beams
    return sc


def _twice(worlds, robots, seed):
    """every robot restarts every other tick; robots 0 and 1 of every world, their goal on their start pose, in every tick"""
    sc = _stage1(worlds, robots, seed, timeout=1)
    sc.reset_mode[:2] = S.RESET_TABLE
    sc.goal_mode[:2] = S.RESET_TABLE
    sc.init_table[0] = (2.0, 0.0, 0.0)
    sc.init_table[1] = (-2.0, 1.0, 1.0)
    sc.goal_table[0] = (2.0, 0.0)
    sc.goal_table[1] = (-2.0, 1.0)
    return sc


# name -> (scenario, the restart patterns it must produce: (ticks of the launch, one robot's flags over them))
SHAPES = {
    # 15 robots, ranges of 10 and 5: no multiple of 8; a restart in a launch's first, middle and last tick
    "3x5": (lambda: _stage1(3, 5, 42, timeout=3), {(3, "100"), (3, "010"), (3, "001"), (2, "01")}),
    # 16 robots, ranges of 8: the XCD arm of block_to_robot
    "4x4": (lambda: _stage1(4, 4, 48, timeout=2), {(3, "100"), (3, "001"), (2, "10"), (2, "01")}),
    # one robot per world: no neighbour candidate, n / R without the magic multiply
    "4x1": (lambda: _stage1(4, 1, 49, timeout=4), {(3, "010"), (3, "001"), (2, "10"), (2, "01")}),
    # 64 beams: raycast_ticks_kernel<1, false, 0> with one marching wave
    "3x5_64beams": (lambda: _stage1(3, 5, 50, timeout=3, beams=64), {(3, "100"), (3, "010"), (3, "001"), (2, "01")}),
    # two ticks of one launch restart the same robot
    "4x4_twice": (lambda: _twice(4, 4, 47), {(3, "101"), (3, "111"), (3, "010"), (2, "11"), (2, "10"), (2, "01")}),
}


def host_actions(sc):
    rng = np.random.default_rng(1000 + sc.seed)
    return [U.random_actions(rng, sc.num_robots) for _ in range(16)]


def restart_patterns(fresh):
    """{(n, flags)}: launches of n > 1 ticks of the CALLS sequence at T ticks per launch in which some robot restarts, with that
    robot's flags over the launch's ticks; fresh: [ticks, N] the fresh flags after every tick"""
    seen, t0 = set(), 0
    for K in CALLS:
        for k, n in launch_plan(K, T):
            if n > 1:
                for flags in fresh[t0 + k: t0 + k + n].T:
                    if flags.any():
                        seen.add((n, "".join(str(int(f)) for f in flags)))
        t0 += K
    return seen


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def make_env(hip, monkeypatch, sc, ticks_per_launch):
    monkeypatch.setenv("MRCA_TICKS_PER_LAUNCH", str(ticks_per_launch))       # (read once, in mrca_create)
    env = hip.VecStageWorld(sc)
    pool = [torch.from_numpy(a).to(env.device) for a in host_actions(sc)]
    env.reset()
    return env, pool


def snapshot(env, fields):
    torch.cuda.synchronize()
    return {f: getattr(env, f).cpu().numpy().copy() for f in fields}


_reference = {}


def reference_run(hip, monkeypatch, name):
    """once per shape: the =1 env tick by tick -> the fresh flags of every tick; the C oracle -> its state after the last tick"""
    if name not in _reference:
        sc = SHAPES[name][0]()
        env, pool = make_env(hip, monkeypatch, sc, 1)
        fresh = []
        for k in range(sum(CALLS)):
            env.step_many(pool, k, 1, 1)
            torch.cuda.synchronize()
            fresh.append(env.fresh.cpu().numpy().copy())
        env.check()
        env.close()
        ora = U.COracleEnv(sc)
        ora.reset()
        for k, a in zip(range(sum(CALLS)), host_actions(sc) * sum(CALLS)):
            ora.step(a)
        _reference[name] = (np.stack(fresh), ora)
    return _reference[name]


def test_the_calls_end_in_launches_of_every_length():
    assert {launch_plan(K, T)[-1][1] for K in CALLS} == {1, 2, 3}
    assert {n for K in CALLS for _k, n in launch_plan(K, T)} == {1, 2, 3}


@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_three_ticks_per_launch_equal_one(hip, monkeypatch, name, chains):
    import bench
    make, claims = SHAPES[name]
    fresh, ora = reference_run(hip, monkeypatch, name)
    # no vacuous pass: the sequence restarts robots in every pattern the shape names
    seen = restart_patterns(fresh)
    assert claims <= seen, f"{name}: no launch with the restart pattern(s) {sorted(claims - seen)}; seen {sorted(seen)}"
    sc = make()
    fields = tuple(dict.fromkeys(FIELDS + bench.DUMP_FIELDS))
    env3, pool3 = make_env(hip, monkeypatch, sc, T)
    env1, pool1 = make_env(hip, monkeypatch, sc, 1)
    k = 0
    for K in CALLS:
        for env, pool in ((env3, pool3), (env1, pool1)):
            env.step_many(pool, k, K, chains)
            env.invalidate_views()
        k += K
        got, want = snapshot(env3, fields), snapshot(env1, fields)
        for f in fields:
            a, b = got[f], want[f]
            same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
            assert same.all(), (f"{name}, {chains} range(s): {f} differs at {int((~same).sum())} of {same.size} entries after "
                                f"the call of {K} ticks ({k} in all)")
        # (the tick-by-tick run the patterns were counted in is this run)
        assert np.array_equal(want["fresh"], fresh[k - 1]), f"{name}: the fresh flags after tick {k}"
    for env in (env3, env1):
        env.check()
        U.assert_state_equal(U.HostView(env), ora, what=f"{name}, {chains} range(s), against the C oracle")
        U.assert_hits_equal(env, ora, what=f"{name}, {chains} range(s), against the C oracle")
        assert np.array_equal(env.fresh.cpu().numpy(), ora.fresh), f"{name}: fresh flags against the C oracle"
        env.close()
