"""The degenerate scenes (tests/degenerate_scenes.py) through the CPU references -- no GPU needed.

Every scene runs through the C oracle (the reference of tests/test_gpu_degenerate_geometry.py), the NumPy oracle (the
specification) and, where it applies (exact rectangles, worlds of at most 64 robots), the host build of the product's
per-lane arithmetic (U.EmulEnv): every field after the reset and after every tick, bit for bit, the hit flags included.
Every value stays finite.  Each scene's coverage flags are asserted from the C oracle's run and from the NumPy oracle's: the
scene meets the edges it is there for.

This is the pre-flight of the GPU file: a scene that does not end, or on which the references disagree, shows here."""
import numpy as np
import pytest

import degenerate_scenes as D
import util as U
from test_gpu_raycast_variants import FAMILIES, selection

FLOAT_FIELDS = [k for k in U.STATE_FIELDS if k not in ("done", "result", "first_result", "crashed", "live", "t", "episode")]


def test_the_scenes_cover_every_family():
    got = {name: selection(D.scenario(name)) for name in D.SCENES}
    for name, sc in D.SCENES.items():
        assert got[name] == sc.selects, f"{name} is here for {sc.selects} and now selects {got[name]}"
    missing = FAMILIES - set(got.values())
    assert not missing, f"no scene selects {sorted(missing)}"
    # the sizes stay the smallest that select the family
    for sc in D.SCENES.values():
        assert 64 <= sc.beams <= 512 and 1 <= sc.frames <= 3 and len(sc.worlds) * sc.R <= 200


def test_the_scenes_are_what_they_say():
    cc, lc = D.hash_cells()
    assert (cc, lc) == (np.float32(0.7), np.float32(6.5))
    for cs, k in ((cc, 2), (cc, 3), (lc, 1)):
        x = D.bucket_border(cs, k)
        assert D.hash_coord(x, cs) == k and D.hash_coord(np.nextafter(x, np.float32(0)), cs) == k - 1
        assert D.hash_coord(-x, cs) == -k and D.hash_coord(np.nextafter(-x, np.float32(-99)), cs) == -k - 1
    for name, sc in D.SCENES.items():
        assert not D.spacing_ok(name), (name, D.spacing_ok(name))
        poses, goals = D.poses_goals(name)
        assert np.isfinite(poses).all() and np.isfinite(goals).all()
        for k in range(sc.ticks):
            a = D.commands(name, k)
            fin = np.isfinite(a)
            assert ((a[:, 0][fin[:, 0]] >= 0) & (a[:, 0][fin[:, 0]] <= 1)).all(), "v outside the documented range"
            assert (np.abs(a[:, 1][fin[:, 1]]) <= 1).all(), "w outside the documented range"
    # pi/2 and pi are NOT exactly axis parallel under the shared sincos; 0 and -0.0 are
    s, c = D.O.sincos(np.array([0.0, -0.0, D.HALF_PI, -D.HALF_PI, D.PI], np.float32), np.float32)
    assert (s[:2] == 0).all() and (c[:2] == 1).all() and (c[2:4] != 0).all() and s[4] != 0
    for beams in sorted({sc.beams for sc in D.SCENES.values()}):
        th, i = D.diagonal_heading(beams)
        bc, bs = D.O.beam_table(np.float32, beams)
        s, c = D.O.sincos(np.array([th], np.float32), np.float32)
        assert (c * bc[i] - s * bs[i])[0] == (s * bc[i] + c * bs[i])[0] > 0


def _finite(env, what):
    for k in FLOAT_FIELDS:
        assert np.isfinite(np.asarray(getattr(env, k))).all(), f"{what}: {k} is not finite"


@pytest.mark.parametrize("name", list(D.SCENES))
def test_cpu_references_agree_on_every_field(name):
    scn, sc = D.SCENES[name], D.scenario(name)
    run = D.oracle_run(name)
    assert not D.missing_flags(name, run.flags), f"{name}: the oracle's run does not exercise {D.missing_flags(name, run.flags)}"
    for k, snap in run.snaps.items():
        _finite(snap, f"{name} C oracle tick {k}")
    envs = {"NumPy oracle": U.oracle_env(sc)}
    if scn.raster == 0 and scn.R <= 64:
        envs["host emulation"] = U.EmulEnv(sc)
    watch = D.Watcher(name, envs["NumPy oracle"])
    for what, e in envs.items():
        e.reset(None, run.poses, run.goals)
        U.assert_state_equal(e, run.snaps[-1], what=f"{name} {what} reset")
    assert np.array_equal(np.asarray(envs["NumPy oracle"].hit_robot).astype(bool), run.snaps[-1].hit_robot.astype(bool))
    watch.after_reset()
    for k in range(scn.ticks):
        watch.before(run.actions[k])
        for what, e in envs.items():
            e.step(run.actions[k])
            U.assert_state_equal(e, run.snaps[k], what=f"{name} {what} tick {k}")
        watch.after()
        assert np.array_equal(np.asarray(envs["NumPy oracle"].hit_robot).astype(bool), run.snaps[k].hit_robot.astype(bool)), \
            f"{name} tick {k}: hit flags"
    assert watch.flags == run.flags, (sorted(watch.flags ^ run.flags))


def test_non_finite_tick_on_the_cpu():
    """the tick of tests/test_gpu_degenerate_geometry.py in which (almost) every command is non-finite: NumPy oracle, C oracle
    and host emulation agree, a live robot whose two components are non-finite keeps its pose, everything stays finite"""
    for name in ("coarse_exact_k1", "big_k1", "stage2_hold"):
        sc = D.scenario(name)
        run = D.oracle_run(name)
        envs = [U.oracle_env(sc), U.COracleEnv(sc)] + ([U.EmulEnv(sc)] if sc.robots_per_world <= 64 else [])
        for e in envs:
            e.reset(None, run.poses, run.goals)
        bad = D.non_finite_commands(sc.num_robots)
        for k, a in enumerate([run.actions[0], run.actions[1], bad, run.actions[2], bad, run.actions[3]]):
            before, live = np.array(envs[0].pose), np.asarray(envs[0].live).astype(bool).copy()
            for e in envs:
                e.step(a)
            for e in envs[1:]:
                U.assert_state_equal(e, envs[0], what=f"{name} call {k}")
            _finite(envs[0], f"{name} call {k}")
            if a is bad:
                idle = live & ~np.isfinite(a).any(1) & (np.asarray(envs[0].done) == 0)
                assert idle.sum() >= 4
                assert (np.asarray(envs[0].pose)[idle].view(np.uint32) == before[idle].view(np.uint32)).all()
                assert (np.asarray(envs[0].speed)[idle].view(np.uint32) == 0).all()
