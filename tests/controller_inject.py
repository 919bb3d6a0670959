"""Puts crafted controller cases (tests/dwa_cases.py, hybrid_cases.py, orca_cases.py, safe_cases.py) into an env on the device,
one case per robot, for the GPU tests of the five controllers.

The env is a small walled world built from ``test_gpu_orca.small_scenario`` (worlds of 7 robots, as many as the cases need) or,
where poses matter, an open ``circle_n`` / ``circle_big`` world.  Its ring heads are made to differ between robots first, as in
the tests named "ring heads that differ"; the robots behind the cases keep the random states of that run.  Poses and goals go in
through ``reset(None, poses, goals)`` only (the head records of the ORCA kernels are written there).  Everything else is written
through the env's zero-copy field views: ``local_goal``, ``speed``, ``speed_gt``, the newest ``scan_ring`` row at each robot's
OWN ``ring_head``, and the ``hit_bits`` word of that row.  The env is not stepped after the write: the GPU tests' ``check_equal``
reads host copies of the fields back and feeds the restatement with them, so what is compared -- and what the edge of a case
is asserted from -- is what the kernel really read."""
import numpy as np
import torch

import util as U
from test_gpu_orca import small_scenario
from util import S

f32 = np.float32
MAX_ROBOTS = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def small_walled_scenario(beams, frames, n_cases):
    """``small_scenario`` with as many 7-robot worlds as ``n_cases`` robots need (at least its own 3, at most 9 = 63 robots)"""
    sc = small_scenario(beams, frames)
    worlds = max(sc.num_worlds, -(-n_cases // sc.robots_per_world))
    assert worlds * sc.robots_per_world <= MAX_ROBOTS, n_cases
    if worlds != sc.num_worlds:
        sc = S.stage1(num_worlds=worlds, robots_per_world=sc.robots_per_world, seed=sc.seed, grid=sc.grid)
        sc.beams, sc.frames = beams, frames
    return sc


def differing_heads(env, seed=6):
    """Random ticks, a masked reset and one more tick of world 0 alone: ring heads that differ between robots (frames >= 2).
    Worlds of more than 64 robots do not tick alone: there the last tick casts the rays of a third of the robots only."""
    rng = np.random.default_rng(seed)
    env.reset()
    for _ in range(4):
        env.step(dev(U.random_actions(rng, env.N)))
    env.reset(dev((np.arange(env.N) % 4 == 1).astype(np.uint8)))         # a masked reset: these robots start a new history
    if env.R > MAX_ROBOTS:
        env.step(dev(U.random_actions(rng, env.N)), ray_slice=(env.N // 3, env.N // 3))
    else:
        env.step(dev(U.random_actions(rng, env.N)), worlds=(0, 1))        # ... and world 0 ticks alone, once more
    torch.cuda.synchronize()
    return env


def heads_differ(env):
    torch.cuda.synchronize()
    return len(set(env.ring_head.cpu().numpy().tolist())) > 1


def walled_env(vec_env, beams, n_cases, frames=3):
    """-> a small walled env of at least ``n_cases`` robots whose ring heads differ"""
    env = differing_heads(vec_env.VecStageWorld(small_walled_scenario(beams, frames, n_cases)))
    assert env.N >= n_cases and heads_differ(env)
    return env


def pack_hits(hit):
    """bool[n,B] -> i64[n,B/64]: bit (b & 63) of word b >> 6, as MRCA_F_HIT_BITS holds it"""
    return np.ascontiguousarray(np.packbits(np.asarray(hit, bool), axis=-1, bitorder="little")).view(np.int64)


def write_cases(env, first=0, local_goal=None, speed=None, speed_gt=None, rows=None, hit=None):
    """Case k of each array given goes to robot ``first + k``; rows / hit: the newest scan row of that robot and its hit flags."""
    def put(view, a, shape):
        a = np.ascontiguousarray(a, f32).reshape(shape)
        assert first + len(a) <= env.N
        view[first:first + len(a)] = dev(a)
        return len(a)
    if local_goal is not None:
        put(env.local_goal, local_goal, (-1, 2))
    if speed is not None:
        put(env.speed, speed, (-1, 2))
    if speed_gt is not None:
        put(env.speed_gt, speed_gt, (-1, 2))
    for a, view in ((rows, env.scan_ring), (hit, env.hit_bits)):
        if a is None:
            continue
        a = np.ascontiguousarray(a, f32) if view is env.scan_ring else pack_hits(a)
        assert first + len(a) <= env.N and a.shape[1] == view.shape[2]
        who = torch.arange(first, first + len(a), device=env.device)
        view[who, env.ring_head.long()[who]] = dev(a)
    env.invalidate_views()               # (``scan`` / ``obs``, if somebody reads them, are formed again from the ring)
    torch.cuda.synchronize()
    return env


# ------------------------------------------------------------------------------------------------ where poses matter
def open_env(vec_env, robots, beams, frames=3):
    """-> an open env whose ring heads differ: two ``circle_n`` worlds of ``robots`` robots each or, for more than 64 robots, one
    ``circle_big`` world"""
    if robots > MAX_ROBOTS:
        sc = S.circle_big(robots)
    else:
        sc = S.circle_n(robots, 20.0, num_worlds=2, grid=S.empty_grid())
    sc.beams, sc.frames = beams, frames
    env = differing_heads(vec_env.VecStageWorld(sc))
    assert heads_differ(env)
    return env


def write_world(env, world):
    """``world``: ``orca_cases.device_world`` -- into EVERY world of the env: poses and goals through a reset of all robots (the
    ring heads stay where they are: a restarted robot's scan fills every slot), then speed_gt, scan rows and hit flags of the
    case robots through the field views."""
    W, R = env.W, env.R
    assert len(world["poses"]) == R
    env.reset(None, dev(np.tile(world["poses"], (W, 1))), dev(np.tile(world["goals"], (W, 1))))
    torch.cuda.synchronize()
    for w in range(W):
        for what, cases in (("speed_gt", world["speed_gt"]), ("rows", world["rows"]), ("hit", world["hit"])):
            for n, v in cases.items():
                write_cases(env, w * R + n, **{what: np.asarray(v)[None]})
    assert heads_differ(env)
    return env
