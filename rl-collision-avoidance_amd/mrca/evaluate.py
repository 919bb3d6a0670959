"""Circle-test evaluator: the reference's ``circle_test.py`` demo loop (``enjoy``, :36-83) for any
number of independent 50-robot circles, with the success metric the reference never computes.

Success rate (decision 12): fraction of robots whose FIRST terminal event since reset is
"Reach Goal" -- latched on the device in ``first_result`` (the reference does not latch,
circle_test.py:64-70).  Also reported: crash rate, unfinished rate, mean ticks-to-goal of the
successful robots and their mean path length ratio vs the 50 m straight line.
"""
import argparse
import json
import math
import sys

import torch

from . import ppo, scenario
from .net import CNNPolicy

ACTION_BOUND = ((0.0, -1.0), (1.0, 1.0))     # circle_test.py:92
# --scenario NAME -> the constructor in mrca.scenario whose boxes the scenario sampler fills (Long et al. 2018, Sec. V)
SCATTER_SCENARIOS = {"random": "random_box", "swap": "group_swap", "crossing": "group_crossing", "corridor": "corridor"}


def go_to_goal_policy(obs, local_goal, speed):
    """Stand-in controller (no learning): drive at the goal, turn towards it, slow down when the
    lidar sees something close ahead.  Used where ``policy/stage2.pth`` is unavailable."""
    lx, ly = local_goal[:, 0], local_goal[:, 1]
    bearing = torch.atan2(ly, lx)
    ahead = (obs[:, -1, 192:320].min(dim=1).values + 0.5) * 6.0      # nearest return in the front 45 degrees
    v = torch.clamp(0.4 * ahead, 0.0, 1.0) * (bearing.abs() < 1.0).float()
    w = torch.clamp(2.0 * bearing, -1.0, 1.0)
    return torch.stack([v, w], dim=1)


def staggered_roundabout_policy(num_robots, bias=1.4, near=3.5, vgain=0.8, stop=0.5, slowest=0.5):
    """A stand-in with NON-TRIVIAL outcomes on the circle test (78 % success / 22 % crashes for one circle):
    head for the goal, veer right in proportion to how close the nearest return in the front sector is (a
    roundabout), slow down before obstacles, and -- to break the perfect symmetry of the scenario, which no
    memoryless symmetric rule survives -- give every robot its own speed limit in [slowest, 1] m/s."""
    idx = torch.arange(num_robots) % 50
    scale = slowest + (1.0 - slowest) * ((idx * 7) % 50).float() / 49.0

    def fn(obs, local_goal, speed):
        lx, ly = local_goal[:, 0], local_goal[:, 1]
        bearing = torch.atan2(ly, lx)
        dist = torch.sqrt(lx * lx + ly * ly)
        front = ((obs[:, -1, 176:336] + 0.5) * 6.0).min(dim=1).values
        prox = ((near - front) / near).clamp(0.0, 1.0)
        target = bearing - bias * prox * (dist > 1.0).float()
        w = torch.clamp(2.5 * target, -1.0, 1.0)
        v = torch.clamp(vgain * (front - stop), 0.0, 1.0) * (target.abs() < 1.0).float() * scale.to(obs.device)
        return torch.stack([v, w], dim=1)
    return fn


def cnn_policy_fn(policy, fused=False, env=None, fused_bf16=False):
    """``fused`` with ``env``: the policy's HIP front end reads the env's frame ring in place (no materialised stacks).
    ``fused_bf16``: the fused path's opt-in bf16 inference (needs ``fused``)."""
    def fn(obs, local_goal, speed):
        head = None
        if fused and env is not None:
            obs, head = ppo.policy_input(env, True)
        _mean, scaled = ppo.generate_action_no_sampling(policy, obs, local_goal, speed, ACTION_BOUND, fused=fused,
                                                        obs_head=head, fused_bf16=fused_bf16)
        return scaled
    fn.wants_obs = not (fused and env is not None)
    return fn


def orca_policy_fn(env, params=None, first=None, other=None):
    """The ORCA baseline controller on the device (``VecStageWorld.orca_actions``): it reads the env's own fields, so it wants
    no observation stack.  ``first = K`` with ``other``: robots with local index < K are driven by ORCA (through the mask),
    the rest by the policy function ``other`` -- the paper's mixed scenarios."""
    if first is None:
        def fn(obs, local_goal, speed):
            return env.orca_actions(params)
        fn.wants_obs = False
        return fn
    mask = (torch.arange(env.N, device=env.device) % env.R < int(first)).to(torch.uint8).contiguous()

    def mixed(obs, local_goal, speed):
        a = other(obs, local_goal, speed).float().contiguous().clone()
        return env.orca_actions(params, mask=mask, out=a)
    mixed.wants_obs = getattr(other, "wants_obs", True)
    mixed.groups = {"orca": mask.bool(), "policy": ~mask.bool()}
    return mixed


def nhorca_policy_fn(env, params=None, first=None, other=None):
    """The NH-ORCA baseline controller on the device (``VecStageWorld.nhorca_actions``), used like ``orca_policy_fn``: every robot,
    or with ``first = K`` and ``other`` the robots with local index < K (group "nhorca") beside ``other``'s.
    ``fn.mode_shares()`` -> the share of its live robot-ticks (robots without a terminal event yet) spent in each mode; the
    counts are kept on the device and read when that is called."""
    from .nhorca import MODES
    codes = torch.arange(len(MODES), dtype=torch.int32, device=env.device)
    counts = torch.zeros(len(MODES), dtype=torch.int64, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    mask = None if first is None else (torch.arange(env.N, device=env.device) % env.R < int(first)).to(torch.uint8).contiguous()

    def fn(obs, local_goal, speed):
        a = None if mask is None else other(obs, local_goal, speed).float().contiguous().clone()
        a = env.nhorca_actions(params, mask=mask, out=a, mode=mode)
        live = env.first_result == 0 if mask is None else (env.first_result == 0) & mask.bool()
        counts.add_(((mode.unsqueeze(1) == codes) & live.unsqueeze(1)).sum(dim=0))
        return a
    fn.wants_obs = False if mask is None else getattr(other, "wants_obs", True)
    if mask is not None:
        fn.groups = {"nhorca": mask.bool(), "policy": ~mask.bool()}

    def mode_shares():
        c = counts.tolist()
        total = sum(c)
        return {name: (n / total if total else None) for name, n in zip(MODES, c)}
    fn.mode_shares = mode_shares
    return fn


def dwa_policy_fn(env, params=None, first=None, other=None, other_name="policy", steer=False):
    """The DWA baseline controller on the device (``VecStageWorld.dwa_actions``): it reads the env's own fields (each robot's
    scan, local goal and speed), so it wants no observation stack.  ``first = K`` with ``other``: robots with local index < K
    are driven by DWA (through the mask), the rest by the policy function ``other`` (a checkpoint, the stand-in or ORCA), whose
    group is reported as ``other_name`` -- or, where ``other`` is itself a mixed run, as its own groups without DWA's robots.
    ``steer``: DWA steers at the ``local_goal`` it is handed (a planner's subgoals) in place of the env's own."""
    if first is None:
        def fn(obs, local_goal, speed):
            return env.dwa_actions(params, goal=local_goal if steer else None)
        fn.wants_obs = False
        return fn
    mask = (torch.arange(env.N, device=env.device) % env.R < int(first)).to(torch.uint8).contiguous()

    def mixed(obs, local_goal, speed):
        a = other(obs, local_goal, speed).float().contiguous().clone()
        return env.dwa_actions(params, mask=mask, out=a, goal=local_goal if steer else None)
    mixed.wants_obs = getattr(other, "wants_obs", True)
    rest = getattr(other, "groups", None) or {other_name: torch.ones(env.N, dtype=torch.bool, device=env.device)}
    mixed.groups = {"dwa": mask.bool(), **{k: v & ~mask.bool() for k, v in rest.items()}}
    return mixed


def hybrid_policy_fn(env, other, params=None, steer=False):
    """Hybrid control (``VecStageWorld.hybrid_actions``) behind the controller function ``other``, whatever it is: per robot and
    tick a PID law where the way to the goal is free, ``other``'s command with v scaled down where something is dangerously
    close, ``other``'s command elsewhere.  ``fn.mode_shares()`` -> the share of the live robot-ticks (robots without a
    terminal event yet) spent in each mode; the counts are kept on the device and read when that is called.  ``steer``: the
    wrapper's goal is the ``local_goal`` it is handed (a planner's subgoals) in place of the env's own."""
    from .hybrid import MODE_NAMES
    codes = torch.tensor(list(MODE_NAMES), dtype=torch.int32, device=env.device)
    counts = torch.zeros(len(MODE_NAMES), dtype=torch.int64, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)

    def fn(obs, local_goal, speed):
        a = env.hybrid_actions(other(obs, local_goal, speed).float().contiguous(), params, mode=mode,
                               goal=local_goal if steer else None)
        live = env.first_result == 0
        counts.add_(((mode.unsqueeze(1) == codes) & live.unsqueeze(1)).sum(dim=0))
        return a
    fn.wants_obs = getattr(other, "wants_obs", True)
    if getattr(other, "groups", None):
        fn.groups = other.groups

    def mode_shares():
        c = counts.tolist()
        total = sum(c)
        return {name: (n / total if total else None) for name, n in zip(MODE_NAMES.values(), c)}
    fn.mode_shares = mode_shares
    return fn


def safe_policy_fn(policy, env, params=None, safe=None, fused_bf16=False, skip_first=0, steer=False):
    """Hybrid control in the paper's form around the checkpoint ``policy`` (fused inference on the env's ring of raw scans):
    per tick ``env.hybrid_plan`` -> ONE forward in which the robots of mode 2 see their scan through the plan's scale ->
    ``env.hybrid_commit``.  ``skip_first = K``: robots with local index < K belong to another controller (--orca-first,
    --dwa-first): they are masked out of the plan and the commit, so they stay in mode 0 with scale 1.  ``fn.mode_shares()`` as
    ``hybrid_policy_fn``'s (the planned robots' live robot-ticks; counted on the device, read when that is called).  ``steer``:
    the plan's goal is the ``local_goal`` handed in (a planner's subgoals) in place of the env's own."""
    from .hybrid import MODE_NAMES
    codes = torch.tensor(list(MODE_NAMES), dtype=torch.int32, device=env.device)
    counts = torch.zeros(len(MODE_NAMES), dtype=torch.int64, device=env.device)
    mode = torch.zeros(env.N, dtype=torch.int32, device=env.device)
    scale = torch.ones(env.N, dtype=torch.float32, device=env.device)
    pid = torch.zeros((env.N, 2), dtype=torch.float32, device=env.device)
    mask = planned = None
    if skip_first:
        planned = torch.arange(env.N, device=env.device) % env.R >= int(skip_first)
        mask = planned.to(torch.uint8).contiguous()

    def fn(obs, local_goal, speed):
        env.hybrid_plan(params, safe, mask=mask, mode=mode, scale=scale, pid=pid, goal=local_goal if steer else None)
        ring, head = ppo.policy_input(env, True)
        _mean, scaled = ppo.generate_action_no_sampling(policy, ring, local_goal, speed, ACTION_BOUND, fused=True, obs_head=head,
                                                        fused_bf16=fused_bf16, scan_scale=scale)
        a = env.hybrid_commit(scaled.float().contiguous(), mode, pid, safe, mask=mask)
        live = env.first_result == 0
        if planned is not None:
            live = live & planned
        counts.add_(((mode.unsqueeze(1) == codes) & live.unsqueeze(1)).sum(dim=0))
        return a
    fn.wants_obs = False

    def mode_shares():
        c = counts.tolist()
        total = sum(c)
        return {name: (n / total if total else None) for name, n in zip(MODE_NAMES.values(), c)}
    fn.mode_shares = mode_shares
    return fn


def planner_policy_fn(env, other, params=None, los=None):
    """The global planner under the controller function ``other`` (a checkpoint or a stand-in): the goal fields are planned at
    the first tick (``VecStageWorld.plan_goals``: the distinct goals of the env as they stand behind the reset), and every tick
    ``other`` is handed the robots' subgoals in their own frames (``VecStageWorld.subgoals``) in place of ``env.local_goal``.
    ``los`` (a ``planner.LosParams``): the subgoals with line of sight (``VecStageWorld.subgoals_los``) -- then ``other`` may
    be any controller that steers at the local goal it is handed (DWA and hybrid control with ``steer=True`` included).
    ``fn.report()`` -> the params, the status counts of the last tick and the mean path length at the first tick; with ``los``
    also its params and the mean (m, m_vis) over the live robot-ticks of the run (summed on the device, read when called)."""
    from .planner import STATUS_NAMES, PlannerParams
    params = params if params is not None else PlannerParams.for_grid(env.scenario.grid)
    state = {"fields": None, "first_dist": None}
    out = (torch.zeros((env.N, 2), dtype=torch.float32, device=env.device), torch.zeros((env.N, 2), dtype=torch.float32, device=env.device),
           torch.zeros(env.N, dtype=torch.float32, device=env.device), torch.zeros(env.N, dtype=torch.int32, device=env.device))
    if los is not None:
        out = out + (torch.zeros((env.N, 2), dtype=torch.int32, device=env.device),)
    ahead_sum = torch.zeros(3, dtype=torch.int64, device=env.device)         # m, m_vis, live robot-ticks

    def fn(obs, local_goal, speed):
        if state["fields"] is None:
            state["fields"] = env.plan_goals(params=params)
        if los is None:
            local, _sub, dist, _status = env.subgoals(state["fields"], out=out)
        else:
            local, _sub, dist, _status, ahead = env.subgoals_los(state["fields"], los, out=out)
            live = (env.first_result == 0).to(torch.int64)
            ahead_sum[:2].add_((ahead.to(torch.int64) * live.unsqueeze(1)).sum(dim=0))
            ahead_sum[2].add_(live.sum())
        if state["first_dist"] is None:
            finite = dist[torch.isfinite(dist)]
            state["first_dist"] = float(finite.mean()) if finite.numel() else None
        return other(obs, local, speed)
    fn.wants_obs = getattr(other, "wants_obs", True)

    def report():
        f = state["fields"]
        extra = {}
        if los is not None:
            m, m_vis, ticks = ahead_sum.tolist()
            extra = {"los_params": los.as_dict(), "planner_mean_ahead": [m / ticks, m_vis / ticks] if ticks else None}
        return {**extra, "planner_params": params.as_dict(),
                "planner_goals": None if f is None else f.num_goals, "planner_rounds": None if f is None else f.rounds,
                "planner_status_last_tick": {name: int((out[3] == code).sum()) for code, name in STATUS_NAMES.items()},
                "planner_mean_initial_path_m": state["first_dist"]}
    fn.report = report
    return fn


def perturbed_start(env, jitter_xy, jitter_th, seed):
    """Start poses of a circle world with every robot moved off its table pose by U(-jitter_xy, jitter_xy) metres in x
    and y and U(-jitter_th, jitter_th) radians of heading -- drawn from a Philox generator seeded with ``seed``, so that
    W circles are W DIFFERENT scenarios (the reference's table, model/utils.py:6-38, is one perfectly symmetric
    scenario: a deterministic policy either solves all of its copies or none).  Goals stay the table's.
    -> (poses f32[N,3], goals f32[N,2]) on the env's device."""
    sc = env.scenario
    dev = env.local_goal.device
    W, R = sc.num_worlds, sc.robots_per_world
    base = torch.as_tensor(sc.init_table, dtype=torch.float32, device=dev).unsqueeze(0).expand(W, R, 3)
    goal = torch.as_tensor(sc.goal_table, dtype=torch.float32, device=dev).unsqueeze(0).expand(W, R, 2)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    u = torch.rand(W, R, 3, generator=g, device=dev) * 2.0 - 1.0
    scale = torch.tensor([jitter_xy, jitter_xy, jitter_th], dtype=torch.float32, device=dev)
    poses = base + u * scale
    poses[..., 2] = torch.atan2(torch.sin(poses[..., 2]), torch.cos(poses[..., 2]))
    return poses.reshape(W * R, 3).contiguous(), goal.reshape(W * R, 2).contiguous()


def scattered_start(env, params=None, face_goal=False):
    """Start poses and goals of every world from the scenario sampler (``VecStageWorld.scatter`` on the scenario's boxes):
    W worlds are W different scenarios, reproducible bit for bit from (seed, ``params.draw``).  A robot for which none of
    ``max_tries`` candidates qualified would start on top of another or in a wall: that is an error here, not a scenario.
    ``face_goal``: the start heading is turned towards the robot's own goal, with torch on the device -- OUTSIDE the bit-pinned
    rule (atan2 is the runtime's).  -> (poses f32[N,3], goals f32[N,2], tries i32[N,2]) on the env's device."""
    poses, goals, tries = env.scatter(params=params)
    failed = (tries < 0).any(dim=1)
    if bool(failed.any()):
        n = int(failed.nonzero()[0, 0])
        raise RuntimeError(f"scatter: no candidate qualified for {int(failed.sum())} of {env.N} robots (the first: world {n // env.R}, "
                           f"local index {n % env.R}) -- fewer robots, a smaller min_sep / clear_cells or more max_tries")
    if face_goal:
        poses[:, 2] = torch.atan2(goals[:, 1] - poses[:, 1], goals[:, 0] - poses[:, 0])
    return poses, goals, tries


def circle_test(env, policy_fn, max_ticks=1200, perturb=None, seed=0, recorder=None, start=None):
    """Runs the circle scenario on ``env`` (any object with the VecStageWorld surface) and returns
    the metrics dict.  Mirrors circle_test.py:52-80: deterministic action, and a robot whose last
    ``get_reward_and_terminate`` said terminal gets v = 0 (``real_action[0] = 0``, :64-65).
    ``perturb = (jitter_xy, jitter_th)``: every circle starts from its own jittered poses (``perturbed_start``); the
    metrics then carry the mean success rate over circles with a 95 % interval.
    ``recorder``: a ``render.Recorder`` whose ``tick(k)`` is called before tick k (pictures of the run, gathered on the device;
    it reads the env and writes nothing of it, so the metrics are the same with and without).
    ``start = (poses, goals)``: the start state itself, float32[N,3] and float32[N,2] on the env's device (``scattered_start``);
    excludes ``perturb``."""
    if start is not None:
        assert perturb is None, "start and perturb are two start states"
        env.reset(None, start[0], start[1])
    elif perturb is None:
        env.reset()
    else:
        poses, goals = perturbed_start(env, perturb[0], perturb[1], seed)
        env.reset(None, poses, goals)
    N = env.N
    dev = env.local_goal.device
    ticks_to_goal = torch.zeros(N, device=dev)
    path = torch.zeros(N, device=dev)
    last_terminal = torch.zeros(N, dtype=torch.bool, device=dev)
    for k in range(max_ticks):
        if recorder is not None:
            recorder.tick(k)
        a = policy_fn(env.obs if getattr(policy_fn, "wants_obs", True) else None, env.local_goal, env.speed).float().clone()
        a[:, 0] = torch.where(last_terminal, torch.zeros_like(a[:, 0]), a[:, 0])
        pending = env.first_result == 0
        env.step(a.contiguous())
        last_terminal = env.done.bool().clone()
        path += torch.where(pending, env.speed_gt[:, 0] * 0.1, torch.zeros_like(path))
        ticks_to_goal += pending.float()
        if k % 25 == 24 and bool((env.first_result != 0).all()):    # one host round trip every 25 ticks
            break
    if hasattr(env, "check"):
        env.check()          # mrca_check: raises if a device-side pass flagged an untrusted state (worlds with > 64 robots)
    fr = env.first_result
    reach = fr == 1
    n_reach = int(reach.sum())
    # the paper's metrics (Long et al. 2018, Sec. V-B) over the robots that reached their goal; the straight
    # line is |goal - init| - goal radius (0.5 m) at the speed limit of 1 m/s, one tick = 0.1 s
    straight = ((env.goal - env.init_pose[:, :2]).norm(dim=1) - 0.5).clamp(min=0.0)
    time_s = ticks_to_goal * 0.1
    extra_time = (time_s - straight / 1.0)[reach]
    extra_dist = (path - straight)[reach]
    avg_speed = (path / time_s.clamp(min=0.1))[reach]
    R = getattr(getattr(env, "scenario", None), "robots_per_world", None)
    per_circle = {}
    if R and N % R == 0 and N // R > 1:
        # the circle is the unit of randomisation: mean of the per-circle success fractions, normal 95 % interval of
        # that mean (robots of one circle succeed or fail together far too often to count as independent samples)
        sr = reach.view(N // R, R).float().mean(dim=1)
        sd = float(sr.std(unbiased=True))
        half = 1.96 * sd / math.sqrt(N // R)
        per_circle = {"circles": N // R, "success_rate_ci95": [max(0.0, float(sr.mean()) - half), min(1.0, float(sr.mean()) + half)],
                      "circles_fully_solved": float((sr == 1.0).float().mean()), "worst_circle": float(sr.min())}
    by_group = {}
    for name, sel in (getattr(policy_fn, "groups", None) or {}).items():      # (a mixed run: the same metrics per group)
        g_reach = reach & sel
        g_n = int(g_reach.sum())
        by_group[name] = {
            "robots": int(sel.sum()), "success_rate": g_n / max(1, int(sel.sum())),
            "crash_rate": float((fr[sel] == 2).float().mean()), "timeout_rate": float((fr[sel] == 3).float().mean()),
            "unfinished_rate": float((fr[sel] == 0).float().mean()),
            "extra_time_s": float((time_s - straight / 1.0)[g_reach].mean()) if g_n else None,
            "extra_distance_m": float((path - straight)[g_reach].mean()) if g_n else None,
            "average_speed_mps": float((path / time_s.clamp(min=0.1))[g_reach].mean()) if g_n else None,
        }
    return {
        **per_circle,
        **({"groups": by_group} if by_group else {}),
        "robots": N, "ticks_run": k + 1,
        "success_rate": n_reach / N,
        "crash_rate": float((fr == 2).float().mean()),
        "timeout_rate": float((fr == 3).float().mean()),
        "unfinished_rate": float((fr == 0).float().mean()),
        "mean_ticks_to_goal": float(ticks_to_goal[reach].mean()) if n_reach else None,
        "mean_path_ratio": float((path[reach] / straight[reach].clamp(min=1e-6)).mean()) if n_reach else None,
        "extra_time_s": float(extra_time.mean()) if n_reach else None,
        "extra_distance_m": float(extra_dist.mean()) if n_reach else None,
        "average_speed_mps": float(avg_speed.mean()) if n_reach else None,
    }


def main():
    ap = argparse.ArgumentParser(description="circle test (circle_test.py) at scale on the MI355X env")
    ap.add_argument("--circles", type=int, default=1, help="independent 50-robot circles (50 -> 50 000 robots: 1000)")
    ap.add_argument("--policy", default=None, help="state_dict file with the reference's keys (policy/stage2.pth)")
    ap.add_argument("--max-ticks", type=int, default=1200)   # circle_world.py:198 allows 10000
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--robots", type=int, default=None, help="robots per circle (default 50 = the reference's table; others: "
                                                             "scenario.circle_n) or per doorway room (default 12, at most 24)")
    ap.add_argument("--scenario", default="circle", choices=["circle", "doorway"] + sorted(SCATTER_SCENARIOS),
                    help="doorway: scenario.doorway, --circles rooms split by a wall whose one door lies on no robot's straight line "
                         "to its goal (excludes --radius / --one-circle / --stage-resolution); random / swap / crossing / corridor: "
                         "the paper's other scenarios (scenario.random_box, group_swap, group_crossing, corridor), --circles worlds "
                         "of --robots robots (default 20; crossing 12) whose starts and goals the scenario sampler draws per world "
                         "(mrca_scatter); same exclusions, and --perturb")
    ap.add_argument("--scatter-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_scatter_params on top of the scenario's, e.g. min_sep=0.8 (repeatable)")
    ap.add_argument("--scatter-draw", type=int, default=None, metavar="D",
                    help="the scenario number of the sampler: another draw, another set of worlds (default: --seed)")
    ap.add_argument("--face-goal", action="store_true",
                    help="scattered starts face their own goal (set with torch behind the sampler: not part of its bit-pinned rule)")
    ap.add_argument("--planner", action="store_true",
                    help="the global planner under --policy P [--fused | --fused-bf16] or the stand-in: goal fields planned once "
                         "(mrca_goal_fields), the controller handed each robot's subgoal (mrca_subgoals) in place of the local goal; "
                         "the result line gains planner_params, the status counts of the last tick and the mean initial path length")
    ap.add_argument("--planner-los", action="store_true",
                    help="the global planner with line of sight (mrca_subgoals_los): implies --planner, takes --planner-param too, and "
                         "goes under --dwa / --dwa-first / --hybrid / --hybrid-safe as well (their kernels are handed the subgoal: "
                         "mrca_dwa_actions_goal, mrca_hybrid_actions_goal, mrca_hybrid_plan_goal), not under --orca / --orca-first; "
                         "the result line gains los_params and planner_mean_ahead = the mean (m, m_vis) over the run")
    ap.add_argument("--los-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_los_params on top of LosParams.for_grid of the map, e.g. reach=40 (repeatable)")
    ap.add_argument("--planner-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_planner_params on top of PlannerParams.for_grid of the map, e.g. lookahead=10 (repeatable)")
    ap.add_argument("--radius", type=float, default=25.0)
    ap.add_argument("--one-circle", type=int, default=None, metavar="N",
                    help="ONE circle of N robots in an open world (scenario.circle_big: the radius grows with N so that the "
                         "spacing along the circle stays --spacing); excludes --circles / --robots / --radius")
    ap.add_argument("--spacing", type=float, default=None, metavar="S",
                    help="with --one-circle: metres between neighbours along the circle (default: the reference's 3.14)")
    ap.add_argument("--perturb", default=None, help="'dxy,dth': start every robot U(-dxy, dxy) m / U(-dth, dth) rad off its table "
                                                     "pose (Philox, seeded by --seed) so that the circles are different scenarios, "
                                                     "e.g. 0.2,0.1; the output carries the mean success rate with a 95 %% interval")
    ap.add_argument("--stage-resolution", action="store_true", help="fidelity mode: the map at Stage's own cell size "
                                                                      "(worlds/circle.world:3) -- the clearances a Stage-trained policy lives with")
    ap.add_argument("--fused", action="store_true", help="policy inference through the fp32 HIP conv front end")
    ap.add_argument("--fused-bf16", action="store_true", help="policy inference through the bf16 MFMA front end and a bf16 "
                                                              "fc1 (opt-in precision, not the reference's; implies --fused)")
    ap.add_argument("--orca", action="store_true", help="every robot driven by the ORCA baseline controller on the device "
                                                        "(mrca_orca_actions); no --policy is needed")
    ap.add_argument("--orca-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_orca_params, e.g. radius=0.4 (repeatable)")
    ap.add_argument("--orca-first", type=int, default=None, metavar="K",
                    help="robots with local index < K are driven by ORCA, the rest by --policy (or the stand-in); the metrics "
                         "are reported for both groups")
    ap.add_argument("--nh-orca", action="store_true",
                    help="every robot driven by the NH-ORCA baseline controller on the device (mrca_nhorca_actions: ORCA over the "
                         "velocities a unicycle tracks within a bound, worlds of any size); no --policy is needed; the result "
                         "line gains nhorca_params and nhorca_modes (the share of live robot-ticks per mode); excluded where "
                         "--orca is")
    ap.add_argument("--nh-orca-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_nhorca_params, e.g. track_error=0.1 (repeatable)")
    ap.add_argument("--nh-orca-first", type=int, default=None, metavar="K",
                    help="robots with local index < K are driven by NH-ORCA, the rest by --policy (or the stand-in); the metrics "
                         "are reported for both groups")
    ap.add_argument("--dwa", action="store_true", help="every robot driven by the DWA baseline controller on the device "
                                                       "(mrca_dwa_actions: sensor-level, worlds of any size); no --policy is needed")
    ap.add_argument("--dwa-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_dwa_params, e.g. horizon=1.5 (repeatable)")
    ap.add_argument("--dwa-first", type=int, default=None, metavar="K",
                    help="robots with local index < K are driven by DWA, the rest by --policy, --orca or the stand-in; the "
                         "metrics are reported for both groups")
    ap.add_argument("--hybrid", action="store_true", help="hybrid control (mrca_hybrid_actions) behind whatever controller the other "
                                                          "flags select: a PID law where the way to the goal is free, the command "
                                                          "scaled down where something is dangerously close, the command as it is "
                                                          "elsewhere; the result line gains hybrid_params and hybrid_modes (the share "
                                                          "of live robot-ticks per mode)")
    ap.add_argument("--hybrid-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_hybrid_params, e.g. risk_dist=0.8 (repeatable)")
    ap.add_argument("--hybrid-safe", action="store_true",
                    help="hybrid control in the paper's form (mrca_hybrid_plan, mrca_hybrid_commit): the robots of mode 2 are driven "
                         "by the network on a rescaled scan, in the same forward as everybody else's, v capped; needs --policy P "
                         "--fused (or --fused-bf16); --hybrid-param is taken for the classification; the result line gains "
                         "hybrid_safe_params, hybrid_params and hybrid_modes")
    ap.add_argument("--hybrid-safe-param", action="append", default=[], metavar="NAME=VALUE",
                    help="a field of mrca_safe_policy_params, e.g. scan_scale=0.7 (repeatable)")
    ap.add_argument("--lidar-noise", default=None, metavar="const=M,prop=P,dropout=Q[,quantum=M]",
                    help="the lidar noise model (mrca_scan_noise) behind every ray cast: range noise of const + prop * range metres "
                         "(an Irwin-Hall deviate of unit variance), beams lost with probability dropout, a read-out step of quantum "
                         "metres; what is not named is 0, 'default' takes the library's defaults.  Every controller reads the noisy "
                         "scans; the result line carries the params as lidar_noise")
    ap.add_argument("--render", default=None, metavar="PATH", help="write pictures of the run (top-down views with trails, rendered on "
                                                                    "the device and copied to the host once after the last tick): "
                                                                    "an animated GIF, or PATH.npz where PIL is missing")
    ap.add_argument("--render-worlds", default=None, help="the circles to show, e.g. 0,1,7 (default: the first 16)")
    ap.add_argument("--render-every", type=int, default=10, help="one frame every K ticks")
    ap.add_argument("--render-size", type=int, default=256, help="pixels per side of one circle's picture")
    a = ap.parse_args()
    if a.fused_bf16:
        a.fused = True
    if (a.nh_orca or a.nh_orca_first is not None) and (a.orca or a.orca_first is not None):
        ap.error("--nh-orca / --nh-orca-first and --orca / --orca-first are two baselines for the same robots: choose one")
    if a.nh_orca_param and not (a.nh_orca or a.nh_orca_first is not None):
        ap.error("--nh-orca-param goes with --nh-orca or --nh-orca-first")
    # (NH-ORCA steers at MRCA_F_GOAL like ORCA: what excludes --orca / --orca-first below excludes it)
    orca_all = a.orca or a.nh_orca
    orca_first = a.orca_first if a.nh_orca_first is None else a.nh_orca_first
    from .vec_env import VecStageWorld
    doorway = a.scenario == "doorway"
    scattered = a.scenario in SCATTER_SCENARIOS
    if scattered and (a.radius != 25.0 or a.one_circle is not None or a.stage_resolution or a.perturb):
        ap.error(f"--scenario {a.scenario} excludes --radius / --one-circle / --stage-resolution / --perturb")
    if not scattered and (a.scatter_param or a.scatter_draw is not None or a.face_goal):
        ap.error("--scatter-param / --scatter-draw / --face-goal go with --scenario " + " / ".join(sorted(SCATTER_SCENARIOS)))
    if scattered and (a.planner or a.planner_los) and a.scenario != "corridor":
        ap.error("--planner / --planner-los: of the scattered scenarios only the corridor has something to plan around")
    if doorway and (a.radius != 25.0 or a.one_circle is not None or a.stage_resolution):
        ap.error("--scenario doorway excludes --radius / --one-circle / --stage-resolution")
    if a.robots is None:
        a.robots = 12 if doorway or a.scenario == "crossing" else (20 if scattered else 50)
    if a.planner_param and not (a.planner or a.planner_los):
        ap.error("--planner-param goes with --planner")
    if a.los_param and not a.planner_los:
        ap.error("--los-param goes with --planner-los")
    if a.planner_los and (orca_all or orca_first is not None):
        ap.error("--planner-los: ORCA steers at the goal in the world frame (MRCA_F_GOAL), it takes no subgoal: not with --orca / "
                 "--orca-first / --nh-orca / --nh-orca-first")
    steer = a.planner_los
    if a.planner and not a.planner_los and (orca_all or a.dwa or a.hybrid or a.hybrid_safe or orca_first is not None or a.dwa_first is not None):
        ap.error("--planner hands the subgoal to a controller that takes the local goal as an argument (--policy, the stand-in): the "
                 "kernels of --orca / --dwa / --hybrid / --hybrid-safe read the env's own local goal")
    if a.hybrid_safe_param and not a.hybrid_safe:
        ap.error("--hybrid-safe-param goes with --hybrid-safe")
    if a.hybrid_safe:
        if a.hybrid:
            ap.error("--hybrid-safe is hybrid control in the paper's form, --hybrid the command scaling: choose one")
        if orca_all or a.dwa:
            ap.error("--hybrid-safe rescales the scan a checkpoint sees: not with --orca / --dwa (use --orca-first / --dwa-first "
                     "for mixed groups)")
        if not a.policy:
            ap.error("--hybrid-safe needs --policy P: the stand-in reads no rescaled scan")
        if not a.fused:
            ap.error("--hybrid-safe needs --fused (or --fused-bf16): the scan is rescaled while the fused front end stages it")
    if a.one_circle is None and a.spacing is not None:
        ap.error("--spacing goes with --one-circle")
    if a.one_circle is not None:
        if a.circles != 1 or a.robots != 50 or a.radius != 25.0:
            ap.error("--one-circle excludes --circles / --robots / --radius")
        if a.stage_resolution:
            ap.error("--one-circle runs in an open world: no --stage-resolution")
        if a.one_circle < 1:
            ap.error("--one-circle needs at least one robot")
        sc = scenario.circle_big(a.one_circle, seed=a.seed, spacing=a.spacing)
    elif doorway:
        try:
            sc = scenario.doorway(num_worlds=a.circles, robots=a.robots, seed=a.seed, timeout=a.max_ticks)
        except ValueError as e:
            ap.error(str(e))
    elif scattered:
        try:
            overrides = {}
            for it in a.scatter_param:        # (min_sep is the constructor's: its coverage rule is judged with it)
                if it.partition("=")[0] == "min_sep" and it.partition("=")[1]:
                    overrides["min_sep"] = float(it.partition("=")[2])
            sc = getattr(scenario, SCATTER_SCENARIOS[a.scenario])(robots=a.robots, num_worlds=a.circles, seed=a.seed, timeout=a.max_ticks,
                                                                 **overrides)
        except ValueError as e:
            ap.error(str(e))
    elif a.robots == 50 and a.radius == 25.0:
        sc = scenario.circle(num_worlds=a.circles, seed=a.seed, stage_resolution=a.stage_resolution)
    else:
        grid = scenario.load_map("circle_rink_r0010") if a.stage_resolution else None
        sc = scenario.circle_n(a.robots, a.radius, num_worlds=a.circles, seed=a.seed, grid=grid)
    noise = None
    if a.lidar_noise is not None:
        from .noise import ScanNoiseParams
        try:
            noise = ScanNoiseParams.from_assignments(a.lidar_noise)
        except ValueError as e:
            ap.error(str(e))
    env = VecStageWorld(sc, **({} if noise is None else {"scan_noise": noise}))
    scatter_params = None
    if scattered:
        from .scatter import ScatterParams
        try:
            scatter_params = ScatterParams.from_assignments(
                a.scatter_param, start=dict(sc.scatter, draw=(a.seed if a.scatter_draw is None else a.scatter_draw) & 0xFFFFFFFF))
        except ValueError as e:
            ap.error(str(e))
    if a.policy:
        pol = CNNPolicy(3, 2).to(env.device)
        pol.load_state_dict(torch.load(a.policy, map_location=env.device))
        fn, name = cnn_policy_fn(pol, fused=a.fused, env=env, fused_bf16=a.fused_bf16), a.policy
        if a.hybrid_safe:
            from .hybrid import HybridParams, SafePolicyParams
            try:
                hybrid_params = HybridParams.from_assignments(a.hybrid_param)
                safe_params = SafePolicyParams.from_assignments(a.hybrid_safe_param)
            except ValueError as e:
                ap.error(str(e))
            fn = safe_policy_fn(pol, env, hybrid_params, safe_params, fused_bf16=a.fused_bf16,
                                skip_first=max(orca_first or 0, a.dwa_first or 0), steer=steer)
            safe_fn, name = fn, f"hybrid control in the paper's form (mrca_hybrid_plan, mrca_hybrid_commit) around {name}"
    elif doorway:
        fn, name = go_to_goal_policy, "go-to-goal stand-in (no checkpoint given)"
    else:
        fn, name = staggered_roundabout_policy(env.N), "staggered-roundabout stand-in (no checkpoint given)"
    los_params = None
    if a.planner or a.planner_los:
        from .planner import LosParams, PlannerParams
        try:
            planner_params = PlannerParams.from_assignments(a.planner_param, base=PlannerParams.for_grid(sc.grid))
            if a.planner_los:
                los_params = LosParams.from_assignments(a.los_param, base=LosParams.for_grid(sc.grid))
        except ValueError as e:
            ap.error(str(e))
        ahead_m = planner_params.lookahead * planner_params.stride * sc.grid.cell
        if a.planner_los and (a.dwa or a.dwa_first is not None or a.hybrid or a.hybrid_safe) and ahead_m <= 0.5:
            ap.error(f"--planner-los under --dwa / --hybrid: a subgoal within 0.5 m stops these controllers, and lookahead x cell "
                     f"is {ahead_m:g} m: raise --planner-param lookahead")
    if a.planner and not a.planner_los:
        fn = planner_fn = planner_policy_fn(env, fn, planner_params)
        name = f"global planner (mrca_goal_fields, mrca_subgoals) under {name}"
    orca_call = "mrca_orca_actions_any" if env.R > 64 else "mrca_orca_actions"
    if a.orca or a.orca_first is not None:
        from .orca import OrcaParams
        params = OrcaParams.from_assignments(a.orca_param)
        if a.orca_first is None:
            fn, name = orca_policy_fn(env, params), f"ORCA baseline ({orca_call})"
        else:
            fn, name = orca_policy_fn(env, params, first=a.orca_first, other=fn), f"ORCA for local index < {a.orca_first}, else {name}"
    if a.nh_orca or a.nh_orca_first is not None:
        from .nhorca import NhOrcaParams
        try:
            nh_params = NhOrcaParams.from_assignments(a.nh_orca_param)
        except ValueError as e:
            ap.error(str(e))
        if a.nh_orca_first is None:
            fn, name = nhorca_policy_fn(env, nh_params), "NH-ORCA baseline (mrca_nhorca_actions)"
        else:
            fn = nhorca_policy_fn(env, nh_params, first=a.nh_orca_first, other=fn)
            name = f"NH-ORCA for local index < {a.nh_orca_first}, else {name}"
        nh_fn = fn
    if a.dwa and (orca_all or orca_first is not None):
        ap.error("--dwa drives every robot: with --orca / --nh-orca use --dwa-first K")
    if a.dwa or a.dwa_first is not None:
        from .dwa import DwaParams
        dwa_params = DwaParams.from_assignments(a.dwa_param)
        if a.dwa_first is None:
            fn, name = dwa_policy_fn(env, dwa_params, steer=steer), "DWA baseline (mrca_dwa_actions)"
        else:
            fn = dwa_policy_fn(env, dwa_params, first=a.dwa_first, other=fn, other_name="orca" if a.orca else ("nhorca" if a.nh_orca else "policy"), steer=steer)
            name = f"DWA for local index < {a.dwa_first}, else {name}"
    if a.hybrid_param and not (a.hybrid or a.hybrid_safe):
        ap.error("--hybrid-param goes with --hybrid or --hybrid-safe")
    if a.hybrid:
        from .hybrid import HybridParams
        try:
            hybrid_params = HybridParams.from_assignments(a.hybrid_param)
        except ValueError as e:
            ap.error(str(e))
        fn, name = hybrid_policy_fn(env, fn, hybrid_params, steer=steer), f"hybrid control (mrca_hybrid_actions) behind {name}"
    if a.planner_los:
        # outermost: every controller below is handed the subgoal where it would read the env's local goal
        inner = fn
        fn = planner_fn = planner_policy_fn(env, inner, planner_params, los_params)
        for attr in ("groups", "mode_shares"):
            if hasattr(inner, attr):
                setattr(fn, attr, getattr(inner, attr))
        name = f"global planner with line of sight (mrca_goal_fields, mrca_subgoals_los) under {name}"
    perturb = tuple(float(v) for v in a.perturb.split(",")) if a.perturb else None
    recorder = None
    if a.render:
        from .render import Recorder, save_frames
        worlds = [int(w) for w in a.render_worlds.split(",")] if a.render_worlds else None
        recorder = Recorder(env, worlds, a.render_every, a.render_size)
    start = tries = None
    if scattered:
        try:
            poses, goals, tries = scattered_start(env, scatter_params, a.face_goal)
        except RuntimeError as e:       # the library's validation text, or robots that found no place
            ap.error(str(e))
        start = (poses, goals)
    out = circle_test(env, fn, a.max_ticks, perturb=perturb, seed=a.seed, recorder=recorder, start=start)
    if recorder is not None:      # (reported on stderr: the result line is the same with and without --render)
        frames = recorder.frames()
        print(f"{len(frames)} frames -> {save_frames(frames, a.render)}", file=sys.stderr)
    out["policy"] = name
    if a.orca or a.orca_first is not None:
        import dataclasses
        out["orca_params"] = dataclasses.asdict(params)
    if a.nh_orca or a.nh_orca_first is not None:
        import dataclasses
        out["nhorca_params"] = dataclasses.asdict(nh_params)
        out["nhorca_modes"] = nh_fn.mode_shares()
    if a.dwa or a.dwa_first is not None:
        import dataclasses
        out["dwa_params"] = dataclasses.asdict(dwa_params)
    if a.hybrid:
        import dataclasses
        out["hybrid_params"] = dataclasses.asdict(hybrid_params)
        out["hybrid_modes"] = fn.mode_shares()
    if a.hybrid_safe:
        import dataclasses
        out["hybrid_safe_params"] = dataclasses.asdict(safe_params)
        out["hybrid_params"] = dataclasses.asdict(hybrid_params)
        out["hybrid_modes"] = safe_fn.mode_shares()
    if a.planner or a.planner_los:
        out.update(planner_fn.report())
    if doorway or scattered:
        out["scenario"] = a.scenario
    if scattered:
        out["scatter_params"], out["scatter_draw"] = scatter_params.as_dict(), scatter_params.draw
        out["scatter_max_tries_used"], out["face_goal"] = int(tries.max()), bool(a.face_goal)
    out["lidar_noise"] = None if noise is None else noise.as_dict()
    out["robots_per_circle"], out["radius_m"] = a.robots, a.radius
    if a.one_circle is not None:
        out["one_circle"], out["robots_per_circle"] = a.one_circle, a.one_circle
        out["radius_m"] = float(max(abs(float(v)) for v in sc.init_table[0][:2]))     # (robot 0 stands at (radius, 0))
        out["spacing_m"] = 2.0 * math.pi * out["radius_m"] / a.one_circle
    out["perturb_xy_th"], out["seed"], out["stage_resolution"] = perturb, a.seed, bool(a.stage_resolution)
    out["inference_precision"] = ("bf16 (fused bf16 MFMA front end + bf16 fc1)" if a.fused_bf16 else "fp32") if a.policy else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
