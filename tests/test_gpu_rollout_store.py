"""GPU: the library's two rollout-buffer stores (csrc/mrca_rollout_store.hip: rollout_store_state_kernel,
rollout_store_outcome_kernel) against the reference's buffer (tests/rollout_ref.py: a list of whole stacks, stacked), on bits.

No policy in the loop (a - c): per tick ``rollout_store_state``, ``step``, ``rollout_store_outcome`` with seeded stand-ins for
the policy's outputs; the C oracle steps in lock-step with the same clipped actions and feeds the model.  The shapes are the
ones at which the kernels' riskier code runs: two workgroups of the outcome kernel with the second nearly empty (259 and 264
robots), the same ticks replayed as hipGraphs of one and of eight ticks, and the state kernel above its grid cap (16 416
robots: a thread serves more than one column).  (d) goes through ``Stage1Trainer.run`` on a Stage-2 env.

Before every horizon the buffer is filled with a pattern no store writes, so a row a kernel skipped cannot pass on what an
earlier horizon (or an earlier test, through the allocator) left there."""
import numpy as np
import pytest
import torch

import rollout_ref as R
import util as U
from util import O

pytestmark = pytest.mark.gpu

FIELDS = ("goal", "speed", "action", "logprob", "value", "reward", "done")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def _poison(buf):
    """Every tensor the stores write -> a pattern they never write: a NaN with a payload, 0xAB for the flags, and row 0 three
    times over for a stack's row indices (a stack no tick has: at tick 0 the rows are 0 .. F-1, later ones name later rows)."""
    for k in ("frames", "goal", "speed", "action", "logprob", "value", "reward"):
        getattr(buf, k).view(torch.int32).fill_(0x7FCDEAD0)
    buf.done.fill_(0xAB)
    buf.fidx.zero_()


def _host(buf, rows=None):
    out = {k: getattr(buf, k)[:rows].cpu().numpy() for k in FIELDS}
    out["obs"] = buf.obs_rows().materialise()[:rows].cpu().numpy()
    return out


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bounds():
    lo, hi = R.ACTION_BOUND
    return torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")


def _new_buffer(env, T):
    from mrca import ppo
    buf = ppo.RolloutBuffer(T, env.N, env.F, env.B, env.device, single_frame=True)
    buf.bind_env(env)
    return buf, torch.zeros(1, dtype=torch.int64, device=env.device)


def _store_tick(env, buf, tick, a, lp, v, lo, hi):
    """The tick body: the state store, the step with the clipped action, the outcome store (which moves ``tick`` on)."""
    env.rollout_store_state(buf._rows, tick, a, lp, v)
    cmd = torch.minimum(torch.maximum(a, lo), hi).contiguous()
    env.step(cmd)
    env.rollout_store_outcome(buf._rows, tick, buf._ticket)
    return cmd


def _copy_state(env, ora):
    """The env's state into the C oracle (as test_fp64_oracle_one_tick_from_identical_state does): restart draws are Philox
    counters of (robot, episode, draw), so identical counters give identical restarts from here on."""
    torch.cuda.synchronize()
    for k in U.STATE_FIELDS + ["fresh"]:
        x = getattr(env, k).cpu().numpy()
        getattr(ora, k)[...] = x.astype(getattr(ora, k).dtype)


def _oracle_tick(ora, model, log, a, lp, v):
    """One tick of the oracle feeding the model; the oracle's flags and stacks into ``log`` for rollout_ref.coverage."""
    model.append(ora.obs, ora.local_goal, ora.speed, a, lp, v)
    log["fresh"].append(ora.fresh.copy())
    log["obs"].append(ora.obs.copy())
    ora.step(R.clip_action(a))
    model.outcome(ora.reward, ora.done)
    log["done"].append(ora.done.copy())


def _check_horizon(buf, model, log, T, what):
    """Every tensor of the buffer against the model; the newest frame of tick t in row t + F - 1."""
    F = buf.nframes
    R.assert_same(model.arrays(), _host(buf), what)
    frames = buf.frames.cpu().numpy()
    for t in range(T):
        assert R.same_bits(frames[t + F - 1], log["obs"][len(log["obs"]) - T + t][:, F - 1]), (what, t)


def _coverage(sc, T, log):
    R.coverage(sc, T, np.array(log["fresh"]), np.array(log["done"]), np.array(log["obs"]))


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("T", [1, 2, 12])
@pytest.mark.parametrize("name", ["stage1", "stage2", "stage2_hold"])
def test_stores_with_two_outcome_workgroups_equal_the_reference_buffer(hip, name, T):
    """259 / 264 robots: the outcome kernel runs two workgroups, the second with 3 / 8 robots; whichever takes the second
    ticket moves the counter on and re-arms the ticket.  Three horizons in a row, ``begin_horizon`` and a zeroed counter between
    them as the trainer does; after every tick the counter reads t + 1 and the ticket 0; after every horizon every tensor of
    the buffer equals the model, special bit patterns of logprob / value included."""
    sc, lead = R.scenario(name, T)
    env, ora = hip.VecStageWorld(sc), U.COracleEnv(sc)
    env.reset()
    ora.reset()
    rng = np.random.default_rng(7)
    lo, hi = _bounds()
    for _ in range(lead):
        cmd = R.clip_action(R.policy_outputs(rng, env.N)[0])
        env.step(_dev(cmd))
        ora.step(cmd)
    buf, tick = _new_buffer(env, T)
    log = {"fresh": [], "done": [], "obs": []}
    for h in range(3):
        _poison(buf)
        buf.begin_horizon(env.obs)
        tick.zero_()
        model = R.RefRollout()
        for t in range(T):
            a, lp, v = R.policy_outputs(rng, env.N)
            cmd = _store_tick(env, buf, tick, _dev(a), _dev(lp), _dev(v), lo, hi)
            assert int(tick) == t + 1 and int(buf._ticket) == 0, (h, t)
            assert R.same_bits(cmd.cpu().numpy(), R.clip_action(a))
            _oracle_tick(ora, model, log, a, lp, v)
        _check_horizon(buf, model, log, T, f"{name} T={T} horizon {h}")
    torch.cuda.synchronize()
    U.assert_state_equal(U.HostView(env), ora, what=f"{name} T={T}: the env after the run")
    env.check()
    _coverage(sc, T, log)
    env.close()


# ---------------------------------------------------------------------------------------------- (b)
def test_captured_ticks_fill_the_buffer_as_the_reference_does(hip):
    """The tick body (two stores and a step) captured once as one tick and once as eight, as ``Stage1Trainer._capture`` does:
    timing off, warm-up on the capture stream.  Stage-2 at 264 robots, T = 12: one replay of eight ticks -- sixteen store
    launches on one ticket and one counter -- then four of one; two horizons, so that a horizon starts on carried frames."""
    T, run = 12, 8
    sc, lead = R.scenario("stage2", T)
    env, ora = hip.VecStageWorld(sc), U.COracleEnv(sc)
    env.reset()
    env.enable_timing(False)
    N = env.N
    rng = np.random.default_rng(7)
    lo, hi = _bounds()
    buf, tick = _new_buffer(env, T)
    act = torch.zeros(run, N, 2, device="cuda")
    lps, vals = torch.zeros(run, N, device="cuda"), torch.zeros(run, N, device="cuda")

    def body(i):
        _store_tick(env, buf, tick, act[i], lps[i], vals[i], lo, hi)

    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        for _ in range(lead):                       # (these ticks advance the env; all write row 0, which is poisoned below)
            act[0].copy_(_dev(R.policy_outputs(rng, N)[0]))
            tick.zero_()
            body(0)
    torch.cuda.current_stream(env.device).wait_stream(side)
    tick.zero_()
    g1, g8 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1, stream=side):
        body(0)
    with torch.cuda.graph(g8, stream=side):
        for i in range(run):
            body(i)
    env.invalidate_views()
    _copy_state(env, ora)
    log = {"fresh": [], "done": [], "obs": []}
    for h in range(2):
        _poison(buf)
        buf.begin_horizon(env.obs)
        tick.zero_()
        model = R.RefRollout()
        draws = [R.policy_outputs(rng, N) for _ in range(T)]
        for dst, j in ((act, 0), (lps, 1), (vals, 2)):
            dst.copy_(_dev(np.stack([d[j] for d in draws[:run]])))
        g8.replay()
        env.invalidate_views()
        assert int(tick) == run and int(buf._ticket) == 0, h
        for t in range(run, T):
            for dst, j in ((act, 0), (lps, 1), (vals, 2)):
                dst[0].copy_(_dev(draws[t][j]))
            g1.replay()
            env.invalidate_views()
            assert int(tick) == t + 1 and int(buf._ticket) == 0, (h, t)
        for a, lp, v in draws:
            _oracle_tick(ora, model, log, a, lp, v)
        _check_horizon(buf, model, log, T, f"captured, horizon {h}")
    torch.cuda.synchronize()
    U.assert_state_equal(U.HostView(env), ora, what="captured: the env after the run")
    env.check()
    _coverage(sc, T, log)
    env.close()


# ---------------------------------------------------------------------------------------------- (c)
def test_state_store_above_its_grid_cap(hip):
    """513 x 32 = 16 416 robots: 2 101 248 float4 columns for a grid capped at 8192 x 256 threads, so 4096 threads go round the
    loop twice -- they own column 0 of robots 16 384 .. 16 415 on their second pass -- and the outcome kernel runs 65
    workgroups.  No oracle at this size: the model is fed from the env's own fields (other tests pin those to the oracle),
    cloned on the device each tick, and compared there."""
    import dataclasses
    from util import S
    T, lead = 2, 3          # (episodes of two ticks behind three ticks: the last world has robots of both kinds at both ticks)
    sc = dataclasses.replace(S.stage1(num_worlds=513, robots_per_world=32, seed=1), timeout=1)
    env = hip.VecStageWorld(sc)
    env.reset()
    N, F = env.N, env.F
    assert N * (env.B // 4) > 8192 * 256
    rng = np.random.default_rng(7)
    lo, hi = _bounds()
    for _ in range(lead):
        env.step(_dev(R.clip_action(R.policy_outputs(rng, N)[0])))
    buf, tick = _new_buffer(env, T)
    _poison(buf)
    buf.begin_horizon(env.obs)
    want, fresh = [], []
    for t in range(T):
        a, lp, v = (_dev(x) for x in R.policy_outputs(rng, N))
        row = {"obs": env.obs.clone(), "goal": env.local_goal.clone(), "speed": env.speed.clone(), "action": a,
               "logprob": lp.view(N, 1), "value": v}
        fresh.append(env.fresh.clone())
        _store_tick(env, buf, tick, a, lp, v, lo, hi)
        row["reward"], row["done"] = env.reward.clone(), env.done.clone()
        want.append(row)
        assert int(tick) == t + 1 and int(buf._ticket) == 0, t
    stacks = buf.obs_rows().materialise()

    def same(x, y):
        return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32 if x.dtype == torch.float32 else x.dtype),
                                                                           y.contiguous().view(torch.int32 if y.dtype == torch.float32 else y.dtype))
    for t in range(T):
        assert same(stacks[t], want[t]["obs"]), ("obs", t)
        assert same(buf.frames[t + F - 1], want[t]["obs"][:, F - 1]), ("frames", t)
        for k in FIELDS:
            assert same(getattr(buf, k)[t], want[t][k]), (k, t)
    # the cases: robots of the loop's second pass among those that restarted and among those that did not, at both ticks
    tail = slice(8192 * 256 // (env.B // 4), N)
    for t in range(T):
        f = fresh[t][tail].bool()
        assert bool(f.any()) and bool((~f).any()), t
    env.check()
    env.close()


# ---------------------------------------------------------------------------------------------- (d)
def test_trainer_run_on_stage2_fills_the_buffer_as_the_reference_does(hip):
    """``Stage1Trainer(stage2=True).run(15)`` with captured ticks and the library's stores: one eight-tick replay and seven of one
    tick, no update.  The oracle is replayed with the stored actions, clipped; every stored tensor the policy did not make
    equals the model, the HIP GAE of the stored rows equals the oracle's fp32 GAE, the filter index equals the reference's walk
    and the rows handed out after filtering equal the model's, eager and lazy."""
    from mrca import ppo
    from mrca.trainer import HParams, Stage1Trainer
    ticks = 15
    sc, lead = R.scenario("stage2", 16)
    env, ora = hip.VecStageWorld(sc), U.COracleEnv(sc)
    hp = HParams(horizon=16, graph_tick=True, rollout_fused=True)
    tr = Stage1Trainer(env, hp=hp, seed=3, stage2=True)
    assert tr.buffer.env_bound
    tr.start()
    tr._capture()                                   # (its warm-up ticks advance the env: the oracle starts from what they left)
    assert lead == 3 and tr._graph_run is not None
    env.invalidate_views()
    _copy_state(env, ora)
    buf = tr.buffer
    _poison(buf)
    tr.run(ticks)
    torch.cuda.synchronize()
    assert tr.global_update == 0 and int(tr._t_idx) == ticks and int(buf._ticket) == 0
    N, F, B = env.N, env.F, env.B
    action, logprob, value = (getattr(buf, k)[:ticks].cpu().numpy() for k in ("action", "logprob", "value"))
    assert np.isfinite(action).all() and np.isfinite(logprob).all() and np.isfinite(value).all()
    model, log = R.RefRollout(), {"fresh": [], "done": [], "obs": []}
    for t in range(ticks):
        _oracle_tick(ora, model, log, action[t], logprob[t], value[t])
    want = model.arrays()
    R.assert_same(want, _host(buf, ticks), "trainer")
    U.assert_state_equal(U.HostView(env), ora, what="trainer: the env after the run")
    _coverage(sc, ticks, log)
    # GAE of the stored rows: the HIP kernel against the oracle's restatement in fp32, the last value as the policy gives it
    with torch.no_grad():
        obs, head = ppo.policy_input(env, True)
        _m, last_v = tr.policy.mean_value_fused(obs, env.local_goal, env.speed, head=head, bf16=False)
    last_v = last_v.reshape(-1).contiguous()
    tg, adv = hip.gae(buf.reward[:ticks].contiguous(), buf.value[:ticks].contiguous(), last_v, buf.done[:ticks].contiguous(),
                      hp.gamma, hp.lam)
    t32, a32 = O.gae(want["reward"], want["value"], last_v.cpu().numpy(), want["done"], hp.gamma, hp.lam, np.float32)
    assert R.same_bits(tg.cpu().numpy(), t32) and R.same_bits(adv.cpu().numpy(), a32)
    # the rows the Stage-2 update drops and the rows it is handed
    drop = R.filter_index(want["done"])
    assert len(drop) > 0 and ppo.get_filter_index(buf.done[:ticks]).tolist() == drop
    keep = torch.ones(hp.horizon * N, dtype=torch.bool, device="cuda")
    keep[ticks * N:] = False                                            # (the row the run did not reach)
    keep[torch.tensor(drop, dtype=torch.long, device="cuda")] = False
    left = np.delete(want["obs"].reshape(ticks * N, F, B), drop, axis=0)
    index = torch.from_numpy(np.random.default_rng(5).permutation(len(left))).cuda()
    assert len(left) == int(keep.sum())
    lazy = ppo.FrameRows(buf.frames, buf.fidx, lazy=True)
    for got in (buf.obs_rows()[keep][index], lazy[keep][index].gather()):
        assert R.same_bits(got.cpu().numpy(), left[index.cpu().numpy()])
    env.check()
    env.close()
