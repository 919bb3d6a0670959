"""Host: the reference's rollout buffer (tests/rollout_ref.py: a list of whole stacks, stacked) against the torch rollout
buffer of mrca/ppo.py -- one frame per tick + row indices, and whole stacks -- both fed from the C oracle, on bits.

This is where the frame-row rule of the one-frame buffer (``fidx``, ``cur``, tick 0 of a horizon, F copies of the fresh scan
after a restart) meets what the reference does; tests/test_gpu_rollout_store.py holds the library's two kernels to the same
model.  Episodes last a few ticks (rollout_ref.CASES), and every test asserts from the oracle's own ``fresh`` / ``done`` that
restarts fell where they matter (rollout_ref.coverage): with the scenarios' own timeouts these assertions fail."""
import numpy as np
import pytest
import torch

import rollout_ref as R
import util as U

HORIZONS = 3
FIELDS = ("goal", "speed", "action", "logprob", "value", "reward", "done")


def _host(buf):
    out = {k: getattr(buf, k).numpy() for k in FIELDS}
    out["obs"] = (buf.obs_rows().materialise() if buf.single_frame else buf.obs).numpy()
    return out


def drive(name, T, case=None):
    """HORIZONS horizons of T ticks on one oracle env; after each, both buffers against the model.  -> what coverage() takes."""
    from mrca import ppo
    if case is not None:
        R.CASES[(name, T)] = case
    sc, lead = R.scenario(name, T)
    ora = U.COracleEnv(sc)
    ora.reset()
    rng = np.random.default_rng(7)
    N, F, B = sc.num_robots, sc.frames, sc.beams
    for _ in range(lead):
        ora.step(R.clip_action(R.policy_outputs(rng, N)[0]))
    cpu = torch.device("cpu")
    one = ppo.RolloutBuffer(T, N, F, B, cpu, single_frame=True)
    full = ppo.RolloutBuffer(T, N, F, B, cpu, single_frame=False)
    env = {k: torch.from_numpy(getattr(ora, k)) for k in ("obs", "local_goal", "speed", "reward", "done", "fresh")}
    fresh, done, obs = [], [], []
    for h in range(HORIZONS):
        model, newest = R.RefRollout(), []
        for buf in (one, full):
            buf.begin_horizon(env["obs"])
        for t in range(T):
            a, lp, v = R.policy_outputs(rng, N)
            model.append(ora.obs, ora.local_goal, ora.speed, a, lp, v)
            t_idx = torch.tensor([t])
            for buf in (one, full):
                buf.store_state_at(t_idx, env["obs"], env["local_goal"], env["speed"], torch.from_numpy(a), torch.from_numpy(lp),
                                   torch.from_numpy(v), env["fresh"])
            fresh.append(ora.fresh.copy())
            obs.append(ora.obs.copy())
            newest.append(ora.obs[:, F - 1].copy())
            ora.step(R.clip_action(a))
            model.outcome(ora.reward, ora.done)
            for buf in (one, full):
                assert buf.store_outcome_at(t_idx, env["reward"], env["done"]) is False
            done.append(ora.done.copy())
        want = model.arrays()
        R.assert_same(want, _host(one), f"{name} T={T} horizon {h}, one frame per tick")
        R.assert_same(want, _host(full), f"{name} T={T} horizon {h}, whole stacks")
        for t in range(T):
            assert R.same_bits(one.frames[t + F - 1].numpy(), newest[t]), (h, t)
        # the rows a Stage-2 update drops, and the rows it is then handed
        drop = R.filter_index(want["done"])
        assert ppo.get_filter_index(one.done).tolist() == drop, f"{name} T={T} horizon {h}: filter index"
        keep = torch.ones(T * N, dtype=torch.bool)
        keep[torch.tensor(drop, dtype=torch.long)] = False
        left = np.delete(want["obs"].reshape(T * N, F, B), drop, axis=0)
        index = torch.from_numpy(rng.permutation(len(left)))
        assert len(left) == int(keep.sum()) > 0
        rows = one.obs_rows()
        lazy = ppo.FrameRows(one.frames, one.fidx, lazy=True)
        for got in (rows[keep][index], lazy[keep][index].gather(), full.obs_rows()[keep][index]):
            assert R.same_bits(got.numpy(), left[index.numpy()]), f"{name} T={T} horizon {h}: kept rows"
    return sc, np.array(fresh), np.array(done), np.array(obs)


@pytest.mark.parametrize("T", [1, 2, 12])
@pytest.mark.parametrize("name", ["stage1", "stage2", "stage2_hold"])
def test_both_torch_buffers_equal_the_reference_buffer_on_the_oracle(name, T):
    """Every row of three horizons in a row on one env: stacks, goal, speed, action, logprob, value, reward, done, the newest
    frame's row, the filter index and the rows left after filtering (eager and through a FrameTable) -- all equal to the list
    the reference would have kept.  T = 1 and 2 are shorter than the stack: the older frames of a horizon's first tick are then
    carried over from the horizon before."""
    sc, fresh, done, obs = drive(name, T)
    R.coverage(sc, T, fresh, done, obs)


def test_the_models_filter_walk():
    """The model's filter index on a case small enough to do by hand: robot-major, two in a row, the run carried from one
    robot's last step into the next robot's first."""
    d = np.array([[0, 1, 1, 0],
                  [1, 1, 0, 0],
                  [1, 0, 1, 1]], np.uint8)             # [T=3, N=4]
    # robot 0: 0 1 1 -> t=2;  robot 1 (run 2 carried in): 1 1 0 -> t=0, t=1;  robot 2: 1 0 1 -> none;  robot 3 (run 1): 0 0 1 -> none
    assert R.filter_index(d) == [2 * 4 + 0, 0 * 4 + 1, 1 * 4 + 1]
    from mrca import ppo
    assert ppo.get_filter_index(torch.from_numpy(d)).tolist() == R.filter_index(d)
