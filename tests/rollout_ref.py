"""The reference's rollout buffer as plain NumPy (tests only): the model the library's stores (csrc/mrca_rollout_store.hip)
and their torch twin (mrca/ppo.py RolloutBuffer) are held to.

The reference keeps a Python list.  Every step it appends what the policy saw and said -- the whole observation stack, the
local goal, the speed, the action, its log-probability, the value -- together with what the env answered (reward, terminal),
and before an update it stacks the list into arrays, one leading axis per step (ppo_stage1.py:59-60, 87-103;
model/ppo.py:22-54 transform_buffer).  That is all this file does: it takes host copies of whole ``[N, F, B]`` stacks and
knows nothing of one-frame stores, frame rows, row indices or ring heads.  Every array keeps the dtype it is given in
(float32 / uint8) and is never recomputed, so a comparison on bits is meaningful (``bits``)."""
import numpy as np


def bits(x):
    """An array's bit patterns (float32 -> uint32: -0.0 != +0.0, a NaN equals itself payload and all); integers pass."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


class RefRollout:
    """One horizon of the reference's ``buff``: ``append`` before the env steps, ``outcome`` after, ``arrays`` at the end."""

    def __init__(self):
        self.buff = []
        self._open = None

    def append(self, obs, goal, speed, action, logprob, value):
        """What the policy saw (the env's stacks, local goals and speeds, as they stand before the step) and what it said."""
        assert self._open is None, "append twice without an outcome in between"
        n = np.asarray(goal).shape[0]
        self._open = (np.array(obs, np.float32), np.array(goal, np.float32), np.array(speed, np.float32),
                      np.array(action, np.float32), np.array(logprob, np.float32).reshape(n, 1),
                      np.array(value, np.float32).reshape(n))

    def outcome(self, reward, done):
        """What the env answered: one list entry is complete."""
        assert self._open is not None, "outcome without an append"
        self.buff.append(self._open + (np.array(reward, np.float32), np.array(done, np.uint8)))
        self._open = None

    def __len__(self):
        return len(self.buff)

    def arrays(self):
        """-> dict of [T, N, ...] arrays (sample t * N + i is robot i at step t), the list stacked step by step."""
        assert self._open is None and self.buff
        names = ("obs", "goal", "speed", "action", "logprob", "value", "reward", "done")
        return {k: np.stack([e[j] for e in self.buff]) for j, k in enumerate(names)}


def filter_index(dones):
    """The samples a Stage-2 update drops (model/utils.py:65-78): walking robot by robot and, inside a robot, step by step,
    a sample goes once the terminal flag has been set for two samples of the walk in a row.  The run length is NOT cleared
    where the walk passes from one robot to the next: a robot whose last step is terminal hands its run to the next robot's
    first step.  dones: [T, N] -> list of t * N + i, in walk order."""
    T, N = dones.shape
    out, run = [], 0
    for i in range(N):
        for t in range(T):
            run = run + 1 if dones[t, i] else 0
            if run >= 2:
                out.append(t * N + i)
    return out


# ------------------------------------------------------------------------------------------------
# What the tests that hold a buffer to the model share (tests/test_rollout_ref_host.py on the CPU, tests/test_gpu_rollout_store.py
# on the device): the scenarios, what stands in for the policy, and the conditions the C oracle's own fields must meet for a
# run to have reached the cases it is there for.

ACTION_BOUND = ((0.0, -1.0), (1.0, 1.0))          # ppo_stage1.py:170

# (scenario, horizon) -> (timeout, ticks stepped before the first horizon).  Episodes of a few ticks, so that restarts fall
# inside horizons of 1, 2 and 12 ticks; Stage-2's groups all time out together and restart in lock-step, so the ticks before
# the first horizon choose where in a horizon that happens.  Found by running the oracle alone; `coverage` asserts them.
CASES = {
    ("stage1", 1): (2, 2), ("stage1", 2): (2, 2), ("stage1", 12): (2, 2),
    ("stage2", 1): (3, 3), ("stage2", 2): (2, 2), ("stage2", 12): (4, 3),
    ("stage2_hold", 1): (3, 3), ("stage2_hold", 2): (2, 2), ("stage2_hold", 12): (4, 3),
    ("stage2", 16): (5, 3),         # the trainer's run of 15 ticks behind the three warm-up ticks of its capture
}


def scenario(name, horizon, seed=1):
    """-> (Scenario, ticks before the first horizon): Stage-1 at 7 x 37 = 259 robots, Stage-2 at 6 x 44 = 264 (two workgroups
    of the outcome kernel, the second nearly empty), with the case's short timeout."""
    import dataclasses
    from mrca import scenario as S
    timeout, lead = CASES[(name, horizon)]
    sc = {"stage1": lambda: S.stage1(num_worlds=7, robots_per_world=37, seed=seed),
          "stage2": lambda: S.stage2(num_worlds=6, seed=seed),
          "stage2_hold": lambda: S.stage2(num_worlds=6, seed=seed, hold_velocity=True)}[name]()
    return dataclasses.replace(sc, timeout=timeout), lead


def clip_action(a):
    """The command the robot gets: the stored action clipped to the bounds (model/ppo.py:79)."""
    lo, hi = (np.asarray(b, np.float32) for b in ACTION_BOUND)
    return np.minimum(np.maximum(np.asarray(a, np.float32), lo), hi)


_ODD_BITS = np.array([0x80000000,      # -0.0
                      0x7F800000,      # +inf
                      0xFF800000,      # -inf
                      0x7FC12345,      # a quiet NaN with a payload
                      0xFFA00001,      # a negative NaN with another
                      0x00000001,      # the smallest denormal
                      0x807FFFFF],     # the largest negative denormal
                     np.uint32).view(np.float32)


def policy_outputs(rng, n):
    """What stands in for the policy at one tick: a finite unclipped action f32[n,2] and a log-probability / value f32[n]
    each, drawn from ``rng``; log-probability and value also carry bit patterns a store must not touch, at robots spread
    over the whole range (the last robot among them)."""
    a = rng.standard_normal((n, 2)).astype(np.float32)
    a[:, 0] += np.float32(0.5)
    lp = rng.standard_normal(n).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    for x in (lp, v):
        at = rng.choice(n - 1, size=len(_ODD_BITS) - 1, replace=False)
        x[at] = _ODD_BITS[:-1]
        x[n - 1] = _ODD_BITS[rng.integers(len(_ODD_BITS))]
    return a, lp, v


def longest_run(flags):
    """[K, N] flags -> the longest run of consecutive set rows any column has."""
    run = np.zeros(flags.shape[1], np.int64)
    best = 0
    for row in flags:
        run = np.where(row != 0, run + 1, 0)
        best = max(best, int(run.max()))
    return best


def coverage(sc, T, fresh, done, obs):
    """Assert, from the C oracle's own fields, that a run of H horizons of T ticks reached the cases it is there for.
    ``fresh`` u8[H*T, N]: the oracle's restart flag as the state store of a tick sees it (before the step); ``done`` u8[H*T, N]:
    its terminal flag after the step; ``obs`` f32[H*T, N, F, B]: its stacks before the step."""
    K, N = fresh.shape
    H, F = K // T, obs.shape[2]
    fr = fresh.reshape(H, T, N) != 0
    if T >= 2:
        assert fr[:, 1:].any(), "no robot restarted at a tick 1 .. T-1 of a horizon"
    if H > 1:           # (a single horizon: the trainer's run, whose first tick already follows other ticks)
        assert fr[1:, 0].any(), "no robot was fresh at tick 0 of a horizon other than the first"
    assert (~fr[:, 0]).any(), "no robot carried older frames into tick 0 of a horizon"
    # a robot that did not restart dropped its oldest frame and appended one (every such robot and tick: this is the rule the
    # one-frame stores lean on, asserted of the oracle)
    carried = 0
    for k in range(1, K):
        keep = fresh[k] == 0
        carried += int(keep.sum())
        assert same_bits(obs[k][keep][:, : F - 1], obs[k - 1][keep][:, 1:]), k
        gone = ~keep
        assert all(same_bits(obs[k][gone][:, f], obs[k][gone][:, F - 1]) for f in range(F - 1)), k
    assert carried > 0, "every robot restarted at every tick"
    if sc.auto_reset != 2:          # (scenario.AUTO_GROUP)
        return
    # ---- Stage-2
    R, gid = sc.robots_per_world, np.asarray(sc.group_id)
    whole = False
    for k in range(1, K):
        for w in range(sc.num_worlds):
            for g in range(int(gid.max()) + 1):
                whole |= bool(fresh[k][w * R: (w + 1) * R][gid == g].all())
    assert whole, "no whole group restarted in one tick"
    assert longest_run(done) >= 3, "no robot waited for its group with done set for three ticks in a row"
    dn = done.reshape(H, T, N)
    if T >= 3:
        assert max(longest_run(dn[h]) for h in range(H)) >= 3
    assert any(len(filter_index(dn[h])) for h in range(H)), "the filter index is empty in every horizon"
    # the quirk: a robot whose last tick is done hands its run to the next robot's first tick -- which is dropped for that
    # reason alone when it starts that robot's walk (T == 1: every done robot behind a done robot)
    quirk = dn[:, T - 1, :-1] & dn[:, 0, 1:]
    assert quirk.any(), "the filter's cross-robot case did not occur"


def assert_same(want, got, what=""):
    """Every array of ``want`` (the model's) against the one of the same name in ``got``, on bits."""
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} is {g.dtype}{g.shape}, the model's {w.dtype}{w.shape}"
        bad = np.argwhere(bits(g) != bits(w))
        if len(bad):
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {w.size} entries; first {i}: {g[i]!r} vs the model's {w[i]!r}")
