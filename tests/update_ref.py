"""One PPO update of the reference as plain float64 on the CPU (tests only): the model the update of mrca/ppo.py -- as the
trainer runs it, and through the HIP kernels -- is held to.

Written from the reference's formulas, with neither ``mrca.ppo`` nor ``mrca.net``: the two towers as ``F.conv1d`` /
``F.linear`` (model/net.py:19-70), the log density (model/utils.py:90-97), the entropy (model/net.py:78-79), the
population-std normalisation of the advantages over ALL rows (model/ppo.py:148, 202) *before* the Stage-2 rows are deleted
(model/ppo.py:212-218), the clipped surrogate, ``20 * mse`` and the entropy bonus (model/ppo.py:172-185), and Adam as
``torch.optim.Adam(lr)`` defines it (ppo_stage1.py:176: betas 0.9 / 0.999, eps 1e-8), by hand.  The model draws nothing: the
minibatches are handed to it as index lists, per epoch, into the rows left after filtering.

The two options the trainer adds to the reference's update are restated as well: ``max_grad_norm`` (the gradient times
``min(1, c / (norm + 1e-6))``) and ``logstd_min`` (the log standard deviation clamped from below after every step).

tests/test_update_ref_host.py grounds the model in the reference's own run (tests/golden/ppo_update.npz); the helpers at the
end are what that file and tests/test_gpu_update_path.py share."""
import contextlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# the parameters in the order the reference declares them (model/net.py:19-33) = ``parameters()`` order = the order of a flat
# gradient bucket
ORDER = ("logstd",
         "act_fea_cv1.weight", "act_fea_cv1.bias", "act_fea_cv2.weight", "act_fea_cv2.bias", "act_fc1.weight", "act_fc1.bias",
         "act_fc2.weight", "act_fc2.bias", "actor1.weight", "actor1.bias", "actor2.weight", "actor2.bias",
         "crt_fea_cv1.weight", "crt_fea_cv1.bias", "crt_fea_cv2.weight", "crt_fea_cv2.bias", "crt_fc1.weight", "crt_fc1.bias",
         "crt_fc2.weight", "crt_fc2.bias", "critic.weight", "critic.bias")

_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

Update = namedtuple("Update", "states grads losses grad_norms advs")


def _f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().clone()
    return torch.from_numpy(np.array(x, dtype=np.float64))


def _tower(p, tw, x, goal, speed):
    """model/net.py:42-48 (actor) and 61-66 (critic)"""
    h = F.relu(F.conv1d(x, p[tw + "_fea_cv1.weight"], p[tw + "_fea_cv1.bias"], stride=2, padding=1))
    h = F.relu(F.conv1d(h, p[tw + "_fea_cv2.weight"], p[tw + "_fea_cv2.bias"], stride=2, padding=1))
    h = h.reshape(h.shape[0], -1)
    h = F.relu(F.linear(h, p[tw + "_fc1.weight"], p[tw + "_fc1.bias"]))
    h = torch.cat((h, goal, speed), dim=-1)
    return F.relu(F.linear(h, p[tw + "_fc2.weight"], p[tw + "_fc2.bias"]))


def forward(p, x, goal, speed):
    """-> (mean [n,2], value [n,1])   model/net.py:49-51, 67"""
    a = _tower(p, "act", x, goal, speed)
    mean = torch.cat((torch.sigmoid(F.linear(a, p["actor1.weight"], p["actor1.bias"])),
                      torch.tanh(F.linear(a, p["actor2.weight"], p["actor2.bias"]))), dim=-1)
    c = _tower(p, "crt", x, goal, speed)
    return mean, F.linear(c, p["critic.weight"], p["critic.bias"])


def log_density(action, mean, logstd):
    """model/utils.py:90-97, summed over the action's components, keepdim"""
    var = torch.exp(logstd) ** 2
    return (-(action - mean) ** 2 / (2.0 * var) - _HALF_LOG_2PI - logstd).sum(dim=1, keepdim=True)


def policy_logprob(sd, obs, goal, speed, action):
    """The log-probability the policy ``sd`` gives ``action`` at every row, float64 [n, 1] (numpy)."""
    p = {k: _f64(sd[k]) for k in ORDER}
    with torch.no_grad():
        mean, _v = forward(p, _f64(obs), _f64(goal), _f64(speed))
        return log_density(_f64(action), mean, p["logstd"].expand_as(mean)).numpy()


def update(sd, mem, drop, batches, lr=5e-5, clip=0.1, value_coef=20.0, entropy_coef=5e-4, max_grad_norm=0.0, logstd_min=None,
           betas=(0.9, 0.999), eps=1e-8, every_state=True):
    """One PPO update.

    ``sd``: the state dict before.  ``mem``: dict of arrays ``obs [T,N,3,512]`` (materialised stacks), ``goal [T,N,2]``,
    ``speed [T,N,2]``, ``action [T,N,2]``, ``logprob [T,N,1]``, ``target [T,N]`` or ``[T,N,1]``, ``adv`` likewise (raw: the
    model normalises them).  ``drop``: the Stage-2 drop list (rows t * N + i) or None.  ``batches``: per epoch the list of
    minibatch index arrays into the rows left after the drop.

    -> Update: ``states`` the state dict (float64 numpy arrays) after every optimiser step (with ``every_state=False`` only
    after the first and after the last: ``states[0]``, ``states[-1]``; empty for an update of no steps), ``grads`` the gradient Adam was handed at every step as one
    flat vector in ``ORDER`` (after the clip, if any), ``losses`` [steps, 3] (policy loss, value loss, entropy: what the
    reference logs, model/ppo.py:189-192), ``grad_norms`` the gradient's norm before the clip, ``advs`` the normalised
    advantages of the rows left."""
    p = {k: _f64(sd[k]).requires_grad_(True) for k in ORDER}
    n = int(np.prod(np.shape(mem["goal"])[:2]))
    flat = {k: _f64(mem[k]).reshape((n,) + s) for k, s in (("obs", tuple(np.shape(mem["obs"])[2:])), ("goal", (2,)), ("speed", (2,)),
                                                          ("action", (2,)), ("logprob", (1,)), ("target", (1,)), ("adv", (1,)))}
    adv = flat["adv"]
    flat["adv"] = (adv - adv.mean()) / adv.std(unbiased=False)              # model/ppo.py:148: np.std, over ALL rows
    if drop is not None and len(drop):                                      # model/ppo.py:212-218: np.delete
        keep = np.ones(n, bool)
        keep[np.asarray(drop, np.int64)] = False
        flat = {k: v[torch.from_numpy(keep)] for k, v in flat.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    states, grads, losses, norms, t = [], [], [], [], 0
    for epoch_batches in batches:
        for index in epoch_batches:
            ix = torch.as_tensor(np.asarray(index, np.int64))
            mb = {k: v[ix] for k, v in flat.items()}
            mean, value = forward(p, mb["obs"], mb["goal"], mb["speed"])                     # model/ppo.py:172
            logstd = p["logstd"].expand_as(mean)
            entropy = (0.5 + _HALF_LOG_2PI + logstd).sum(-1).mean()                          # model/net.py:78-79
            ratio = torch.exp(log_density(mb["action"], mean, logstd) - mb["logprob"])      # model/ppo.py:175
            s1 = ratio * mb["adv"]
            s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * mb["adv"]
            policy_loss = -torch.min(s1, s2).mean()                                          # model/ppo.py:180
            value_loss = ((value - mb["target"]) ** 2).mean()                                # model/ppo.py:183
            loss = policy_loss + value_coef * value_loss - entropy_coef * entropy            # model/ppo.py:185
            g = dict(zip(ORDER, torch.autograd.grad(loss, [p[k] for k in ORDER])))
            norm = float(torch.sqrt(sum((x ** 2).sum() for x in g.values())))
            if max_grad_norm > 0:
                scale = min(1.0, max_grad_norm / (norm + 1e-6))
                g = {k: x * scale for k, x in g.items()}
            t += 1
            with torch.no_grad():                                                            # torch.optim.Adam's step
                for k in ORDER:
                    m[k] = betas[0] * m[k] + (1.0 - betas[0]) * g[k]
                    v2[k] = betas[1] * v2[k] + (1.0 - betas[1]) * g[k] * g[k]
                    denom = torch.sqrt(v2[k]) / np.sqrt(1.0 - betas[1] ** t) + eps
                    p[k] -= (lr / (1.0 - betas[0] ** t)) * m[k] / denom
                if logstd_min is not None:
                    p["logstd"].clamp_(min=logstd_min)
            grads.append(torch.cat([g[k].reshape(-1) for k in ORDER]).numpy())
            norms.append(norm)
            losses.append((float(policy_loss.detach()), float(value_loss.detach()), float(entropy.detach())))
            if every_state or t == 1:
                states.append({k: p[k].detach().numpy().copy() for k in ORDER})
    if not every_state and t > 1:
        states.append({k: p[k].detach().numpy().copy() for k in ORDER})
    return Update(states, grads, np.array(losses, np.float64).reshape(-1, 3), norms, flat["adv"].numpy())


# ------------------------------------------------------------------------------------------------
# What the tests that hold an update to the model share.

@contextlib.contextmanager
def recorded_randperm():
    """Inside: ``torch.randperm`` is the real one, and every permutation it returns is appended (as a host int64 array) to
    the list this yields.  Outside: ``torch.randperm`` is what it was."""
    real, out = torch.randperm, []

    def randperm(*args, **kw):
        perm = real(*args, **kw)
        out.append(perm.detach().cpu().numpy().astype(np.int64))
        return perm
    torch.randperm = randperm
    try:
        yield out
    finally:
        torch.randperm = real


def cut(perm, batch, drop_last):
    """A permutation -> its minibatches, in order (torch's BatchSampler, model/ppo.py:159, 222): ``batch`` entries each, the
    short last one kept unless ``drop_last``."""
    perm = np.asarray(perm)
    out = [perm[lo: lo + batch] for lo in range(0, len(perm), batch)]
    if drop_last and out and len(out[-1]) < batch:
        out.pop()
    return out


def state_of(policy):
    """A module's state dict as float64 numpy arrays (copies)."""
    return {k: v.detach().cpu().double().numpy().copy() for k, v in policy.state_dict().items()}


def distance(before, got, want):
    """D: the largest, over the parameter tensors, of ||d_got - d_want|| / ||d_want|| with d = after - before.
    -> (D, {tensor: its ratio})"""
    per = {}
    for k in ORDER:
        b = np.asarray(before[k], np.float64)
        dg, dw = np.asarray(got[k], np.float64) - b, np.asarray(want[k], np.float64) - b
        per[k] = float(np.linalg.norm(dg - dw) / np.linalg.norm(dw))
    return max(per.values()), per


def loss_distance(log, losses):
    """L: the largest |logged loss - model| / max(1, |model|) over the steps and the three logged figures."""
    got = np.array([[float(x) for x in row] for row in log], np.float64).reshape(-1, 3)
    assert got.shape == losses.shape, (got.shape, losses.shape)
    return float((np.abs(got - losses) / np.maximum(1.0, np.abs(losses))).max()) if got.size else 0.0


def frame_store(T, N, rng, restarts=((2, 5),)):
    """A one-frame-per-tick store as ppo.RolloutBuffer keeps it: ``frames`` f32[T+2, N, 512] and, per tick and robot, the rows
    of its stack ``fidx`` i64[T, N, 3] -- rows t, t+1, t+2, and for a robot that restarted at tick t (``restarts``: (t, i))
    three times its fresh scan, the stacks of the ticks behind filling up from it (ppo_stage1.py:59-60)."""
    frames = (rng.random((T + 2, N, 512)) - 0.5).astype(np.float32)
    fidx = np.empty((T, N, 3), np.int64)
    for t in range(T):
        fidx[t] = np.arange(t, t + 3)[None, :]
    for t0, i in restarts:
        cur = np.array([t0 + 2] * 3)
        for t in range(t0, T):
            if t > t0:
                cur = np.array([cur[1], cur[2], t + 2])
            fidx[t, i] = cur
    return frames, fidx


def stacks(frames, fidx):
    """The store's stacks written out, f32[T, N, 3, 512]: frame f of robot i's stack at tick t is row fidx[t, i, f] of robot i."""
    T, N, Fr = fidx.shape
    return frames[fidx, np.arange(N)[None, :, None]]


def done_flags(T, N, rng, empty=False, single_carry=None):
    """Synthetic terminal flags u8[T, N] with runs of ones -- inside a robot, and handed from one robot's last tick to the next
    robot's first (the cross-robot carry of model/utils.py:65-78).  ``empty``: isolated ones only, nothing to drop.
    ``single_carry=i``: robot i's last tick and robot i + 1's first and nothing else: one row dropped, by the carry alone."""
    d = np.zeros((T, N), np.uint8)
    if single_carry is not None:
        d[T - 1, single_carry] = d[0, single_carry + 1] = 1
        return d
    if empty:
        d[1, ::3] = 1
        return d
    d[rng.integers(0, T, N // 2), rng.integers(0, N, N // 2)] = 1            # isolated ones (some may touch)
    d[1:4, 1] = 1                                                           # a run of three inside a robot
    d[T - 2:, 2] = 1                                                        # a run that ends a robot's walk ...
    d[0, 3] = 1                                                             # ... and carries into the next robot's first tick
    d[T - 1, N - 2] = d[0, N - 1] = 1                                       # the carry alone
    return d


def synthetic_memory(sd, T, N, seed, clip=0.1):
    """-> (mem, frames, fidx): a memory for ``update`` over a frame store with a restarted robot; the old log-probabilities sit
    around the ones the policy ``sd`` itself gives the actions -- exactly on them for every fifth row, otherwise a normal
    0.15 away, so that with ``clip`` = 0.1 the first minibatches have ratios inside the clip range, below it and above it
    (the construction of tests/test_gpu_ppo_loss.py; ``ratio_classes`` counts them)."""
    rng = np.random.default_rng(seed)
    frames, fidx = frame_store(T, N, rng, restarts=((2, min(5, N - 1)), (0, 0)))
    obs = stacks(frames, fidx)
    goal = rng.standard_normal((T, N, 2)).astype(np.float32) * 3
    speed = rng.random((T, N, 2)).astype(np.float32)
    action = (rng.random((T, N, 2)) * np.array([1.0, 2.0]) - np.array([0.0, 1.0])).astype(np.float32)
    action += (rng.standard_normal((T, N, 2)) * 0.5).astype(np.float32)
    lp = policy_logprob(sd, obs.reshape(T * N, 3, 512), goal.reshape(-1, 2), speed.reshape(-1, 2), action.reshape(-1, 2))
    shift = rng.standard_normal((T * N, 1)) * 0.15
    shift[::5] = 0.0
    mem = {"obs": obs, "goal": goal, "speed": speed, "action": action,
           "logprob": (lp - shift).astype(np.float32).reshape(T, N, 1),
           "target": rng.standard_normal((T, N, 1)).astype(np.float32),
           "adv": (rng.standard_normal((T, N, 1)) * 2 + 0.3).astype(np.float32)}
    return mem, frames, fidx


def ratio_classes(sd, mem, clip):
    """-> (inside, below, above): how many rows' ratio new / old density, at the policy ``sd``, lies within [1 - clip, 1 + clip],
    below it and above it."""
    n = int(np.prod(mem["goal"].shape[:2]))
    lp = policy_logprob(sd, mem["obs"].reshape((n,) + mem["obs"].shape[2:]), mem["goal"].reshape(n, 2), mem["speed"].reshape(n, 2),
                        mem["action"].reshape(n, 2))
    ratio = np.exp(lp - mem["logprob"].reshape(n, 1).astype(np.float64))
    return int(((ratio >= 1 - clip) & (ratio <= 1 + clip)).sum()), int((ratio < 1 - clip).sum()), int((ratio > 1 + clip).sum())


def torch_memory(mem, device, rows=None):
    """``mem`` as the tuple ``ppo.ppo_update_stage{1,2}`` take (obss, goals, speeds, actions, logprobs, targets, values,
    rewards, advs); ``rows``: what stands for the stacks (a ppo.FrameRows) instead of the materialised tensor."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)        # noqa: E731
    obss = rows if rows is not None else dev(mem["obs"])
    return (obss, dev(mem["goal"]), dev(mem["speed"]), dev(mem["action"]), dev(mem["logprob"]), dev(mem["target"]), None, None,
            dev(mem["adv"]))


HP = dict(lr=5e-5, clip=0.1, value_coef=20.0, entropy_coef=5e-4)          # ppo_stage1.py:22-35, model/ppo.py:185


def run_update(ppo, policy, optimizer, flat_grads, memory, T, N, batch, stage2, drop=None, epoch=2, index_batches=None,
               hp=HP, **opts):
    """One update through ``ppo.ppo_update_stage{1,2}`` (``ppo``: the module under test, handed in).  ``index_batches=None``: the
    production path, which draws its own permutations.  -> (loss log, the permutations ``torch.randperm`` returned meanwhile)."""
    log = []
    kw = dict(policy=policy, optimizer=optimizer, batch_size=batch, memory=memory, epoch=epoch, coeff_entropy=hp["entropy_coef"],
              clip_value=hp["clip"], num_step=T, num_env=N, frames=3, obs_size=512, act_size=2, value_coef=hp["value_coef"],
              index_batches=index_batches, flat_grads=flat_grads, log=log, **opts)
    with recorded_randperm() as perms:
        if stage2:
            ppo.ppo_update_stage2(filter_index=drop, **kw)
        else:
            ppo.ppo_update_stage1(**kw)
    return log, perms


def replay_batches(perms, batch, drop_last, device):
    """Recorded permutations -> an ``index_batches`` callable that hands them back, one epoch per call, cut the way the
    production path cuts them."""
    it = iter(perms)
    return lambda n: [torch.as_tensor(b, device=device) for b in cut(next(it), batch, drop_last)]


def snapshot_updates(monkeypatch, ppo):
    """Wrap ``ppo.ppo_update_stage1`` / ``_stage2`` for one test: what the trainer hands them -- the memory tuple (host copies,
    the stacks written out from the frame store), the filter index, the state dict at that moment -- and the permutations
    drawn meanwhile are appended to the list this returns; then the update runs."""
    seen = []

    def wrap(real, stage2):
        def update(*args, **kw):
            assert not args
            obss, goals, speeds, actions, logprobs, targets, _values, _rewards, advs = kw["memory"]
            host = lambda x: x.detach().cpu().numpy().copy()        # noqa: E731
            obs = stacks(host(obss.frames), host(obss.fidx)) if isinstance(obss, ppo.FrameRows) else host(obss)
            snap = {"mem": {"obs": obs, "goal": host(goals), "speed": host(speeds), "action": host(actions),
                            "logprob": host(logprobs), "target": host(targets), "adv": host(advs)},
                    "drop": host(kw["filter_index"]) if stage2 else None, "state": state_of(kw["policy"]), "kw": kw,
                    "stage2": stage2, "log_from": len(kw["log"])}
            with recorded_randperm() as perms:
                real(*args, **kw)
            snap["perms"] = perms
            seen.append(snap)
        return update
    monkeypatch.setattr(ppo, "ppo_update_stage1", wrap(ppo.ppo_update_stage1, False))
    monkeypatch.setattr(ppo, "ppo_update_stage2", wrap(ppo.ppo_update_stage2, True))
    return seen


def trainer_update_against_the_model(tr, snap, want=None):
    """The update a trainer ran (``snap``: what snapshot_updates caught) against the model replayed from the snapshot.
    ``want``: the model's Update where a caller already has it for this very snapshot.  -> (D, per-tensor ratios, L, the Update)"""
    hp, kw = tr.hp, snap["kw"]
    assert kw["batch_size"] == hp.batch_size and kw["epoch"] == hp.epoch and len(snap["perms"]) == hp.epoch
    if want is None:
        want = update(snap["state"], snap["mem"], snap["drop"], [cut(p, hp.batch_size, snap["stage2"]) for p in snap["perms"]],
                      lr=hp.learning_rate, clip=hp.clip_value, value_coef=hp.value_coef, entropy_coef=hp.coeff_entropy,
                      every_state=False)
    log = tr.loss_log[snap["log_from"]:]
    assert len(log) == len(want.losses) > 0
    D, per = distance(snap["state"], state_of(tr.policy), want.states[-1])
    return D, per, loss_distance(log, want.losses), want


def gradient_distance(sizes, got, want, min_size=32):
    """G: the largest, over the parameter tensors of at least ``min_size`` elements, of ||g_got - g_want|| / ||g_want|| for one
    step's flat gradient.  (The four smaller tensors -- logstd and the three heads' biases -- are one or two sums over the
    minibatch that cancel: their relative error is one draw of rounding noise, and the quotient of two such draws says nothing.
    They are listed, not ranked.)  ``sizes``: {tensor: number of elements}.  -> (G, {tensor: its ratio})"""
    per, off = {}, 0
    for k in ORDER:
        a, b = got[off: off + sizes[k]], want[off: off + sizes[k]]
        per[k] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        off += sizes[k]
    return max(v for k, v in per.items() if sizes[k] >= min_size), per


def first_step(optimizer, policy):
    """Keep what the optimiser's FIRST step is handed and what it leaves -> a dict that then holds ``"grad"`` (the gradient, flat,
    ``parameters()`` order, float64 on the host) and ``"after"`` (the state dict behind that step, as ``state_of`` gives it)."""
    kept, real = {}, optimizer.step

    def step(*a, **kw):
        first = not kept
        if first:
            kept["grad"] = torch.cat([p.grad.detach().reshape(-1) for p in policy.parameters()]).double().cpu().numpy()
        out = real(*a, **kw)
        if first:
            kept["after"] = state_of(policy)
        return out
    optimizer.step = step
    return kept
