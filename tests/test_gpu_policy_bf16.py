"""GPU: the opt-in bf16 rollout inference -- the bf16 MFMA front end (csrc/mrca_policy_bf16.hip) against its rounding-point
reference (tests/bf16_ref.py), and act_fused(bf16=True) / the trainer / the evaluate CLI against the fp32 fused path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_ref as R
import util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pol():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca.net import CNNPolicy
    torch.manual_seed(3)
    p = CNNPolicy(3, 2).cuda()
    with torch.no_grad():                      # not the symmetric default init: distinct, sizeable biases
        for q in p.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return p


def _ckpt(name):
    from mrca.net import CNNPolicy
    p = CNNPolicy(3, 2).cuda()
    p.load_state_dict(torch.load(os.path.join(U.ROOT, "rl-collision-avoidance_amd", "mrca", "data", name), map_location="cuda"))
    return p


@pytest.mark.parametrize("n", [1, 2, 3, 7, 255, 4096, 5000])
def test_front_end_follows_the_rounding_points(pol, n):
    from mrca import policy_ops
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand(n, 3, 512, device="cuda", generator=g) - 0.5
    rc = pol.refresh_rollout_cache()
    feat = policy_ops.lidar_features_bf16(x, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    assert feat.shape == (2, n, 4096) and feat.dtype == torch.bfloat16
    got = feat.float().cpu().numpy()
    xs = x.cpu().numpy()
    same = total = 0
    for t in range(2):
        want, exact, S = R.front_end_ref(xs, rc["w1"][t].cpu().numpy(), rc["b1"][t].cpu().numpy(), rc["w2"][t].cpu().numpy(),
                                         rc["b2"][t].cpu().numpy())
        err = np.abs(got[t].astype(np.float64) - exact)
        bound = 2.0 ** -8 * np.abs(exact) + 2.0 ** -12 * S
        bad = err > bound
        # an h1 element that rounds the other way moves its conv2 terms by one bf16 ulp (<= 2^-7 of the term): spread over
        # 96 terms that is inside 2^-12 S, but where one term dominates S it is not -- measured: at most 8 of 16.8 M elements
        # per tower (n = 4096), at most 1.6e-4 over (profiles/bf16/test_gpu_policy_bf16.txt).  Those few must stay inside one
        # h1 ulp of the whole sum.
        if bad.any():
            print(f"n={n} tower {t}: {int(bad.sum())} elements over 2^-8 |ref| + 2^-12 S, worst by {float((err - bound).max()):.3g}")
        assert int(bad.sum()) <= 1e-5 * err.size, (t, n, int(bad.sum()))
        assert (err <= 2.0 ** -8 * np.abs(exact) + 2.0 ** -7 * S).all(), (t, n)
        assert float(np.abs(exact).max()) > 0.05           # not a comparison between zeros
        same += int((got[t] == want).sum())
        total += want.size
    print(f"n={n}: {same / total:.5f} of the bf16 features bit-identical to the rounding-point reference")
    assert same >= 0.99 * total


def test_ring_form_equals_deque_form_and_launches_repeat(pol):
    from mrca import policy_ops
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(U.S.stage1(num_worlds=8, robots_per_world=24, seed=2), device="cuda:0")
    env.reset()
    rc = pol.refresh_rollout_cache()
    g = torch.Generator(device="cuda").manual_seed(0)
    for k in range(5):
        a = torch.stack([torch.rand(env.N, generator=g, device="cuda"), torch.rand(env.N, generator=g, device="cuda") * 2 - 1], 1)
        env.step(a.contiguous())
        ring, head = env.policy_obs()
        via_ring = policy_ops.lidar_features_bf16(ring, rc["w1"], rc["b1"], rc["w2"], rc["b2"], head=head)
        via_copy = policy_ops.lidar_features_bf16(env.obs, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
        again = policy_ops.lidar_features_bf16(env.obs, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
        assert torch.equal(via_ring, via_copy) and torch.equal(via_copy, again), k
    env.close()


def test_rejects_a_frame_table_and_other_geometries(pol):
    from mrca import policy_ops
    rc = pol.refresh_rollout_cache()
    table = policy_ops.FrameTable(torch.zeros(6, 512, device="cuda"), torch.zeros(2, 3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        policy_ops.lidar_features_bf16(table, rc["w1"], rc["b1"], rc["w2"], rc["b2"])
    with pytest.raises(ValueError):
        policy_ops.lidar_features_bf16(torch.zeros(4, 3, 256, device="cuda"), rc["w1"], rc["b1"], rc["w2"], rc["b2"])


def test_act_fused_bf16_is_bounded_against_fp32():
    """The bounds of test_gpu_policy_ops.py::test_bf16_inference_is_bounded_against_fp32 (autocast on the stock layers),
    here for the fused bf16 path against the fused fp32 path on the same circle observations."""
    from mrca import evaluate, ppo
    from mrca import scenario as S
    from mrca.vec_env import VecStageWorld
    pol = _ckpt("policy_r02_stage2_circles.pth")
    env = VecStageWorld(S.circle(num_worlds=20, seed=0))
    env.reset()
    lo, hi = ppo._bounds(evaluate.ACTION_BOUND, env.device, torch.float32)
    worst_m, worst_v, sum_m, cnt = 0.0, 0.0, 0.0, 0
    for k in range(240):
        obs, head = ppo.policy_input(env, True)
        v32, _a, _lp, s32, m32 = pol.act_fused(obs, env.local_goal, env.speed, None, lo, hi, head=head)
        v16, _a, _lp, _s, m16 = pol.act_fused(obs, env.local_goal, env.speed, None, lo, hi, head=head, bf16=True)
        worst_m = max(worst_m, float((m32 - m16).abs().max()))
        sum_m += float((m32 - m16).abs().mean())
        cnt += 1
        worst_v = max(worst_v, float(((v32 - v16).abs() / (1.0 + v32.abs())).max()))
        env.step(s32.contiguous())
    print(f"fused bf16 vs fused fp32 over 240 circle ticks x 1000 robots: max |d mean| {worst_m:.4f} "
          f"(mean {sum_m / cnt:.5f}), max |d value| / (1 + |value|) {worst_v:.4f}")
    assert worst_m < 0.25 and sum_m / cnt < 0.02 and worst_v < 0.3
    env.close()


def test_success_rate_under_fused_bf16():
    """North-star tolerance: on 20 perturbed circles (identical seeds), SR(bf16 fused) >= SR(fp32 fused) - 0.02."""
    from mrca import evaluate
    from mrca import scenario as S
    from mrca.vec_env import VecStageWorld
    pol = _ckpt("policy_r03_fused_update_11min.pth")
    sr = {}
    for bf16 in (False, True):
        env = VecStageWorld(S.circle(num_worlds=20, seed=0))
        fn = evaluate.cnn_policy_fn(pol, fused=True, env=env, fused_bf16=bf16)
        m = evaluate.circle_test(env, fn, max_ticks=1500, perturb=(0.2, 0.1), seed=0)
        sr[bf16] = m["success_rate"]
        env.close()
    print(f"circle SR on 20 perturbed circles: fp32 fused {sr[False]:.4f}, bf16 fused {sr[True]:.4f}")
    assert sr[True] >= sr[False] - 0.02


def test_graph_replay_is_bit_identical(pol):
    from mrca import ppo
    n = 1000
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, 3, 512, device="cuda", generator=g) - 0.5
    goal = torch.rand(n, 2, device="cuda", generator=g) * 20 - 10
    speed = torch.rand(n, 2, device="cuda", generator=g)
    noise = torch.randn(n, 2, device="cuda", generator=g)
    lo, hi = ppo._bounds(((0.0, -1.0), (1.0, 1.0)), x.device, torch.float32)
    eager = pol.act_fused(x, goal, speed, noise, lo, hi, bf16=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act_fused(x, goal, speed, noise, lo, hi, bf16=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = pol.act_fused(x, goal, speed, noise, lo, hi, bf16=True)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_with_the_bf16_rollout(graph):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mrca import ppo
    from mrca.trainer import HParams, Stage1Trainer
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(U.S.stage1(num_worlds=4, robots_per_world=24, seed=8))
    hp = HParams(horizon=16, batch_size=192, epoch=1, rollout_fused=True, rollout_bf16=True, graph_tick=graph)
    tr = Stage1Trainer(env, hp=hp, seed=4)
    tr.start()
    if not graph:
        # the first tick's stored action is generate_action(fused, fused_bf16) on the same noise, bit for bit
        gen = torch.Generator(device="cuda")
        gen.set_state(tr.gen.get_state())
        obs, head = ppo.policy_input(env, True)
        _v, a_ref, _lp, _s = ppo.generate_action(tr.policy, obs, env.local_goal, env.speed, hp.action_bound, gen,
                                                  fused=True, obs_head=head, fused_bf16=True)
        a_ref = a_ref.clone()
        tr.tick()
        torch.cuda.synchronize()
        assert torch.equal(tr.buffer.action[0], a_ref)
        ticks = 2 * hp.horizon - 1
    else:
        ticks = 2 * hp.horizon
    for _ in range(ticks):
        tr.tick()
    torch.cuda.synchronize()
    assert tr.global_update == 2 and len(tr.loss_log) > 0
    assert all(torch.isfinite(torch.stack(x)).all() for x in tr.loss_log)
    assert tr.policy._rc_bf16 is not None
    env.close()


def test_fused_bf16_needs_the_fused_path(pol):
    from mrca import ppo
    x = torch.zeros(4, 3, 512, device="cuda")
    z = torch.zeros(4, 2, device="cuda")
    with pytest.raises(ValueError):
        ppo.generate_action(pol, x, z, z, ((0.0, -1.0), (1.0, 1.0)), fused=False, fused_bf16=True)
    with pytest.raises(ValueError):
        ppo.generate_action_no_sampling(pol, x, z, z, ((0.0, -1.0), (1.0, 1.0)), fused=False, fused_bf16=True)


def test_evaluate_cli_fused_bf16():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ck = os.path.join(U.ROOT, "rl-collision-avoidance_amd", "mrca", "data", "policy_r02_stage2_circles.pth")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), U.ROOT]))
    r = subprocess.run([sys.executable, "-m", "mrca.evaluate", "--circles", "2", "--fused-bf16", "--policy", ck,
                        "--max-ticks", "200"], cwd=U.ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '"inference_precision": "bf16' in r.stdout, r.stdout[-2000:]
