"""GPU: the refusals of the controllers' entry points that stand BEHIND the env -- what tests/test_abi_refusals_host.py cannot
reach with env = NULL -- with the whole text of mrca_last_error(), written out from the source as it stood before the entry
points moved to csrc/mrca_abi_controllers.hip.  Every call returns before any launch: the test costs an env and a reset.  (The
refusals that need a world of more than 64 robots are in test_gpu_orca_big.py, next to its env.)"""
import ctypes as C

import pytest
import torch

from util import S

pytestmark = pytest.mark.gpu


def test_refusals_behind_the_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import _lib
    from mrca.vec_env import VecStageWorld
    env = VecStageWorld(S.stage1(num_worlds=2, robots_per_world=6, seed=3))
    lib, h, N = env.lib, env._h, env.N
    f = torch.zeros(N * 64, device=env.device)
    i = torch.zeros(N * 64, dtype=torch.int32, device=env.device)
    fp, ip = C.c_void_p(f.data_ptr()), C.c_void_p(i.data_ptr())

    def refused(rc):
        return rc, lib.mrca_last_error().decode()

    def view(world):
        return (_lib.RenderView * 1)(_lib.RenderView(world, 0.0, 0.0, 0.1))

    # before the first reset
    st = env._stream()
    assert refused(lib.mrca_scan_noise(h, None, None, st)) == (-1, "mrca_scan_noise before the first mrca_reset: there is no scan yet")
    assert refused(lib.mrca_hybrid_actions(h, None, None, fp, fp, None, None, st)) == \
        (-1, "mrca_hybrid_actions before the first mrca_reset: there is no scan yet")
    assert refused(lib.mrca_hybrid_plan(h, None, None, None, ip, fp, fp, None, st)) == \
        (-1, "mrca_hybrid_plan before the first mrca_reset: there is no scan yet")
    assert refused(lib.mrca_goal_fields(h, None, fp, 6, ip, None, st)) == (-1, "mrca_goal_fields before the first mrca_reset")
    assert refused(lib.mrca_subgoals(h, None, ip, fp, 6, None, None, fp, None, None, None, st)) == \
        (-1, "mrca_subgoals before the first mrca_reset: there is no head record yet")
    assert refused(lib.mrca_subgoals(h, None, ip, fp, 4, ip, None, fp, None, None, None, st)) == \
        (-1, "mrca_subgoals before the first mrca_reset: there is no head record yet")
    # slot_dev NULL stands for slot = n % robots_per_world: only with as many goal points (judged before the reset is asked for)
    for G in (4, 7):
        assert refused(lib.mrca_subgoals(h, None, ip, fp, G, None, None, fp, None, None, None, st)) == \
            (-1, f"mrca_subgoals: slot_dev NULL (slot = n % robots_per_world) needs G == robots_per_world (6), got {G}")
    # a view's world
    for world in (2, -1):
        assert refused(lib.mrca_render(h, view(world), 1, 8, 8, 7, ip, None, None, st)) == \
            (-1, f"mrca_render: view 0 shows world {world} of 2")
    two = (_lib.RenderView * 2)(_lib.RenderView(1, 0.0, 0.0, 0.1), _lib.RenderView(5, 0.0, 0.0, 0.1))
    assert refused(lib.mrca_render(h, two, 2, 8, 8, 7, ip, None, None, st)) == (-1, "mrca_render: view 1 shows world 5 of 2")
    env.reset()
    # mrca_goal_fields synchronises the stream: not inside a capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            f.add_(1.0)
            got = refused(lib.mrca_goal_fields(h, None, fp, 6, ip, None, env._stream()))
    assert got == (-1, "mrca_goal_fields inside a stream capture: it synchronises the stream while it looks for convergence")
    torch.cuda.synchronize()
    env.check()                 # no HIP error was left behind
    assert not i.any()
    env.close()
