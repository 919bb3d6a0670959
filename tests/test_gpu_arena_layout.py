"""Where an env's memory lies, on the device: mrca_get_field of every field against the restatement of the layout
(arena_layout_cases.restated_layout), and an env in a caller's arena against what lies behind that arena and against a twin in
an arena of the library's own -- through reset, step and a run-ahead mrca_step_many, whose slots are sized from the same parts."""
import ctypes as C

import numpy as np
import pytest
import torch

import arena_layout_cases as AC
import util as U
from mrca import _lib
from mrca import scenario as S

pytestmark = pytest.mark.gpu


def scenario(num_worlds, robots_per_world, beams, frames=3, raster=0.0):
    sc = S.stage1(num_worlds=num_worlds, robots_per_world=robots_per_world, seed=5)
    sc.beams, sc.frames, sc.collision_raster = beams, frames, raster
    return sc


@pytest.mark.parametrize("shape", [(1, 1, 64, 1, 0.0), (2, 3, 128, 3, 0.2), (1, 65, 512, 3, 0.0)], ids=["1x1", "2x3 raster", "1x65"])
def test_get_field_gives_the_restated_layout(built_lib, shape):
    from mrca.vec_env import VecStageWorld
    sc = scenario(*shape)
    at, total = AC.restated_layout(AC.config_of(sc)[0])
    env = VecStageWorld(sc, device="cuda:0")
    try:
        assert env.arena.numel() == total
        for k, (name, _dt, _shape) in enumerate(_lib.FIELDS):
            ptr, off, nbytes = C.c_void_p(), C.c_size_t(), C.c_size_t()
            assert built_lib.mrca_get_field(env._h, k, C.byref(ptr), C.byref(off), C.byref(nbytes)) == 0
            assert (ptr.value - env.arena.data_ptr(), off.value, nbytes.value) == (at[name][0],) + at[name], (k, name)
    finally:
        env.close()


def _device_bytes(ptr, count):
    """`count` bytes of device memory that is no tensor's, through the HIP runtime the process has loaded already"""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths            # (one runtime in the process: mrca/_lib.py load())
    hip = C.CDLL(paths.pop())
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, count, 2) == 0           # hipMemcpyDeviceToHost
    return out


def test_a_callers_arena_is_kept_to_and_equals_the_librarys_own(built_lib):
    lib = built_lib
    sc = scenario(2, 8, 64)
    cfg, _keep = AC.config_of(sc)
    n = C.c_size_t()
    assert lib.mrca_arena_bytes(C.byref(cfg), C.byref(n)) == 0
    total, guard = n.value, 4096
    assert total == AC.restated_layout(cfg)[1]
    mine = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    rng = np.random.default_rng(11)
    actions = [torch.from_numpy(U.random_actions(rng, sc.num_robots)).cuda() for _ in range(9)]
    table = (C.c_void_p * 6)(*[a.data_ptr() for a in actions[3:]])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    envs = []
    try:
        for arena_ptr, arena_bytes in ((mine.data_ptr(), total), (None, 0)):
            h = C.c_void_p()
            _lib.check(lib.mrca_create(C.byref(cfg), arena_ptr, arena_bytes, C.byref(h)), "mrca_create")
            envs.append(h)
            _lib.check(lib.mrca_reset(h, None, None, None, stream), "mrca_reset")
            for a in actions[:3]:
                _lib.check(lib.mrca_step(h, a.data_ptr(), stream), "mrca_step")
            _lib.check(lib.mrca_step_many(h, table, 6, 0, 6, 2, stream), "mrca_step_many")
            torch.cuda.synchronize()
            _lib.check(lib.mrca_check(h, stream), "mrca_check")
        ptr, off = C.c_void_p(), C.c_size_t()
        assert lib.mrca_get_field(envs[1], 0, C.byref(ptr), C.byref(off), None) == 0
        twin = _device_bytes(ptr.value - off.value, total)
        got = mine.cpu().numpy()
        assert (got[total:] == 0xA5).all()              # nothing behind mrca_arena_bytes was written
        assert np.array_equal(got[:total], twin)
        assert got[:total].any() and not (got[:total] == 0xA5).all()
    finally:
        for h in envs:
            lib.mrca_destroy(h)
