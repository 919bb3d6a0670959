"""Where an env's memory lies, as a list of configs and a restatement of the rule: what tools/make_golden_arena.py records into
tests/golden/arena_layout.json (mrca_arena_bytes of every config), what tests/test_arena_layout_host.py replays and holds
csrc/mrca_arena.h to, and what tests/test_gpu_arena_layout.py holds mrca_get_field to.

The configs are the smallest shapes at which a layout can go wrong: every part under one granule, the two sides of
robots_per_world = 64 (the big-world parts appear), of the power-of-two steps of the two hash masks and of the 1024-bucket block
count, every frame and beam count at the ends and in the middle, outlines or none, maps whose rows are no multiple of a word or
padded beyond need, the two stages as the scenarios give them -- and the configs mrca_arena_bytes refuses."""
import ctypes as C

import numpy as np

from mrca import _lib
from mrca import scenario as S

ALIGN = 256
DTYPE_BYTES = {"f32": 4, "u8": 1, "i32": 4, "i64": 8}
FIELD_PAD_X, FIELD_PAD_Y = 2, 1         # csrc/mrca_device.h: kFieldPadX, kFieldPadY
SLOT_PARTS = ("pose", "head", "goal", "fresh", "outline")       # what a slot of mrca_step_many's ring holds, in its order


def config_of(sc, lazy_obs=1):
    """mrca_config of a scenario, as VecStageWorld fills it -> (config, what must outlive its use)"""
    keep = [np.ascontiguousarray(sc.grid.bits, np.uint32), np.ascontiguousarray(sc.reset_mode, np.int32),
            np.ascontiguousarray(sc.goal_mode, np.int32), np.ascontiguousarray(sc.init_table, np.float32),
            np.ascontiguousarray(sc.goal_table, np.float32), np.ascontiguousarray(sc.group_id, np.int32)]
    bits, reset_mode, goal_mode, init_table, goal_table, group_id = (k.ctypes.data for k in keep)
    cfg = _lib.MrcaConfig(abi_version=_lib.ABI_VERSION, device=0, num_worlds=sc.num_worlds, robots_per_world=sc.robots_per_world,
                          beams=sc.beams, frames=sc.frames, map_width=sc.grid.width, map_height=sc.grid.height,
                          map_words_per_row=sc.grid.words_per_row, map_cell=sc.grid.cell, map_x0=sc.grid.x0, map_y0=sc.grid.y0,
                          map_bits=bits, timeout=sc.timeout, w_thresh=sc.w_thresh, pre_dist_zero=int(sc.pre_dist_zero),
                          auto_reset=sc.auto_reset, seed=sc.seed, reset_mode=reset_mode, goal_mode=goal_mode, init_table=init_table,
                          goal_table=goal_table, group_id=group_id, collision_raster=float(sc.collision_raster),
                          hold_velocity=int(bool(sc.hold_velocity)), lazy_obs=lazy_obs)
    return cfg, keep


def plain(num_worlds=1, robots_per_world=1, beams=64, frames=1, map_width=1, map_height=1, map_words_per_row=None,
          collision_raster=0.0):
    """a config of these dimensions on an empty map, no tables"""
    wpr = (map_width + 31) // 32 if map_words_per_row is None else map_words_per_row
    bits = np.zeros(max(1, map_height * wpr), np.uint32)
    cfg = _lib.MrcaConfig(abi_version=_lib.ABI_VERSION, device=0, num_worlds=num_worlds, robots_per_world=robots_per_world,
                          beams=beams, frames=frames, map_width=map_width, map_height=map_height, map_words_per_row=wpr,
                          map_cell=0.5, map_x0=0.0, map_y0=0.0, map_bits=bits.ctypes.data, timeout=150, w_thresh=1.05,
                          pre_dist_zero=0, auto_reset=1, seed=0, collision_raster=collision_raster, lazy_obs=1)
    return cfg, [bits]


def _bad(field, value, **stage1):
    def make():
        cfg, keep = config_of(S.stage1(**dict(dict(num_worlds=2, robots_per_world=8), **stage1)))
        setattr(cfg, field, value)
        return cfg, keep
    return make


def cases():
    """{key: function -> (config, keep)}"""
    out = {"1x1 b64 f1 map 1x1": plain}
    for r in (64, 65, 128, 129, 512, 513):          # (one world of more than 64: the hash masks and block count step with N)
        out[f"1x{r}"] = lambda r=r: plain(robots_per_world=r, map_width=8, map_height=8)
    for w, r in ((2, 64), (3, 43), (8, 64), (9, 57)):       # N = 128, 129, 512, 513 without the big-world parts
        out[f"{w}x{r}"] = lambda w=w, r=r: plain(num_worlds=w, robots_per_world=r, map_width=8, map_height=8)
    for f in (1, 3, 8):
        for b in (64, 512, 1024):
            out[f"2x3 b{b} f{f}"] = lambda f=f, b=b: plain(num_worlds=2, robots_per_world=3, beams=b, frames=f, map_width=8, map_height=8)
    for raster in (0.0, 0.2, 0.1):
        out[f"2x3 b128 f3 raster {raster}"] = lambda raster=raster: plain(num_worlds=2, robots_per_world=3, beams=128, frames=3,
                                                                           map_width=8, map_height=8, collision_raster=raster)
    out["map 33x1 wpr 2"] = lambda: plain(map_width=33, map_height=1, map_words_per_row=2)
    out["map 40x7 wpr 3"] = lambda: plain(map_width=40, map_height=7, map_words_per_row=3)
    out["stage1"] = lambda: config_of(S.stage1())
    out["stage2"] = lambda: config_of(S.stage2())
    # refused: tests/test_abi.py's test_config_validation_errors, and big worlds with group-synchronous episodes
    for field, value in (("robots_per_world", 0), ("beams", 500), ("frames", 0), ("abi_version", 99), ("map_cell", 0.0),
                         ("auto_reset", 7), ("num_worlds", 0), ("map_width", 0), ("map_height", 20000)):
        out[f"bad {field}={value}"] = _bad(field, value)
    out["bad robots_per_world=300 auto_reset=2"] = _bad("auto_reset", 2, robots_per_world=300)
    return out


def record(lib):
    """{key: [return code, bytes] or, refused, [return code, mrca_last_error()]}"""
    got = {}
    for key, make in cases().items():
        cfg, _keep = make()
        n = C.c_size_t()
        rc = lib.mrca_arena_bytes(C.byref(cfg), C.byref(n))
        got[key] = [rc, n.value] if rc == 0 else [rc, lib.mrca_last_error().decode()]
    return got


def align_up(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def restated_parts(cfg):
    """[(EnvView member, bytes)] in the arena's order: the public fields as _lib.FIELDS sizes them, the scenario and beam tables,
    the map and its two fields, head records, outlines, the ten big-world parts, the status word.  0 bytes: the part is absent."""
    R, B, F = cfg.robots_per_world, cfg.beams, cfg.frames
    N = cfg.num_worlds * R
    per_robot = {"B": B, "FB": F * B, "FW": F * (B // 64)}
    parts = [(name, N * per_robot.get(shape, shape) * DTYPE_BYTES[dt]) for name, dt, shape in _lib.FIELDS]
    parts += [("reset_mode", R * 4), ("goal_mode", R * 4), ("group_id", R * 4), ("init_table", R * 12), ("goal_table", R * 8),
              ("beam_cos", B * 4), ("beam_sin", B * 4),
              ("map_bits", cfg.map_height * cfg.map_words_per_row * 4),
              ("free_rect", (cfg.map_width + 2 * FIELD_PAD_X) * (cfg.map_height + 2 * FIELD_PAD_Y) * 4 * 2),
              ("cellfield", cfg.map_width * cfg.map_height),
              ("head", N * 16), ("outline", N * 16 if cfg.collision_raster > 0 else 0)]
    big = R > 64
    cmask, lmask = hash_masks(cfg)
    bw = [("bw_ticket", 4), ("bw_prov", N * 32), ("bw_state", N * 4), ("bw_chead", (cmask + 1) * 4), ("bw_cnext", 2 * N * 4),
          ("bw_lstart", (lmask + 3) * 4), ("bw_lcount", (lmask + 2) * 4), ("bw_lsorted", N * 4),
          ("bw_lblock", ((lmask + 1) // 1024 + 2) * 4), ("bw_lcursor", (lmask + 2) * 4)]
    parts += [(name, nbytes if big else 0) for name, nbytes in bw]
    return parts + [("status", 4)]


def hash_masks(cfg):
    """(bw_cmask, bw_lmask): the collision hash has the first power of two >= 4 N buckets, the lidar hash >= 2 N; (0, 0) for
    worlds of at most 64 robots"""
    N = cfg.num_worlds * cfg.robots_per_world
    if cfg.robots_per_world <= 64:
        return 0, 0
    return (1 << (4 * N - 1).bit_length()) - 1, (1 << (2 * N - 1).bit_length()) - 1


def restated_layout(cfg):
    """({member: (offset, bytes)}, total): each part at the running sum of the 256-aligned sizes before it"""
    at, off = {}, 0
    for name, nbytes in restated_parts(cfg):
        at[name] = (off, nbytes)
        off += align_up(nbytes)
    return at, off
