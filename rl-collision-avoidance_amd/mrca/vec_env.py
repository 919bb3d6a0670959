"""VecStageWorld -- the batched, device-resident replacement of N ``StageWorld`` objects.

One instance owns one libmrca_env handle on one GPU.  Every reference getter
(stage_world1.py:116-160) is a zero-copy torch view on a field of the env's device arena;
``step`` is one trip round the reference's loop body (ppo_stage1.py:75-91) for all robots at
once.  torch is used for device memory and streams only; all arithmetic runs in the HIP library.
"""
import ctypes as C
import operator

import numpy as np
import torch

from . import _lib
from .scenario import Scenario

_DTYPES = {"f32": torch.float32, "u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}

RESULT_NAMES = {0: 0, 1: "Reach Goal", 2: "Crashed", 3: "Time out"}  # stage_world1.py:190-208


def sparse_beam_index(raw_beams, beam_num):
    """The beams get_laser_observation keeps when the world was constructed with ``beam_num`` != the lidar's sample count
    (stage_world1.py:126-139): a float64 index advanced by raw / beam_num per pick and truncated, beam_num / 2 picks
    ascending from beam 0 and beam_num / 2 descending from the last beam (the right half then reversed)."""
    step = float(raw_beams) / beam_num
    left, right = [], []
    index = 0.0
    for _ in range(int(beam_num / 2)):
        left.append(int(index))
        index += step
    index = raw_beams - 1.0
    for _ in range(int(beam_num / 2)):
        right.append(int(index))
        index -= step
    return np.asarray(left + right[::-1], np.int32)


class VecStageWorld:
    def __init__(self, scenario: Scenario, device=None, lib_path=None, lazy_obs=True, scan_noise=None):
        """``lazy_obs=False``: the library forms the two reference-shaped views (MRCA_F_SCAN, MRCA_F_OBS) inside every
        ``step`` / ``reset`` -- what a plain C caller written against the reference's getters expects (mrca_config.lazy_obs
        = 0: one more kernel per call); the default leaves them to the ``scan`` / ``obs`` properties.
        ``scan_noise``: a ``noise.ScanNoiseParams`` -- the lidar noise model (mrca_scan_noise) is then applied once behind every
        ray cast of ``reset`` / ``step`` / ``observe``, to exactly the robots that call cast; ``step_many`` refuses.  ``None``
        (the default): exact ranges, nothing is launched."""
        if not torch.cuda.is_available():
            raise RuntimeError("VecStageWorld needs an MI355X (torch.cuda is unavailable); there is no CPU path")
        self.lib = _lib.load(lib_path)      # lib_path: another build of the same library (the profiling build)
        self.scenario = sc = scenario
        if device is None:
            index = torch.cuda.current_device()
        else:
            d = torch.device(device)
            index = d.index if d.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self.N, self.R, self.W = sc.num_robots, sc.robots_per_world, sc.num_worlds
        self.B, self.F = sc.beams, sc.frames

        # host-side tables must outlive mrca_create only
        bits = np.ascontiguousarray(sc.grid.bits, dtype=np.uint32)
        reset_mode = np.ascontiguousarray(sc.reset_mode, np.int32)
        goal_mode = np.ascontiguousarray(sc.goal_mode, np.int32)
        group_id = np.ascontiguousarray(sc.group_id, np.int32)
        init_table = np.ascontiguousarray(sc.init_table, np.float32)
        goal_table = np.ascontiguousarray(sc.goal_table, np.float32)
        cfg = _lib.MrcaConfig(
            abi_version=_lib.ABI_VERSION, device=self.device.index, num_worlds=sc.num_worlds,
            robots_per_world=sc.robots_per_world, beams=sc.beams, frames=sc.frames,
            map_width=sc.grid.width, map_height=sc.grid.height, map_words_per_row=sc.grid.words_per_row,
            map_cell=sc.grid.cell, map_x0=sc.grid.x0, map_y0=sc.grid.y0, map_bits=bits.ctypes.data,
            timeout=sc.timeout, w_thresh=sc.w_thresh, pre_dist_zero=int(sc.pre_dist_zero),
            auto_reset=sc.auto_reset, seed=sc.seed, reset_mode=reset_mode.ctypes.data,
            goal_mode=goal_mode.ctypes.data, init_table=init_table.ctypes.data,
            goal_table=goal_table.ctypes.data, group_id=group_id.ctypes.data,
            collision_raster=float(getattr(sc, "collision_raster", 0.0)),
            hold_velocity=int(bool(getattr(sc, "hold_velocity", False))),
            lazy_obs=1 if lazy_obs else 0)   # 1: MRCA_F_OBS is materialised by the ``obs`` property when somebody asks for it
        nbytes = C.c_size_t()
        _lib.check(self.lib.mrca_arena_bytes(C.byref(cfg), C.byref(nbytes)), "mrca_arena_bytes")
        # the arena is a torch allocation so that every field is a plain torch view (zero copy)
        self.arena = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mrca_create(C.byref(cfg), self.arena.data_ptr(), nbytes.value, C.byref(handle)),
                       "mrca_create")
        self._h = handle
        for k, (name, dt, shape) in enumerate(_lib.FIELDS):
            ptr, off, nb = C.c_void_p(), C.c_size_t(), C.c_size_t()
            _lib.check(self.lib.mrca_get_field(self._h, k, C.byref(ptr), C.byref(off), C.byref(nb)), "mrca_get_field")
            assert ptr.value == self.arena.data_ptr() + off.value
            flat = self.arena[off.value: off.value + nb.value].view(_DTYPES[dt])
            if shape == "B":
                t = flat.view(self.N, self.B)
            elif shape == "FB":
                t = flat.view(self.N, self.F, self.B)
            elif shape == "FW":
                t = flat.view(self.N, self.F, self.B // 64)
            elif shape == 1:
                t = flat.view(self.N)
            else:
                t = flat.view(self.N, shape)
            setattr(self, "_" + name if name in ("obs", "scan") else name, t)
        self._eager_views = 0 if lazy_obs else (_lib.VIEW_SCAN | _lib.VIEW_OBS)   # views the library itself keeps current
        self._views_current = 0          # bits of _lib.VIEW_*: which of MRCA_F_SCAN / MRCA_F_OBS follow the ring right now
        self._scan_noise = None if scan_noise is None else scan_noise.struct()
        self._scatter_boxes = None       # (the boxes' bytes, their float32[R,8] tensor on the device): what scatter() uploaded last
        self._noise_masks = {}           # (first, count) -> uint8[N] with ones in that range of robots: kept, so a capture can replay them

    # ------------------------------------------------------------------ the scans and the observation stack
    # The env keeps the last F scans of every robot as a RING of raw ranges (``scan_ring`` + ``ring_head``: a tick writes
    # ONE row per robot -- no shift, no second normalised copy) and makes the two reference-shaped views when somebody
    # reads them after a tick (mrca_materialize: one kernel on the current stream).  The fused policy path reads the ring.
    def _view(self, bit, what):
        if not self._views_current & bit:
            _lib.check(self.lib.mrca_materialize(self._h, bit, self._stream()), "mrca_materialize")
            self._views_current |= bit
        return what

    @property
    def scan(self):
        """f32[N,B] the newest scan of every robot (base_scan ranges, stageros.cpp:479-516)."""
        return self._view(_lib.VIEW_SCAN, self._scan)

    @property
    def obs(self):
        """f32[N,F,B] the observation stacks x / 6 - 0.5 in deque order (oldest frame first; what ``CNNPolicy.forward``
        eats: stage_world1.py:140, ppo_stage1.py:59-60,87-89)."""
        return self._view(_lib.VIEW_OBS, self._obs)

    @property
    def hit_robot(self):
        """bool[N,B]: beam b of robot n returned from ANOTHER ROBOT (the newest scan's words of MRCA_F_HIT_BITS, one bit per
        beam; clear = the floorplan or no return).  stageros publishes it as LaserScan.intensities: 1 floorplan, 0 robot or
        miss (stageros.cpp:501-506, ranger_return 0.5 cast to uint8)."""
        ar = torch.arange(self.N, device=self.device)
        words = self.hit_bits[ar, self.ring_head.long()]                       # i64 [N, B/64]
        bit = torch.arange(64, device=self.device, dtype=torch.int64)
        return ((words.unsqueeze(-1) >> bit) & 1).bool().reshape(self.N, self.B)

    def invalidate_views(self):
        """Tell the binding that the env moved on without it: ticks replayed as a hipGraph (or stepped by another binding of
        the same handle) advance the scan ring behind its back, so ``scan`` / ``obs`` must be formed again at their next
        read.  (With ``lazy_obs=False`` the replayed ticks re-formed them themselves.)"""
        self._views_current = self._eager_views

    @property
    def _obs_current(self):
        return bool(self._views_current)

    @_obs_current.setter
    def _obs_current(self, value):      # (older spelling of invalidate_views(), kept for callers written against it)
        if not value:
            self.invalidate_views()

    def policy_obs(self):
        """-> (ring, heads) for consumers that understand the ring: (scan_ring f32[N,F,B] of RAW ranges, RingHead)."""
        from .policy_ops import RingHead
        return self.scan_ring, RingHead(self.ring_head, raw=True)

    def newest_frame(self, out=None):
        """f32[N,B]: every robot's newest observation row x / 6 - 0.5 (the frame a tick appended), from the ring."""
        if out is None:
            out = torch.empty(self.N, self.B, dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.N * self.B):
            raise ValueError("newest_frame: out must be a contiguous cuda float32 tensor of N x B elements")
        _lib.check(self.lib.mrca_newest_obs(self._h, out.data_ptr(), self._stream()), "mrca_newest_obs")
        return out

    # ---- the learner's rollout buffer written by the library (include/mrca_env.h: mrca_rollout_rows)
    def rollout_rows(self, buf):
        """The C view of a one-frame-per-tick ``ppo.RolloutBuffer`` of this env's shape (checked here, once): hand it to
        ``rollout_store_state`` / ``rollout_store_outcome``.  Keeps the buffer's tensors alive."""
        T, N, F, B = buf.horizon, self.N, self.F, self.B
        want = {"frames": (torch.float32, (T + F - 1, N, B)), "fidx": (torch.int64, (T, N, F)), "_cur": (torch.int64, (N, F)),
                "goal": (torch.float32, (T, N, 2)), "speed": (torch.float32, (T, N, 2)), "action": (torch.float32, (T, N, 2)),
                "logprob": (torch.float32, (T, N, 1)), "value": (torch.float32, (T, N)), "reward": (torch.float32, (T, N)),
                "done": (torch.uint8, (T, N))}
        rows = _lib.RolloutRows()
        for name, (dtype, shape) in want.items():
            t = getattr(buf, name, None)
            if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f"rollout_rows: buffer.{name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}"
                                 + (f", got {tuple(t.shape)} {t.dtype} {t.device}" if torch.is_tensor(t) else ""))
            setattr(rows, name.lstrip("_"), t.data_ptr())
        rows.horizon = T
        rows._keep = buf
        return rows

    def rollout_store_state(self, rows, tick, action, logprob, value):
        """Row ``tick`` (int64[1] on the device) of the buffer before the env steps: newest frame, stack rows, goal, speed and
        the policy's ``action`` f32[N,2] / ``logprob`` / ``value`` (N elements each) -- one launch."""
        if not (tick.is_cuda and tick.dtype == torch.int64 and tick.numel() == 1):
            raise ValueError("rollout_store_state: tick must be an int64[1] cuda tensor")
        _lib.check(self.lib.mrca_rollout_store_state(self._h, C.byref(rows), tick.data_ptr(), self._ptr(action, torch.float32, 2 * self.N),
                                                     self._ptr(logprob, torch.float32, self.N), self._ptr(value, torch.float32, self.N),
                                                     self._stream()), "mrca_rollout_store_state")

    def rollout_store_outcome(self, rows, tick, ticket):
        """... and after it stepped: reward / done into row ``tick``, then ``tick += 1`` on the device -- one launch.
        ``ticket``: a zeroed int32[1] cuda tensor of the caller's, the same one for every call."""
        if not (tick.is_cuda and tick.dtype == torch.int64 and tick.numel() == 1 and ticket.is_cuda and ticket.dtype == torch.int32
                and ticket.numel() == 1):
            raise ValueError("rollout_store_outcome: tick int64[1] and ticket int32[1] cuda tensors")
        _lib.check(self.lib.mrca_rollout_store_outcome(self._h, C.byref(rows), tick.data_ptr(), ticket.data_ptr(), self._stream()),
                   "mrca_rollout_store_outcome")

    def sparse_obs(self, beam_num):
        """f32[N,F,beam_num]: the observation stacks a ``StageWorld(beam_num, ...)`` with beam_num != 512 would build
        (stage_world1.py:126-140), formed on the device from the ring."""
        cache = self.__dict__.setdefault("_sparse_index", {})
        if beam_num not in cache:
            cache[beam_num] = torch.from_numpy(sparse_beam_index(self.B, beam_num)).to(self.device)
        idx = cache[beam_num]
        out = torch.empty(self.N, self.F, idx.numel(), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mrca_sparse_obs(self._h, idx.data_ptr(), idx.numel(), out.data_ptr(), self._stream()),
                   "mrca_sparse_obs")
        return out

    # ------------------------------------------------------------------ looking at worlds (mrca_render)
    def default_view(self, size=(256, 256)):
        """(cx, cy, m_per_px) of the view that fits the map's extent into ``size`` = (width, height) pixels -- or, for an
        all-free map (``scenario.empty_grid``: the open world of ``circle_big``), the bounding box of the init and goal tables
        plus 1 m on every side."""
        g, sc = self.scenario.grid, self.scenario
        if np.asarray(g.bits).any():
            lo = np.array([g.x0, g.y0], np.float64)
            hi = lo + np.array([g.width, g.height], np.float64) * g.cell
        else:
            pts = np.concatenate([np.asarray(sc.init_table)[:, :2], np.asarray(sc.goal_table)[:, :2]])
            lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
        ext = hi - lo
        return float(0.5 * (lo[0] + hi[0])), float(0.5 * (lo[1] + hi[1])), float(max(ext[0] / size[0], ext[1] / size[1]))

    def render(self, worlds=None, size=(256, 256), centre=None, m_per_px=None,
               layers=_lib.RENDER_MAP | _lib.RENDER_GOALS | _lib.RENDER_BODIES, trail=None, out=None):
        """Top-down pictures of ``worlds`` (default: all, at most 256 per call) as a uint8[V,H,W,3] tensor on the env's device,
        rendered from the env's fields as they stand on the current stream: nothing synchronises, nothing of the env is
        written.  ``size`` = (width, height); ``centre`` = (cx, cy) or [V,2] and ``m_per_px`` = a number or [V] default to
        ``default_view``; ``layers``: bits of ``_lib.RENDER_*``; ``trail``: an int32[V,H,W] tensor of the caller's that
        collects where robots have been (zero it to start over); ``out``: the picture's tensor to reuse.  The ID image of the
        call (layer << 24 | local robot index per pixel, int32[V,H,W]) stays in ``self.render_ids``."""
        worlds = list(range(self.W)) if worlds is None else [int(w) for w in worlds]
        V, (Wp, Hp) = len(worlds), (int(size[0]), int(size[1]))
        if not (0 < V <= 256 and 0 < Wp <= 4096 and 0 < Hp <= 4096):       # (mrca_render's own limits, before anything is allocated)
            raise ValueError(f"render: {V} views of {Wp} x {Hp} pixels; a call takes 1..256 views of 1..4096 pixels a side")
        dcx, dcy, dm = self.default_view((Wp, Hp))
        cen = np.broadcast_to(np.asarray((dcx, dcy) if centre is None else centre, np.float64), (V, 2))
        mpp = np.broadcast_to(np.asarray(dm if m_per_px is None else m_per_px, np.float64), (V,))
        views = (_lib.RenderView * V)(*[_lib.RenderView(w, cen[v, 0], cen[v, 1], mpp[v]) for v, w in enumerate(worlds)])
        ids = getattr(self, "render_ids", None)
        if ids is None or tuple(ids.shape) != (V, Hp, Wp):
            ids = self.render_ids = torch.empty((V, Hp, Wp), dtype=torch.int32, device=self.device)
        if trail is not None and not (trail.is_cuda and trail.dtype == torch.int32 and trail.is_contiguous()
                                      and tuple(trail.shape) == (V, Hp, Wp)):
            raise ValueError(f"render: trail must be a contiguous cuda int32 tensor of shape {(V, Hp, Wp)}")
        if out is None:
            out = torch.empty((V, Hp, Wp, 3), dtype=torch.uint8, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (V, Hp, Wp, 3)):
            raise ValueError(f"render: out must be a contiguous cuda uint8 tensor of shape {(V, Hp, Wp, 3)}")
        _lib.check(self.lib.mrca_render(self._h, views, V, Wp, Hp, int(layers), ids.data_ptr(),
                                        None if trail is None else trail.data_ptr(), out.data_ptr(), self._stream()), "mrca_render")
        return out

    def orca_actions(self, params=None, mask=None, out=None, vel=None):
        """(v, omega) of the ORCA baseline controller (mrca_orca_actions) for every robot, as a float32[N,2] tensor on the env's
        device, from the env's fields as they stand on the current stream: one launch, nothing synchronises, nothing of the
        env is written -- ``env.step(env.orca_actions())`` is a closed-loop scripted tick.  ``params``: an ``orca.OrcaParams``
        (default: the library's); ``mask``: a uint8[N] tensor, rows with 0 keep what ``out`` holds (so a policy's actions can
        be passed as ``out`` and ORCA overwrites its robots' rows); ``vel``: a float32[N,2] tensor that takes the holonomic
        velocity chosen.
        Worlds of more than 64 robots (``scenario.circle_big``) go through mrca_orca_actions_any: the same rule with the
        neighbours found through the env's lidar hash, ``neighbor_dist`` up to 19.3 m; between ``move`` and ``observe`` it
        raises (the hash describes the poses before the move).  Smaller worlds keep mrca_orca_actions."""
        if out is None:
            out = torch.zeros((self.N, 2), dtype=torch.float32, device=self.device)
        st = None if params is None else params.struct()
        name = "mrca_orca_actions_any" if self.R > 64 else "mrca_orca_actions"
        _lib.check(getattr(self.lib, name)(self._h, None if st is None else C.byref(st), self._ptr(mask, torch.uint8, self.N),
                                           self._ptr(out, torch.float32, 2 * self.N), self._ptr(vel, torch.float32, 2 * self.N),
                                           self._stream()), name)
        return out

    def nhorca_actions(self, params=None, mask=None, out=None, vel=None, mode=None):
        """(v, omega) of the NH-ORCA baseline controller (mrca_nhorca_actions) for every robot, as a float32[N,2] tensor on the
        env's device: ORCA restricted to the holonomic velocities a unicycle tracks within ``track_error`` metres, every disc grown
        by that much.  One launch on the current stream, nothing synchronises, nothing of the env is written:
        ``env.step(env.nhorca_actions())`` is a closed-loop scripted tick.  ``params``: an ``nhorca.NhOrcaParams`` (default: the
        library's); ``mask`` and ``out``: as ``orca_actions``; ``vel``: a float32[N,2] tensor that takes the velocity of the
        tracked solve; ``mode``: an int32[N] tensor that takes what each robot does (0 tracks its preferred velocity, 1 turns in
        place, 2 stands still, 3 moves although it should turn).  Worlds of any size, under ``orca_actions``' rules for worlds of
        more than 64 robots."""
        if out is None:
            out = torch.zeros((self.N, 2), dtype=torch.float32, device=self.device)
        st = None if params is None else params.struct()
        _lib.check(self.lib.mrca_nhorca_actions(self._h, None if st is None else C.byref(st), self._ptr(mask, torch.uint8, self.N),
                                                self._ptr(out, torch.float32, 2 * self.N), self._ptr(vel, torch.float32, 2 * self.N),
                                                self._ptr(mode, torch.int32, self.N), self._stream()), "mrca_nhorca_actions")
        return out

    def dwa_actions(self, params=None, mask=None, out=None, choice=None, score=None, goal=None):
        """(v, omega) of the DWA baseline controller (mrca_dwa_actions) for every robot, as a float32[N,2] tensor on the env's
        device: the sensor-level counterpart of ``orca_actions`` -- it reads each robot's newest scan, local goal and own speed
        and nothing of any other robot, so it takes worlds of any size.  One launch on the current stream, nothing
        synchronises, nothing of the env is written: ``env.step(env.dwa_actions())`` is a closed-loop scripted tick.
        ``params``: a ``dwa.DwaParams`` (default: the library's); ``mask``: a uint8[N] tensor, rows with 0 keep what ``out``
        (and ``choice`` / ``score``) hold; ``choice``: an int32[N] tensor that takes the candidate chosen (-1: none was
        admissible, -2: at the goal); ``score``: a float32[N] tensor that takes its score; ``goal``: a float32[N,2] tensor in
        the robots' frames to steer at in place of ``env.local_goal`` (mrca_dwa_actions_goal) -- ``subgoals_los(...)[0]``; a
        subgoal within 0.5 m stops the robot, so the planner's lookahead must reach further than that."""
        if out is None:
            out = torch.zeros((self.N, 2), dtype=torch.float32, device=self.device)
        st = None if params is None else params.struct()
        args = (self._h, None if st is None else C.byref(st), self._ptr(mask, torch.uint8, self.N),
                self._ptr(out, torch.float32, 2 * self.N), self._ptr(choice, torch.int32, self.N), self._ptr(score, torch.float32, self.N))
        if goal is None:
            _lib.check(self.lib.mrca_dwa_actions(*args, self._stream()), "mrca_dwa_actions")
        else:
            _lib.check(self.lib.mrca_dwa_actions_goal(*args, self._ptr(goal, torch.float32, 2 * self.N), self._stream()),
                       "mrca_dwa_actions_goal")
        return out

    def hybrid_actions(self, actions, params=None, mask=None, out=None, mode=None, clear=None, goal=None):
        """Hybrid control behind a policy (mrca_hybrid_actions): per robot, ``actions`` (float32[N,2], the policy's (v, omega))
        replaced by a PID law where nothing stands between the robot and its goal, scaled down in v where something is
        dangerously close, kept as it is elsewhere -- decided from each robot's newest scan and local goal alone.  One launch
        on the current stream, nothing synchronises, nothing of the env is written: ``env.step(env.hybrid_actions(a))`` is one
        tick.  ``out=None`` works IN PLACE on ``actions`` and returns it.  ``params``: a ``hybrid.HybridParams`` (default: the
        library's); ``mask``: a uint8[N] tensor, rows with 0 keep what ``out`` (and ``mode`` / ``clear``) hold; ``mode``: an
        int32[N] tensor that takes 0 (the policy), 1 (PID), 2 (the policy made careful) or -2 (at the goal); ``clear``: a
        float32[N,3] tensor that takes (d_min, d_front, d_block); ``goal``: a float32[N,2] tensor in the robots' frames that
        stands where ``env.local_goal`` would (mrca_hybrid_actions_goal), as for ``dwa_actions``."""
        if out is None:
            out = actions
        st = None if params is None else params.struct()
        args = (self._h, None if st is None else C.byref(st), self._ptr(mask, torch.uint8, self.N),
                self._ptr(actions, torch.float32, 2 * self.N), self._ptr(out, torch.float32, 2 * self.N),
                self._ptr(mode, torch.int32, self.N), self._ptr(clear, torch.float32, 3 * self.N))
        if goal is None:
            _lib.check(self.lib.mrca_hybrid_actions(*args, self._stream()), "mrca_hybrid_actions")
        else:
            _lib.check(self.lib.mrca_hybrid_actions_goal(*args, self._ptr(goal, torch.float32, 2 * self.N), self._stream()),
                       "mrca_hybrid_actions_goal")
        return out

    def hybrid_plan(self, params=None, safe=None, mask=None, mode=None, scale=None, pid=None, clear=None, goal=None):
        """The first half of hybrid control in the paper's form (mrca_hybrid_plan): per robot, from its newest scan and local
        goal alone -- no command is read -- the mode ``hybrid_actions`` would report (int32[N]: 0, 1, 2, -2), the factor its
        scan is to be seen through (float32[N]: ``safe.scan_scale`` in mode 2, else 1) and the PID command (float32[N,2]: mode
        1's; zeros elsewhere).  -> ``(mode, scale, pid)``.  A tick is ``plan`` -> one forward with ``scan_scale=scale``
        (``CNNPolicy.act_fused``) -> ``hybrid_commit`` -> ``step``.  One launch on the current stream, nothing synchronises,
        nothing of the env is written.  ``params``: a ``hybrid.HybridParams``, ``safe``: a ``hybrid.SafePolicyParams`` (default:
        the library's); ``mask``: a uint8[N] tensor, rows with 0 keep what the outputs hold (fresh outputs start as mode 0,
        scale 1, pid 0); ``clear``: a float32[N,3] tensor that takes (d_min, d_front, d_block); ``goal``: a float32[N,2] tensor in
        the robots' frames that stands where ``env.local_goal`` would (mrca_hybrid_plan_goal), as for ``dwa_actions``."""
        if mode is None:
            mode = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        if scale is None:
            scale = torch.ones(self.N, dtype=torch.float32, device=self.device)
        if pid is None:
            pid = torch.zeros((self.N, 2), dtype=torch.float32, device=self.device)
        st = None if params is None else params.struct()
        ss = None if safe is None else safe.struct()
        args = (self._h, None if st is None else C.byref(st), None if ss is None else C.byref(ss), self._ptr(mask, torch.uint8, self.N),
                self._ptr(mode, torch.int32, self.N), self._ptr(scale, torch.float32, self.N), self._ptr(pid, torch.float32, 2 * self.N),
                self._ptr(clear, torch.float32, 3 * self.N))
        if goal is None:
            _lib.check(self.lib.mrca_hybrid_plan(*args, self._stream()), "mrca_hybrid_plan")
        else:
            _lib.check(self.lib.mrca_hybrid_plan_goal(*args, self._ptr(goal, torch.float32, 2 * self.N), self._stream()),
                       "mrca_hybrid_plan_goal")
        return mode, scale, pid

    def hybrid_commit(self, actions, mode, pid, safe=None, mask=None, out=None):
        """The second half (mrca_hybrid_commit): ``actions`` (float32[N,2], what the forward with the plan's scan scale gave)
        kept in mode 0, replaced by ``pid`` in modes 1 and -2, capped in v at ``safe.v_cap`` in mode 2 (omega kept).
        ``out=None`` works IN PLACE on ``actions`` and returns it; ``mask``: rows with 0 keep what ``out`` holds.  One launch on
        the current stream."""
        if out is None:
            out = actions
        ss = None if safe is None else safe.struct()
        _lib.check(self.lib.mrca_hybrid_commit(self.N, None if ss is None else C.byref(ss), self._ptr(mask, torch.uint8, self.N),
                                               self._ptr(mode, torch.int32, self.N), self._ptr(pid, torch.float32, 2 * self.N),
                                               self._ptr(actions, torch.float32, 2 * self.N), self._ptr(out, torch.float32, 2 * self.N),
                                               self._stream()), "mrca_hybrid_commit")
        return out

    def plan_goals(self, goals=None, params=None):
        """The planning call of the global planner (mrca_goal_fields): one integer field of shortest-path lengths over the
        coarsened map per goal point -> a ``planner.GoalFields``.  ``goals``: a float32[G,2] tensor of goal points; every robot
        then walks to goal ``n % G`` (set ``fields.slot`` for another assignment; -1: none).  Default: the distinct rows of
        ``env.goal`` as they stand, one slot per robot.  ``params``: a ``planner.PlannerParams`` (default: the library's).
        SYNCHRONISES the current stream while it looks for convergence; not capturable.  Plan again when the goals change."""
        from .planner import GoalFields, PlannerParams
        params = params if params is not None else PlannerParams()
        if goals is None:
            goals, slot = torch.unique(self.goal, dim=0, return_inverse=True)
            goals, slot = goals.contiguous(), slot.to(torch.int32).contiguous()
        else:
            goals = torch.as_tensor(goals, dtype=torch.float32, device=self.device).reshape(-1, 2).contiguous()
            slot = (torch.arange(self.N, device=self.device) % goals.shape[0]).to(torch.int32)
        G = int(goals.shape[0])
        st = params.struct()
        pw, ph = C.c_int32(), C.c_int32()
        _lib.check(self.lib.mrca_planner_grid(self._h, C.byref(st), C.byref(pw), C.byref(ph)), "mrca_planner_grid")
        field = torch.empty((G, ph.value, pw.value), dtype=torch.int32, device=self.device)
        rounds = C.c_int32()
        _lib.check(self.lib.mrca_goal_fields(self._h, C.byref(st), self._ptr(goals, torch.float32, 2 * G), G,
                                             C.c_void_p(field.data_ptr()), C.byref(rounds), self._stream()), "mrca_goal_fields")
        return GoalFields(field, goals, slot, params, rounds.value)

    def subgoals(self, fields, mask=None, out=None):
        """The per-tick call (mrca_subgoals): every robot's subgoal a few steps down its slot's field ->
        ``(local, subgoal, dist, status)``: the subgoal in the robot's frame (float32[N,2]: hand it to the controller in place
        of ``env.local_goal``), in the world (float32[N,2]), the path length from where the robot stands in metres (float32[N],
        inf: none) and int32[N] 1 (the goal itself) / 0 (a cell centre on the path) / -1 (no slot) / -2 (no path: the goal
        itself).  One launch on the current stream, nothing synchronises, nothing of the env is written.  ``out``: the four
        tensors to write into; ``mask``: a uint8[N] tensor, rows with 0 keep what ``out`` holds."""
        if out is None:
            out = (torch.zeros((self.N, 2), dtype=torch.float32, device=self.device),
                   torch.zeros((self.N, 2), dtype=torch.float32, device=self.device),
                   torch.zeros(self.N, dtype=torch.float32, device=self.device),
                   torch.zeros(self.N, dtype=torch.int32, device=self.device))
        local, subgoal, dist, status = out
        G = fields.num_goals
        st = fields.params.struct()
        _lib.check(self.lib.mrca_subgoals(self._h, C.byref(st), C.c_void_p(fields.field.data_ptr()),
                                          self._ptr(fields.goals, torch.float32, 2 * G), G, self._ptr(fields.slot, torch.int32, self.N),
                                          self._ptr(mask, torch.uint8, self.N), self._ptr(local, torch.float32, 2 * self.N),
                                          self._ptr(subgoal, torch.float32, 2 * self.N), self._ptr(dist, torch.float32, self.N),
                                          self._ptr(status, torch.int32, self.N), self._stream()), "mrca_subgoals")
        return local, subgoal, dist, status

    def subgoals_los(self, fields, los=None, mask=None, out=None):
        """The per-tick call with line of sight (mrca_subgoals_los): as ``subgoals``, but the subgoal is the farthest cell of the
        path, up to ``los.reach`` steps down it, that the robot's planning cell sees (never nearer than ``subgoals``' own) ->
        ``(local, subgoal, dist, status, ahead)``; ``ahead`` int32[N,2] = (m, m_vis): how many steps down the path the subgoal
        lies and the farthest visible one (0, 0: no walk).  ``los``: a ``planner.LosParams`` (default: the library's, reach
        60); ``out``: the five tensors to write into; ``mask``: a uint8[N] tensor, rows with 0 keep what ``out`` holds.  One
        launch on the current stream, nothing synchronises, nothing of the env is written."""
        if out is None:
            out = (torch.zeros((self.N, 2), dtype=torch.float32, device=self.device),
                   torch.zeros((self.N, 2), dtype=torch.float32, device=self.device),
                   torch.zeros(self.N, dtype=torch.float32, device=self.device),
                   torch.zeros(self.N, dtype=torch.int32, device=self.device),
                   torch.zeros((self.N, 2), dtype=torch.int32, device=self.device))
        local, subgoal, dist, status, ahead = out
        G = fields.num_goals
        st = fields.params.struct()
        ls = None if los is None else los.struct()
        _lib.check(self.lib.mrca_subgoals_los(self._h, C.byref(st), None if ls is None else C.byref(ls),
                                              C.c_void_p(fields.field.data_ptr()), self._ptr(fields.goals, torch.float32, 2 * G), G,
                                              self._ptr(fields.slot, torch.int32, self.N), self._ptr(mask, torch.uint8, self.N),
                                              self._ptr(local, torch.float32, 2 * self.N), self._ptr(subgoal, torch.float32, 2 * self.N),
                                              self._ptr(dist, torch.float32, self.N), self._ptr(status, torch.int32, self.N),
                                              self._ptr(ahead, torch.int32, 2 * self.N), self._stream()), "mrca_subgoals_los")
        return local, subgoal, dist, status, ahead

    def scan_noise(self, params=None, mask=None):
        """The lidar noise model (mrca_scan_noise) applied IN PLACE to the newest scan row of every robot (``mask``: a uint8[N]
        tensor, rows with 0 are not touched): range noise, quantisation and dropout as ``params`` (a ``noise.ScanNoiseParams``;
        default: the library's) say, drawn per (seed, robot, episode, T, beam).  One launch on the current stream.  NOT
        idempotent: call it ONCE behind each ``reset`` / ``step`` -- or construct the env with ``scan_noise=`` and let it."""
        st = None if params is None else params.struct()
        self._apply_noise(st, self._ptr(mask, torch.uint8, self.N))
        return self

    def _apply_noise(self, st, mask_ptr):
        _lib.check(self.lib.mrca_scan_noise(self._h, None if st is None else C.byref(st), mask_ptr, self._stream()), "mrca_scan_noise")
        self._views_current &= self._eager_views          # (the library keeps its eager views in step; the lazy ones are stale)

    def _noise_range(self, first, count):
        """the env's own noise behind a cast of robots [first, first + count)"""
        if (first, count) == (0, self.N):
            return self._apply_noise(self._scan_noise, None)
        m = self._noise_masks.get((first, count))
        if m is None:
            m = self._noise_masks[(first, count)] = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
            m[first:first + count] = 1
        self._apply_noise(self._scan_noise, C.c_void_p(m.data_ptr()))

    def scatter(self, boxes=None, params=None, out=None):
        """The scenario sampler (mrca_scatter): per world a different set of starts and goals, each robot's drawn in its own
        start / goal box (``boxes``: [R,8] per local index, default ``scenario.boxes``), clear of the map and apart from the
        robots placed before it -- reproducible bit for bit from (seed, ``params.draw``).  -> ``(poses, goals, tries)``:
        float32[N,3], float32[N,2] and int32[N,2] tensors on the env's device (``out``: such a triple to write into), what
        ``reset(None, poses, goals)`` takes; ``tries`` holds the candidates used per start and goal, -1 where none of
        ``max_tries`` qualified (the robot then stands on its last candidate).  ``params``: a ``scatter.ScatterParams`` (default:
        the scenario's ``scatter`` overrides on the library's defaults).  One launch on the current stream, nothing
        synchronises, nothing of the env is written; valid before the first ``reset``."""
        from .scatter import ScatterParams, check_boxes
        if boxes is None:
            boxes = self.scenario.boxes
        if boxes is None:
            raise ValueError("scatter: the scenario has no boxes and none were given")
        b = check_boxes(boxes, self.R)
        key = b.tobytes()
        if self._scatter_boxes is None or self._scatter_boxes[0] != key:      # the uploaded boxes are kept: a capture can replay them
            self._scatter_boxes = (key, torch.from_numpy(b).to(self.device))
        if params is None:
            params = ScatterParams(**(self.scenario.scatter or {}))
        st = params.struct()
        if out is None:
            out = (torch.zeros((self.N, 3), dtype=torch.float32, device=self.device),
                   torch.zeros((self.N, 2), dtype=torch.float32, device=self.device),
                   torch.zeros((self.N, 2), dtype=torch.int32, device=self.device))
        poses, goals, tries = out
        _lib.check(self.lib.mrca_scatter(self._h, C.byref(st), C.c_void_p(self._scatter_boxes[1].data_ptr()),
                                         self._ptr(poses, torch.float32, 3 * self.N), self._ptr(goals, torch.float32, 2 * self.N),
                                         self._ptr(tries, torch.int32, 2 * self.N), self._stream()), "mrca_scatter")
        return poses, goals, tries

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            self.lib.mrca_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ptr(t, dtype, numel):
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"expected a contiguous cuda {dtype} tensor with {numel} elements")
        return C.c_void_p(t.data_ptr())

    # ------------------------------------------------------------------ the StageWorld surface, batched
    def reset(self, mask=None, poses=None, goals=None):
        """reset_pose + generate_goal_point (+ first observation) for the masked robots
        (stage_world1.py:171-177,213-223; ppo_stage1.py:52-62)."""
        _lib.check(self.lib.mrca_reset(self._h, self._ptr(mask, torch.uint8, self.N),
                                       self._ptr(poses, torch.float32, self.N * 3),
                                       self._ptr(goals, torch.float32, self.N * 2), self._stream()), "mrca_reset")
        self._views_current = self._eager_views
        if self._scan_noise is not None:
            self._apply_noise(self._scan_noise, self._ptr(mask, torch.uint8, self.N))
        return self

    def step(self, actions, ray_slice=None, worlds=None):
        """control_vel + one Stage tick + get_reward_and_terminate + next observation for every
        robot (ppo_stage1.py:75-91).  ``actions`` f32[N,2] = clipped (v, omega).
        ``ray_slice=(first, count)``: one world sharded over ranks (mrca_step_slice) -- all robots advance, the
        lidar is cast for robots [first, first + count) only.
        ``worlds=(first, count)``: only these worlds tick (mrca_step_worlds), on the current stream; disjoint ranges may be
        stepped on different streams at the same time (worlds never interact)."""
        a = self._ptr(actions, torch.float32, self.N * 2)
        if worlds is not None:
            if ray_slice is not None:
                raise ValueError("step: ray_slice and worlds exclude each other")
            _lib.check(self.lib.mrca_step_worlds(self._h, a, int(worlds[0]), int(worlds[1]), self._stream()),
                       "mrca_step_worlds")
            self._views_current = 0       # (lazy_obs=False re-formed the views of this range only)
            cast = (int(worlds[0]) * self.R, int(worlds[1]) * self.R)
        elif ray_slice is None:
            _lib.check(self.lib.mrca_step(self._h, a, self._stream()), "mrca_step")
            self._views_current = self._eager_views
            cast = (0, self.N)
        else:
            _lib.check(self.lib.mrca_step_slice(self._h, a, int(ray_slice[0]), int(ray_slice[1]), self._stream()),
                       "mrca_step_slice")
            self._views_current = 0
            cast = (int(ray_slice[0]), int(ray_slice[1]))
        if self._scan_noise is not None:
            self._noise_range(*cast)
        return self

    def move(self, actions, worlds):
        """First launch of ``step(actions, worlds=...)``: control_vel, the Stage tick, reward / terminal and episode
        bookkeeping of the worlds (first, count) (mrca_move_worlds).  ``observe`` must follow before the next ``move``."""
        _lib.check(self.lib.mrca_move_worlds(self._h, self._ptr(actions, torch.float32, self.N * 2), int(worlds[0]),
                                             int(worlds[1]), self._stream()), "mrca_move_worlds")
        self._views_current = 0
        return self

    def observe(self, worlds):
        """Second launch: the lidar scans and local goals of the worlds (first, count) at their current poses
        (mrca_observe_worlds)."""
        _lib.check(self.lib.mrca_observe_worlds(self._h, int(worlds[0]), int(worlds[1]), self._stream()),
                   "mrca_observe_worlds")
        self._views_current = 0
        if self._scan_noise is not None:
            self._noise_range(int(worlds[0]) * self.R, int(worlds[1]) * self.R)
        return self

    def step_many(self, actions, first_tick, num_ticks, chains=1):
        """``num_ticks`` ticks from ONE call: tick k takes ``actions[(first_tick + k) % len(actions)]`` (a list of f32[N,2]
        device tensors: a scripted scenario, the benchmark's action pool).  Equal to ``num_ticks`` calls of ``step``.
        ``chains`` = P > 0: the library's run-ahead schedule -- the move launches on a stream of the env's own, ahead of the ray
        casts of P world ranges on P streams (mrca_step_many); ``chains`` = -P: round 5's P chains half a tick
        apart.  The first call on a stream spends ~1 ms warming and checking the env's streams (and synchronises once)."""
        if self._scan_noise is not None:
            raise ValueError("step_many: this env was constructed with scan_noise, and mrca_step_many casts the rays of several "
                             "ticks per call -- the noise model is applied once per cast (mrca_scan_noise); use step")
        # (the pointer table of a list is built once per list object: a 20-tick region is 0.6 ms, sixteen data_ptr() calls and
        # their checks are 2 % of it.  The entry keeps the tensors themselves: an element replaced in place -- pool[i] = t --
        # fails the identity compare below and rebuilds the table, and a table never outlives the memory it points at)
        cache = self.__dict__.setdefault("_many_ptrs", {})
        entry = cache.get(id(actions))
        if entry is None or entry[0] is not actions or len(actions) != entry[2] or \
                not all(map(operator.is_, actions, entry[3])):
            ptrs = [self._ptr(t, torch.float32, self.N * 2).value for t in actions]
            cache.clear()
            entry = cache[id(actions)] = (actions, (C.c_void_p * len(actions))(*ptrs), len(actions), tuple(actions))
        rc = self.lib.mrca_step_many(self._h, entry[1], entry[2], int(first_tick), int(num_ticks), int(chains), self._stream())
        if rc:
            _lib.check(rc, "mrca_step_many")
        self._views_current = self._eager_views if chains <= 1 else 0
        return self

    def ring_ranges(self):
        """f32[N,F,B]: a copy of the scan ring.  (ABI 4-5 kept what a beam hit in the sign bit of its ring entry and this
        accessor stripped it; since ABI 6 the flag is ``hit_bits`` / ``hit_robot`` and the ring holds plain ranges -- kept
        for the callers written against it.)"""
        return self.scan_ring.abs()

    def check(self):
        """Host round trip: raises if a kernel flagged a device-side failure since the last check (mrca_check)."""
        _lib.check(self.lib.mrca_check(self._h, self._stream()), "mrca_check")

    # ------------------------------------------------------------------ timing (bench / profiles)
    def enable_timing(self, on=True):
        _lib.check(self.lib.mrca_enable_timing(self._h, int(on)), "mrca_enable_timing")

    def set_debug_flags(self, flags):
        """Profiling build only (MRCA_ENV_LIB=.../libmrca_env_prof.so, include/mrca_env.h): ablation switches and
        launch-shape knobs of the kernels.  The product library does not have them."""
        if not hasattr(self.lib, "mrca_set_debug_flags"):
            raise RuntimeError("this is the product build of libmrca_env.so: ablation switches exist only in the "
                               "profiling build (csrc/build.sh --profiling, MRCA_ENV_LIB=...)")
        _lib.check(self.lib.mrca_set_debug_flags(self._h, int(flags)), "mrca_set_debug_flags")

    def event_pair_overhead(self, samples=200):
        """us an empty HIP-event pair reads on the current stream: contained once per kernel in ``read_timing``'s figures."""
        us = C.c_float()
        _lib.check(self.lib.mrca_event_pair_overhead(self._stream(), int(samples), C.byref(us)), "mrca_event_pair_overhead")
        return us.value

    def read_timing(self):
        mv, ry, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self.lib.mrca_read_timing(self._h, C.byref(mv), C.byref(ry), C.byref(n)), "mrca_read_timing")
        return mv.value, ry.value, n.value


def gae(rewards, values, last_value, dones, gamma, lam):
    """generate_train_data (model/ppo.py:122-139) on device: rewards/values f32[T,N], last_value
    f32[N], dones u8[T,N] -> (targets, advs) f32[T,N]."""
    lib = _lib.load()
    T, N = rewards.shape
    for t, dt in ((rewards, torch.float32), (values, torch.float32), (last_value, torch.float32),
                  (dones, torch.uint8)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dt):
            raise ValueError("gae: expected contiguous cuda tensors (f32, f32, f32, u8)")
    targets = torch.empty_like(rewards)
    advs = torch.empty_like(rewards)
    stream = C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream)
    _lib.check(lib.mrca_gae(rewards.data_ptr(), values.data_ptr(), last_value.data_ptr(), dones.data_ptr(),
                            float(gamma), float(lam), T, N, targets.data_ptr(), advs.data_ptr(), stream), "mrca_gae")
    return targets, advs
