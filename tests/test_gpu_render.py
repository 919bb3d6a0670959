"""GPU: mrca_render -- the ID image, the trail and the RGB picture EQUAL to the NumPy float32 gather reference of
tests/render_ref.py (small worlds, a big world, fidelity mode); beam ends against fp64 endpoints; the call reads the env and
writes nothing of it; the map layer and the robot markers against Stage's own GUI picture of stage2.world
(tests/golden/stage_gui_stage2.npz); ``mrca.evaluate --render``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as RR
import util as U
from test_golden_gui import PX_TOL, _clean_zone, _render, gui  # noqa: F401  (gui: the golden picture's fixture)
from util import S

pytestmark = pytest.mark.gpu

SIZES = [(70, 45), (64, 64)]
SCALES = [1.0 / 16.0, 0.05, 0.3, 2.0]
ALL = RR.MAP | RR.GOALS | RR.BODIES


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.build()
    from mrca import vec_env
    return vec_env


def small_scenario(**kw):
    """3 worlds x 7 robots on a 40 x 40-cell map (0.5 m cells, walled, two blocks)."""
    occ = np.zeros((40, 40), bool)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = True
    occ[8:11, 25:33] = occ[28:34, 6:8] = True
    return S.stage1(num_worlds=3, robots_per_world=7, seed=4, grid=S.GridData.from_dense(occ, 0.5, -10.0, -10.0), **kw)


def teleported(env, rng):
    """A reset that puts robots 1 and 2 of every world on ONE spot (different headings: the priority rule decides every
    pixel they share), robot 3 half over robot 0, and robot 4's goal under robot 0."""
    R = env.R
    poses = np.zeros((env.W, R, 3), np.float32)
    poses[..., :2] = rng.uniform(-7.0, 7.0, (env.W, R, 2))
    poses[..., 2] = rng.uniform(-np.pi, np.pi, (env.W, R))
    poses[:, 2, :2] = poses[:, 1, :2]
    poses[:, 3, :2] = poses[:, 0, :2] + np.float32(0.2)
    poses[0, 5] = (-8.0, 0.0, np.pi)                  # world 0: robot 5 faces the wall at x = -9.5, robot 6 stands behind it
    poses[0, 6] = (-6.8, 0.3, np.pi)
    goals = rng.uniform(-7.0, 7.0, (env.W, R, 2)).astype(np.float32)
    goals[:, 4] = poses[:, 0, :2]
    env.reset(None, torch.from_numpy(poses.reshape(-1, 3)).cuda(), torch.from_numpy(goals.reshape(-1, 2)).cuda())
    return env


def host_state(env):
    torch.cuda.synchronize()
    pose = env.pose.cpu().numpy().reshape(env.W, env.R, 3)
    s, c = U.O.sincos(pose[..., 2], np.float32)           # the head record: sincos_det of the stored heading
    st = {k: getattr(env, k).cpu().numpy().reshape(env.W, env.R) for k in ("crashed", "first_result", "live")}
    return pose, np.stack([s, c], -1), env.goal.cpu().numpy().reshape(env.W, env.R, 2), st


def check_equal(env, worlds, views, W, H, layers=ALL, trail=None, trail_ref=None):
    """One render of ``views`` (cx, cy, m) of ``worlds``: ids, trail and rgb equal to the gather reference."""
    cen = np.array([v[:2] for v in views], np.float64)
    mpp = np.array([v[2] for v in views], np.float64)
    rgb = env.render(worlds, (W, H), cen, mpp, layers=layers, trail=trail)
    pose, sincos, goals, st = host_state(env)
    ids, rgb = env.render_ids.cpu().numpy().view(np.uint32), rgb.cpu().numpy()
    tr = None if trail is None else trail.cpu().numpy().view(np.uint32)
    for v, (w, view) in enumerate(zip(worlds, views)):
        want = RR.gather_ids(view, W, H, layers, env.scenario.grid, pose[w, :, :2], sincos[w], goals[w])
        assert np.array_equal(ids[v], want), (w, view, (W, H), np.argwhere(ids[v] != want)[:5])
        if tr is not None:
            assert np.array_equal(tr[v], trail_ref[v]), (w, view)
        want_rgb = RR.resolve(want, None if tr is None else trail_ref[v], st["crashed"][w], st["first_result"][w], st["live"][w])
        assert np.array_equal(rgb[v], want_rgb), (w, view, np.argwhere(rgb[v] != want_rgb)[:5])
    return ids


def view_kinds(env, m, W, H):
    """Per world: the map's centre, a robot's neighbourhood (half a pixel off its centre), a window partly off the map and
    one wholly off it."""
    pose = env.pose.cpu().numpy().reshape(env.W, env.R, 3)
    worlds, views = [], []
    for w in range(env.W):
        for cx, cy in [(0.0, 0.0), (pose[w, 1, 0] + 0.5 * m, pose[w, 1, 1] - 0.25 * m), (pose[w, 0, 0], pose[w, 0, 1]),
                       (10.0 - 0.2 * W * m, -10.0 + 0.1 * H * m), (200.0, -150.0)]:
            worlds.append(w)
            views.append((cx, cy, m))
    return worlds, views


@pytest.fixture(scope="module")
def small_env(hip):
    env = teleported(hip.VecStageWorld(small_scenario()), np.random.default_rng(2))
    yield env
    env.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("m", SCALES)
def test_ids_and_rgb_equal_the_gather_reference(small_env, size, m):
    W, H = size
    worlds, views = view_kinds(small_env, m, W, H)
    ids = check_equal(small_env, worlds, views, W, H)
    layers = set(np.unique(ids >> 24).tolist())
    assert layers >= {0, RR.L_MAP, RR.L_GOAL, RR.L_BODY}, layers
    for layers in (RR.MAP, RR.GOALS, RR.BODIES, 0):
        check_equal(small_env, worlds[:5], views[:5], W, H, layers=layers)


def test_same_state_twice_is_bit_identical(small_env):
    worlds, views = view_kinds(small_env, 0.05, 70, 45)
    cen, mpp = np.array([v[:2] for v in views]), np.array([v[2] for v in views])
    a = small_env.render(worlds, (70, 45), cen, mpp, layers=ALL | RR.BEAMS).clone()
    ids = small_env.render_ids.clone()
    b = small_env.render(worlds, (70, 45), cen, mpp, layers=ALL | RR.BEAMS)
    assert torch.equal(a, b) and torch.equal(ids, small_env.render_ids)


def test_trail_after_five_ticks(hip):
    env = teleported(hip.VecStageWorld(small_scenario()), np.random.default_rng(3))
    W, H = 70, 45
    worlds, views = [0, 1, 2, 0], [(0.0, 0.0, 0.3), (0.0, 0.0, 0.3), (1.0, -2.0, 0.05), (0.0, 0.0, 2.0)]
    trail = torch.zeros(len(views), H, W, dtype=torch.int32, device=env.device)
    ref = [None] * len(views)
    rng = np.random.default_rng(0)
    for k in range(6):
        pose = env.pose.cpu().numpy().reshape(env.W, env.R, 3)
        ref = [RR.trail_marks(view, W, H, pose[w, :, :2], ref[v]) for v, (w, view) in enumerate(zip(worlds, views))]
        check_equal(env, worlds, views, W, H, trail=trail, trail_ref=ref)
        if k < 5:
            env.step(torch.from_numpy(U.random_actions(rng, env.N)).cuda())
    assert all((r != 0).sum() > env.R for r in ref[:2])           # robots moved: more marks than robots
    env.close()


def test_big_world_and_fidelity_mode(hip):
    """One world of 80 robots in the open (robots_per_world > 64: the big-world path), and a fidelity-mode env."""
    env = hip.VecStageWorld(S.circle_big(80)).reset()
    cx, cy, m = env.default_view((64, 64))
    assert (cx, cy) == (0.0, 0.0) and abs(m * 64 - 2 * (env.scenario.init_table[:, 0].max() + 1.0)) < 1e-9
    p = env.pose.cpu().numpy()
    for W, H in SIZES:
        views = [(cx, cy, max(m * 64 / W, m * 64 / H)), (p[0, 0], p[0, 1], 0.05), (p[40, 0] + 1.0, p[40, 1], 0.3), (0.0, 0.0, 2.0)]
        ids = check_equal(env, [0] * len(views), views, W, H)
        # the zoomed-out view shows every robot although each is a fraction of a pixel
        assert ((ids[0] >> 24) >= RR.L_BODY).sum() >= 70
    env.close()
    env = hip.VecStageWorld(S.stage1(num_worlds=2, robots_per_world=6, seed=3, stage_resolution=True)).reset()
    check_equal(env, [0, 1], [env.default_view((64, 64))] * 2, 64, 64)
    env.close()


def test_beam_ends(small_env):
    """Every marked pixel within 1 pixel (Chebyshev) of an fp64 endpoint of its kind formed from the env's pose and newest
    scan, and every such endpoint inside the image within 1 pixel of a mark; wall and robot returns both present."""
    env = small_env
    torch.cuda.synchronize()
    R, B = env.R, env.B
    pose = env.pose.cpu().numpy().astype(np.float64)[:R]
    head = env.ring_head.cpu().numpy()[:R]
    rng_ = env.scan_ring.cpu().numpy()[np.arange(R), head].astype(np.float64)
    hit = env.hit_robot.cpu().numpy()[:R]
    bearing = -U.O.FOV / 2.0 + np.arange(B) * (U.O.FOV / (B - 1))
    ang = pose[:, 2:3] + bearing[None]
    ex, ey = pose[:, 0:1] + rng_ * np.cos(ang), pose[:, 1:2] + rng_ * np.sin(ang)
    ret = rng_ < 6.0
    assert (ret & hit).any() and (ret & ~hit).any(), "the scene needs wall returns and robot returns"
    for (W, H), view in [((70, 45), (-7.0, 0.0, 0.1)), ((64, 64), (-6.0, 1.0, 0.3))]:
        env.render([0], (W, H), view[:2], view[2], layers=RR.BEAMS)
        ids = env.render_ids.cpu().numpy().view(np.uint32)[0]
        assert set(np.unique(ids >> 24).tolist()) == {0, RR.L_BEAM_WALL, RR.L_BEAM_ROBOT}
        fc = np.floor((ex - (view[0] - 0.5 * W * view[2])) / view[2])
        fr = np.floor(((view[1] + 0.5 * H * view[2]) - ey) / view[2])
        for layer, kind in ((RR.L_BEAM_ROBOT, ret & hit), (RR.L_BEAM_WALL, ret & ~hit)):
            ends = np.zeros((H + 2, W + 2), bool)                   # fp64 endpoints' pixels, one pixel of border
            ok = kind & (fc >= -1) & (fc <= W) & (fr >= -1) & (fr <= H)
            ends[fr[ok].astype(int) + 1, fc[ok].astype(int) + 1] = True
            near = np.zeros((H, W), bool)                           # within 1 pixel of such an endpoint
            for dr in range(3):
                for dc in range(3):
                    near |= ends[dr:dr + H, dc:dc + W]
            marked = (ids >> 24) == layer
            assert marked.any() and not (marked & ~near).any(), (layer, np.argwhere(marked & ~near)[:5])
        marks = np.pad((ids >> 24) >= RR.L_BEAM_WALL, 1)
        near_mark = np.zeros((H, W), bool)
        for dr in range(3):
            for dc in range(3):
                near_mark |= marks[dr:dr + H, dc:dc + W]
        inside = ret & (fc >= 1) & (fc <= W - 2) & (fr >= 1) & (fr <= H - 2)       # (a pixel off the border: fp32 may round across it)
        assert inside.sum() > 50 and near_mark[fr[inside].astype(int), fc[inside].astype(int)].all()
        # the index is the beam's owner's: a mark of robot i has an endpoint of robot i within a pixel
        for row, col in np.argwhere((ids >> 24) >= RR.L_BEAM_WALL)[::7]:
            i = int(ids[row, col] & 0xFFFFFF)
            assert (ret[i] & (np.abs(fc[i] - col) <= 1) & (np.abs(fr[i] - row) <= 1)).any()


def test_render_writes_nothing_of_the_env(hip, small_env):
    env = small_env
    from mrca import _lib
    names = ["_" + n if n in ("obs", "scan") else n for n, _, _ in _lib.FIELDS]
    before = {n: getattr(env, n).clone() for n in names}
    arena = env.arena.clone()
    trail = torch.zeros(3, 45, 70, dtype=torch.int32, device=env.device)
    env.render(None, (70, 45), layers=ALL | RR.BEAMS, trail=trail)
    env.render([2, 0], (64, 64), (1.0, 1.0), 0.05)
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(getattr(env, n), before[n]), n
    assert torch.equal(env.arena, arena)


def test_rendered_env_stays_bit_identical_to_an_unrendered_one(hip):
    from mrca import _lib
    a, b = (hip.VecStageWorld(small_scenario()).reset() for _ in range(2))
    trail = torch.zeros(3, 64, 64, dtype=torch.int32, device=a.device)
    rng = np.random.default_rng(7)
    for k in range(20):
        act = torch.from_numpy(U.random_actions(rng, a.N)).cuda()
        a.step(act)
        b.step(act)
        a.render(None, (64, 64), layers=ALL | RR.BEAMS, trail=trail)
        if k % 5 == 4:
            for n, _, _ in _lib.FIELDS:       # (scan / obs through their properties: both envs form the views from their rings)
                assert torch.equal(getattr(a, n), getattr(b, n)), (k, n)
    a.check()
    a.close()
    b.close()


def test_bad_worlds_are_refused(small_env):
    from mrca import _lib
    for w in (-1, 3):
        v = (_lib.RenderView * 1)(_lib.RenderView(w, 0.0, 0.0, 0.1))
        ids = torch.zeros(8, 8, dtype=torch.int32, device=small_env.device)
        assert small_env.lib.mrca_render(small_env._h, v, 1, 8, 8, 7, ids.data_ptr(), None, None, None) == -1
        assert "world" in small_env.lib.mrca_last_error().decode()


# ---------------------------------------------------------------------------------------------- against Stage's GUI
def golden_view(g):
    """The golden picture's viewport as ONE view: the picture's two axis scales differ by 8e-6 (a fit per axis of one
    isotropic scale, test_golden_gui.py), a view has one m_per_px -- their mean.  -> (W, H, view as float32, the same
    viewport as exact numbers in the golden's own terms for ``_render``)."""
    H, W = (int(v) for v in g["wall_shape"])
    m = np.float32(2.0 / (g["sx"] + g["sy"]))
    cx = np.float32((0.5 * W - g["x0"]) * float(m))
    cy = np.float32((g["y0"] - 0.5 * H) * float(m))
    snap = dict(g, sx=1.0 / float(m), sy=1.0 / float(m), x0=0.5 * W - float(cx) / float(m), y0=0.5 * H + float(cy) / float(m))
    return W, H, (float(cx), float(cy), float(m)), snap


@pytest.fixture(scope="module")
def stage2_env(hip):
    env = hip.VecStageWorld(S.stage2()).reset()
    yield env
    env.close()


def test_map_layer_against_the_fp64_sample_and_stages_picture(stage2_env, gui):  # noqa: F811
    env, grid = stage2_env, stage2_env.scenario.grid
    W, H, view, snap = golden_view(gui)
    assert abs(snap["x0"] - gui["x0"]) < 0.01 and abs(snap["y0"] - gui["y0"]) < 0.01     # the same viewport to 1 / 100 pixel
    env.render([0], (W, H), view[:2], view[2], layers=RR.MAP)
    got = (env.render_ids.cpu().numpy().view(np.uint32)[0] >> 24) == RR.L_MAP
    ref = _render(snap, grid)
    # fp32 coordinates may move a pixel centre across a cell boundary only where it lies within 1e-4 m of one
    xs = (np.arange(W) + 0.5 - snap["x0"]) / snap["sx"]
    ys = (snap["y0"] - (np.arange(H) + 0.5)) / snap["sy"]
    fx, fy = (xs - grid.x0) / grid.cell, (ys - grid.y0) / grid.cell
    boundary = (np.abs(fy - np.round(fy)) * grid.cell <= 1e-4)[:, None] | (np.abs(fx - np.round(fx)) * grid.cell <= 1e-4)[None, :]
    diff = got != ref
    print("map layer: pixels differing from the fp64 sample", int(diff.sum()), "of them off a cell boundary", int((diff & ~boundary).sum()),
          "boundary pixels", int(boundary.sum()))
    assert not (diff & ~boundary).any()
    zone = _clean_zone(gui)
    agree_got, agree_ref = int((got == gui["walls"])[zone].sum()), int((ref == gui["walls"])[zone].sum())
    print("agreement with Stage's wall mask in the clean zone:", agree_got / zone.sum(), "fp64 sample:", agree_ref / zone.sum())
    assert agree_got >= agree_ref - int(boundary[zone].sum())
    assert agree_ref / zone.sum() > 0.95


def marker_headings(g, robots):
    """The picture does not say where a robot faces; its marker's bounding box does, up to symmetry: the heading in
    [0, pi / 2] whose 0.44 x 0.38 footprint has the bounding box closest to the marker's (from the golden alone)."""
    bb = g["marker_bbox_px"][0, robots]
    bw, bh = (bb[:, 2] - bb[:, 0]) / g["sx"], (bb[:, 3] - bb[:, 1]) / g["sy"]
    th = np.linspace(0.0, np.pi / 2, 91)
    fw = 0.44 * np.cos(th) + 0.38 * np.sin(th)
    fh = 0.44 * np.sin(th) + 0.38 * np.cos(th)
    return th[np.argmin((fw[None] - bw[:, None]) ** 2 + (fh[None] - bh[:, None]) ** 2, axis=1)]


def test_robot_markers_against_stages_picture(stage2_env, gui):  # noqa: F811
    env = stage2_env
    W, H, view, _ = golden_view(gui)
    robots = gui["robots"]
    assert len(robots) == env.R == 44
    poses = np.zeros((44, 3), np.float32)
    poses[:, :2] = gui["marker_xy_m"][0, robots]
    poses[:, 2] = marker_headings(gui, robots)
    env.reset(None, torch.from_numpy(poses).cuda(), None)
    env.render([0], (W, H), view[:2], view[2], layers=RR.BODIES)
    ids = env.render_ids.cpu().numpy().view(np.uint32)[0]
    checked = 0
    for i, j in enumerate(robots):
        if gui["marker_area_px"][0, j] >= 150:        # the selected robot: Stage draws a highlight box round it (test_robot_footprint)
            continue
        rows, cols = np.nonzero(((ids >> 24) >= RR.L_BODY) & ((ids & 0xFFFFFF) == i))
        assert len(rows), i
        box = np.array([cols.min(), rows.min(), cols.max() + 1, rows.max() + 1], float)
        assert np.abs(box - gui["marker_bbox_px"][0, j]).max() <= PX_TOL + 1, (i, box, gui["marker_bbox_px"][0, j])
        checked += 1
    assert checked >= 43


# ---------------------------------------------------------------------------------------------- the command line
def test_evaluate_render_leaves_the_results_alone(hip, tmp_path):
    cmd = [sys.executable, "-m", "mrca.evaluate", "--circles", "2", "--robots", "8", "--radius", "6", "--max-ticks", "30"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(U.ROOT, "rl-collision-avoidance_amd"), os.environ.get("PYTHONPATH", "")]))
    out = str(tmp_path / "out")
    with_r = subprocess.run(cmd + ["--render", out, "--render-every", "5", "--render-size", "64"], env=env, capture_output=True, text=True,
                            timeout=300)
    assert with_r.returncode == 0, with_r.stderr[-2000:]
    without = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert without.returncode == 0, without.stderr[-2000:]
    assert with_r.stdout == without.stdout and json.loads(without.stdout)["robots"] == 16
    if os.path.exists(out + ".gif"):
        from PIL import Image
        im = Image.open(out + ".gif")
        assert im.n_frames == 6 and im.size == (128, 64)
    else:
        frames = np.load(out + ".npz")["frames"]
        assert frames.shape == (6, 64, 128, 3) and frames.dtype == np.uint8
