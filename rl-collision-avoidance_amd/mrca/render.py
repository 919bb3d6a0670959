"""What to do with the pictures ``VecStageWorld.render`` makes: tile views into one sheet, record frames of a run on the
device, write them out.  The reference's users watch Stage's GUI window (``stageros`` without ``-g``) and its ``doc/*.gif``
are captures of it; this is the ROS-free view of the same worlds.  Nothing here computes a pixel: that is mrca_render.
"""
import os

import numpy as np
import torch


def contact_sheet(frames, cols):
    """[V,H,W,3] (or [T,V,H,W,3]) -> [rows * H, cols * W, 3] (or [T, ...]): the V views tiled row-major, ``cols`` to a row,
    missing tiles white.  Works on torch tensors (stays on their device) and NumPy arrays alike."""
    is_torch = torch.is_tensor(frames)
    lead = frames.shape[:-4]
    V, H, W, C = frames.shape[-4:]
    cols = max(1, min(int(cols), V))
    rows = (V + cols - 1) // cols
    if rows * cols != V:
        pad_shape = (*lead, rows * cols - V, H, W, C)
        pad = frames.new_full(pad_shape, 255) if is_torch else np.full(pad_shape, 255, frames.dtype)
        frames = torch.cat([frames, pad], dim=-4) if is_torch else np.concatenate([frames, pad], axis=-4)
    x = frames.reshape(*lead, rows, cols, H, W, C)
    n = len(lead)
    order = (*range(n), n, n + 2, n + 1, n + 3, n + 4)
    x = x.permute(*order) if is_torch else x.transpose(order)
    return x.reshape(*lead, rows * H, cols * W, C)


def save_frames(frames, path):
    """Writes uint8 frames [T,H,W,3] (host array or tensor) and returns the file's path: an animated GIF ``path`` (+ ``.gif``
    unless it names one) when PIL is importable, otherwise the stack as ``path`` + ``.npz`` (key ``frames``).  Never fails for
    lack of PIL."""
    if torch.is_tensor(frames):
        frames = frames.cpu().numpy()
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"save_frames: expected uint8 frames [T,H,W,3], got {frames.shape}")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    root, ext = os.path.splitext(path)
    if Image is None:
        out = (root if ext.lower() in (".gif", ".npz") else path) + ".npz"
        np.savez_compressed(out, frames=frames)
        return out
    out = path if ext.lower() == ".gif" else path + ".gif"
    imgs = [Image.fromarray(f) for f in frames]
    imgs[0].save(out, save_all=True, append_images=imgs[1:], duration=100, loop=0)
    return out


class Recorder:
    """Frames of a run, gathered on the device: ``tick(k)`` renders ``worlds`` every ``every``-th tick (with trails) into a
    tensor of its own on the env's current stream -- no synchronisation, nothing of the env written -- and ``frames()``
    copies them to the host ONCE, as contact sheets [T, rows * size, cols * size, 3]."""

    def __init__(self, env, worlds=None, every=10, size=256, layers=None):
        self.env, self.every, self.size = env, max(1, int(every)), int(size)
        self.worlds = list(range(min(env.W, 16))) if worlds is None else [int(w) for w in worlds]
        self.kw = {} if layers is None else {"layers": layers}
        self.trail = torch.zeros(len(self.worlds), self.size, self.size, dtype=torch.int32, device=env.device)
        self.shots = []

    def tick(self, k):
        if k % self.every == 0:
            self.shots.append(self.env.render(self.worlds, (self.size, self.size), trail=self.trail, **self.kw))

    def frames(self):
        if not self.shots:
            return np.zeros((0, self.size, self.size, 3), np.uint8)
        cols = int(np.ceil(np.sqrt(len(self.worlds))))
        return contact_sheet(torch.stack(self.shots), cols).cpu().numpy()
