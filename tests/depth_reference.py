"""Float64 (or float32) PyTorch transliteration of the depth march, DESIGN.md D18: ray-depth moments and all their gradients.

A composition, like rgba_reference.py + rgba_pose_reference.py; nothing of a backward is written here. The sample loop of
tests/golden/make_autograd_golden.py (`march`: positions, sample count, max_samples clip, early termination at A >= 0.99,
front-to-back compositing), its trilinear tap and table lookup and its per-view driver (`render_view`) are imported, with a
sample that classifies by the table's alpha alone and composites, beside its opacity, the distance of its position from the
camera along the ray and that distance squared. The free camera's ray setup, per-ray leaves and driver are
tests/pose_reference.run_march. torch.autograd differentiates the programs, with their branch predicates frozen. The fov leaf is
in RADIANS, as the C ABI's column 9 is.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import make_autograd_golden as G  # noqa: E402
import pose_reference as PR  # noqa: E402


def raycast_depth(vol, tf, cam, entry, exit_, rays, n, max_samples, sampling_rate):
    """All pixels of one view at once; cam (3,) or one row per ray (P, 3). Returns the moments (P, 4) = (M1, M2, 0, A) and the
    live-sample counts."""
    def sample(pos):
        alpha = G.apply_transfer_function(tf, G.sample_volume_trilinear(vol, pos))[:, 3]
        op = 1.0 - torch.pow(1.0 - alpha, 1.0 / sampling_rate)
        t = ((pos - cam) * rays).sum(1)
        return torch.stack([op * t, op * t * t, torch.zeros_like(op), op], dim=1), alpha, {}

    out, _, count, _ = G.march(cam, entry, exit_, rays, n, max_samples, False, sample)
    return out, count


def run(vol, tf, cam, entry, exit_, rays, n, grad_out, max_samples, sampling_rate, dtype=torch.float64, want_grad=True,
        pixels=None):
    """The transliteration over views. vol (VX,VY,VZ) or (V,VX,VY,VZ), tf (R,4) or (V,R,4), cam (V,3), ray buffers (V,W,H[,3])
    and grad_out (V,W,H,4): numpy arrays (the GPU's ray buffers, copied). Rays with n <= 1 are not marched (pixel 0, H6) and
    `pixels` (a (V,W,H) mask) restricts the march further. Returns "moments" (V,W,H,4), "steps" and, with want_grad, "dvol" and
    "dtf" (the gradients of sum(moments * grad_out)) as float64 numpy arrays in the shapes of the inputs."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    V, W, H = n.shape
    volt, tft = T(vol).requires_grad_(want_grad), T(tf).requires_grad_(want_grad)
    views, total = [], 0.0
    for v in range(V):
        def march_rays(sel):
            out, cnt = raycast_depth(volt[v] if volt.ndim == 4 else volt, tft[v] if tft.ndim == 3 else tft, T(cam[v]),
                                     T(entry[v]).reshape(-1)[sel], T(exit_[v]).reshape(-1)[sel], T(rays[v]).reshape(-1, 3)[sel],
                                     torch.from_numpy(n[v].astype(np.int64)).reshape(-1)[sel], int(max_samples),
                                     float(sampling_rate))
            return out, dict(steps=cnt.int())

        loss, res = G.render_view((W, H), n[v], None if pixels is None else pixels[v], T(grad_out[v]).reshape(-1, 4), march_rays)
        total = total + loss
        views.append(res)
    res = {"moments": np.stack([r["rgba"] for r in views]), "steps": np.stack([r["steps"] for r in views])}
    if want_grad:
        if torch.is_tensor(total):
            total.backward()
        res["dvol"], res["dtf"] = G.grad_or_zero(volt), G.grad_or_zero(tft)
    return res


def run_case(inp, dtype=torch.float64, pixels=None):
    """pose_reference.run_case for the depth march: entry, exit, rays, n, steps, rgba (the moments), dpose_ray (W,H,10), dpose;
    the forward in `dtype`. inp: vol, tf, look_from, grad_out (W,H,4), sr, max_samples, jitter_seed, view; optional look_at, up,
    fov_rad."""
    return PR.run_march(inp, dtype, pixels, lambda T, cam, e, x, r, n: raycast_depth(
        T(inp["vol"]), T(inp["tf"]), cam, e, x, r, n, int(inp["max_samples"]), float(inp["sr"])))
