"""Float64 (or float32) PyTorch transliteration of the march through a pre-classified RGBA volume, DESIGN.md D14.

The sample loop of tests/golden/make_autograd_golden.py (`march`: positions, sample count, max_samples clip, early termination at
A >= 0.99, front-to-back compositing) and its per-view driver (`render_view`), imported here, not copied, with a sample that
neither classifies nor shades: a sample's (r, g, b, a) is the trilinear interpolation of the volume's four channels, each by that
file's sample_volume_trilinear (one cell, the lerps x -> y -> z), its opacity 1 - (1 - a)^(1 / sampling_rate), and it composites
with L = 1. Nothing of the backward is written here: torch.autograd differentiates the program, with its branch predicates frozen.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_autograd_golden as G  # noqa: E402


def sample_rgba(vol4, pos):
    """(P, 4): the four channels of vol4 (4, VX, VY, VZ) at pos (P, 3)."""
    return torch.stack([G.sample_volume_trilinear(vol4[k], pos) for k in range(4)], dim=1)


def raycast_rgba(vol4, cam, entry, exit_, rays, n, max_samples, sampling_rate, nondiff=False):
    """All pixels of one view at once. Returns (P, 4), the live-sample counts, and a mask of the rays with a live sample whose
    alpha lies within 1e-5 of 1e-3.
    nondiff: the non-differentiable march -- no max_samples clip, samples with alpha <= 1e-3 are counted but not composited,
    the result clamped to <= 1."""
    def sample(pos):
        c = sample_rgba(vol4, pos)
        opacity = 1.0 - torch.pow(1.0 - c[:, 3], 1.0 / sampling_rate)   # (rate 1: 1 - (1 - a), also for a > 1)
        shaded = torch.cat([opacity[:, None] * c[:, :3], opacity[:, None]], dim=1)
        return shaded, c[:, 3], dict(near=(c[:, 3] - 1e-3).abs() < 1e-5)

    out, _, count, counts = G.march(cam, entry, exit_, rays, n, max_samples, nondiff, sample)
    return out, count, counts["near"] > 0


def run(vol4, cam, entry, exit_, rays, n, grad_out, max_samples, sampling_rate, dtype=torch.float64, want_grad=True,
        pixels=None, nondiff=False):
    """The transliteration over views. vol4 (4,VX,VY,VZ) or (V,4,VX,VY,VZ), cam (V,3), ray buffers (V,W,H[,3]) and grad_out
    (V,W,H,4): numpy arrays (the GPU's ray buffers, copied). Rays with n <= 1 are not marched (pixel 0, H6) and `pixels` (a
    (V,W,H) mask) restricts the march further. Returns rgba, steps and d_vol ("dvol", the gradient of sum(out * grad_out)) as
    float64 numpy arrays in the shapes of the inputs, and `near`, the (V,W,H) mask of rays with a sample whose alpha lies within
    1e-5 of the non-differentiable march's 1e-3 threshold."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    V, W, H = n.shape
    volt = T(vol4).requires_grad_(want_grad)
    views, total = [], 0.0
    for v in range(V):
        def march_rays(sel):
            out, cnt, nr = raycast_rgba(volt[v] if vol4.ndim == 5 else volt, T(cam[v]), T(entry[v]).reshape(-1)[sel],
                                        T(exit_[v]).reshape(-1)[sel], T(rays[v]).reshape(-1, 3)[sel],
                                        torch.from_numpy(n[v].astype(np.int64)).reshape(-1)[sel], int(max_samples),
                                        float(sampling_rate), nondiff)
            return out, dict(steps=cnt.int(), near=nr)

        loss, res = G.render_view((W, H), n[v], None if pixels is None else pixels[v], T(grad_out[v]).reshape(-1, 4), march_rays)
        total = total + loss
        views.append(res)
    res = {k: np.stack([r[k] for r in views]) for k in ("rgba", "steps", "near")}
    if want_grad:
        if torch.is_tensor(total):
            total.backward()
        res["dvol"] = G.grad_or_zero(volt)
    return res
