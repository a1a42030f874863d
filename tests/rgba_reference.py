"""Float64 (or float32) PyTorch transliteration of the march through a pre-classified RGBA volume, DESIGN.md D14.

The sample loop of tests/golden/make_autograd_golden.py's `raycast` (positions, sample count, max_samples clip, early termination
at A >= 0.99, front-to-back compositing), whose helpers are imported here, not copied, with the classification and the shading
taken out: a sample's (r, g, b, a) is the trilinear interpolation of the volume's four channels, each by the helpers'
sample_volume_trilinear (one cell, the lerps x -> y -> z), its opacity 1 - (1 - a)^(1 / sampling_rate), and it composites with
L = 1. Nothing of the backward is written here: torch.autograd differentiates the program, with its branch predicates frozen.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_autograd_golden as G  # noqa: E402
from make_autograd_golden import low_high_frac, mix, sample_volume_trilinear  # noqa: E402,F401


def _trilinear(vol, pos, dtype):
    old = G.F64
    G.F64 = dtype   # the helpers read their float type at call time
    try:
        return sample_volume_trilinear(vol, pos)
    finally:
        G.F64 = old


def sample_rgba(vol4, pos):
    """(P, 4): the four channels of vol4 (4, VX, VY, VZ) at pos (P, 3)."""
    return torch.stack([_trilinear(vol4[k], pos, vol4.dtype) for k in range(4)], dim=1)


def raycast_rgba(vol4, cam, entry, exit_, rays, n, max_samples, sampling_rate, nondiff=False):
    """All pixels of one view at once. Returns (P, 4), the live-sample counts, and a mask of the rays with a live sample whose
    alpha lies within 1e-5 of 1e-3.
    nondiff: the non-differentiable march -- no max_samples clip, samples with alpha <= 1e-3 are counted but not composited,
    the result clamped to <= 1."""
    dt = vol4.dtype
    P = entry.shape[0]
    tape = torch.zeros((P, 4), dtype=dt)
    count = torch.zeros(P, dtype=torch.long)
    near = torch.zeros(P, dtype=torch.bool)
    nf = n.to(dt)
    for s in range(int(n.max()) if P else 0):
        active = ((s < n) & (tape[:, 3] < 0.99) & (nondiff or s < max_samples)).detach()
        if not bool(active.any()):
            continue
        ray_len = exit_ - entry
        tmin = entry + 0.5 * ray_len / nf
        frac = torch.where(n > 1, float(s) / torch.clamp(nf - 1.0, min=1.0), torch.zeros_like(nf))
        pos = cam[None, :] + mix(tmin, exit_, frac)[:, None] * rays
        pos = torch.where(active[:, None], pos, torch.zeros_like(pos))
        c = sample_rgba(vol4, pos)
        opacity = 1.0 - torch.pow(1.0 - c[:, 3], 1.0 / sampling_rate)   # (rate 1: 1 - (1 - a), also for a > 1)
        shaded = torch.cat([opacity[:, None] * c[:, :3], opacity[:, None]], dim=1)
        # (a ray that is over takes no part: not even a 0 * NaN in the backward, should its pixel have become NaN)
        prev = torch.where(active[:, None], tape, torch.zeros_like(tape))
        new = (1.0 - prev[:, 3:4]) * shaded + prev
        near |= active & ((c[:, 3] - 1e-3).abs() < 1e-5).detach()
        lit = (active & (c[:, 3] > 1e-3)) if nondiff else active
        tape = torch.where(lit[:, None], new, tape)
        count = count + active.long()
    if nondiff:
        tape = torch.clamp(tape, max=1.0)
    return tape, count, near


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
    rgba = np.zeros((V, W, H, 4))
    steps = np.zeros((V, W, H), np.int32)
    near = np.zeros((V, W, H), bool)
    total = 0.0
    for v in range(V):
        live = n[v].reshape(-1) > 1
        if pixels is not None:
            live &= pixels[v].reshape(-1)
        sel = torch.from_numpy(np.nonzero(live)[0])
        if sel.numel() == 0:
            continue
        out, cnt, nr = raycast_rgba(volt[v] if vol4.ndim == 5 else volt, T(cam[v]), T(entry[v]).reshape(-1)[sel],
                                    T(exit_[v]).reshape(-1)[sel], T(rays[v]).reshape(-1, 3)[sel],
                                    torch.from_numpy(n[v].astype(np.int64)).reshape(-1)[sel], int(max_samples),
                                    float(sampling_rate), nondiff)
        flat = np.zeros((W * H, 4)); flat[sel.numpy()] = out.detach().double().numpy()
        rgba[v] = flat.reshape(W, H, 4)
        st = np.zeros(W * H, np.int32); st[sel.numpy()] = cnt.numpy()
        steps[v] = st.reshape(W, H)
        nm = np.zeros(W * H, bool); nm[sel.numpy()] = nr.numpy()
        near[v] = nm.reshape(W, H)
        total = total + (out * T(grad_out[v]).reshape(-1, 4)[sel]).sum()
    res = dict(rgba=rgba, steps=steps, near=near)
    if want_grad:
        if torch.is_tensor(total):
            total.backward()
        res["dvol"] = volt.grad.double().numpy() if volt.grad is not None else np.zeros(vol4.shape)
    return res
