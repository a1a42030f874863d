"""Float64 (or float32) PyTorch transliteration of the X-ray line-integral and maximum intensity projections, DESIGN.md D13.

The samples are those of the march: the ray setup of tests/golden/make_camgrad_golden.py and the trilinear sample of
tests/golden/make_autograd_golden.py, both imported, not copied.
    s < m = min(n, max_samples) (m = 0 for n <= 1), t0 = entry + 0.5 (exit - entry)/n, pos_s = cam + mix(t0, exit, s/(n-1)) vd
    sum: D * sum_s mu(pos_s), D = (exit - entry)/n;   max: the first maximum over s (strict >), 0 when there is no sample
Nothing of the backward is written here: torch.autograd differentiates the program with its branches frozen (n, the jitter
draw, the slab faces, the trilinear cells, the argmax).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_autograd_golden as G  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402


def trilinear(vol, pos):
    old = G.F64
    G.F64 = vol.dtype   # the helper reads its float type at call time
    try:
        return G.sample_volume_trilinear(vol, pos)
    finally:
        G.F64 = old


def project(vol, cam, entry, exit_, rays, n, max_samples, mode):
    """vol (VX, VY, VZ); cam (3,) or (P, 3); entry, exit_ (P,), rays (P, 3), n (P,) integer. Returns out (P,) and, for "max",
    the argmax sample index (P,) int64 (-1: no sample); None for "sum"."""
    dt = vol.dtype
    P = n.shape[0]
    cam = cam.expand(P, 3) if cam.ndim == 1 else cam
    n = n.long()
    S = (1 << 62) if max_samples is None else int(max_samples)
    m = torch.where(n > 1, torch.clamp(n, max=S), torch.zeros_like(n))
    nf = torch.where(n > 0, n, torch.ones_like(n)).to(dt)   # (a missed ray's D is never used)
    t0 = entry + 0.5 * (exit_ - entry) / nf
    acc = torch.zeros(P, dtype=dt)
    best = torch.zeros(P, dtype=dt)
    arg = torch.full((P,), -1, dtype=torch.long)
    for s in range(int(m.max()) if P else 0):
        idx = torch.nonzero(s < m)[:, 0]
        f = s / (nf[idx] - 1.0)
        t = G.mix(t0[idx], exit_[idx], f)
        pos = cam[idx] + t[:, None] * rays[idx]
        mu = torch.zeros(P, dtype=dt).index_put((idx,), trilinear(vol, pos))
        live = torch.zeros(P, dtype=torch.bool).index_fill_(0, idx, True)
        if mode == "sum":
            acc = acc + mu
        else:
            upd = (live & ((arg < 0) | (mu > best))).detach()
            best = torch.where(upd, mu, best)
            arg = torch.where(upd, torch.full_like(arg, s), arg)
    if mode == "sum":
        return torch.where(m > 0, (exit_ - entry) / nf * acc, torch.zeros_like(acc)), None
    return best, arg


def project_camera(vol, cam, W, H, sr, max_samples, mode, fov_deg=30.0, near=0.1, jitter_seed=0, view=0):
    """The whole program from the camera: ray setup (make_camgrad_golden.ray_setup, one camera row per ray) + project.
    cam (3,) or (W*H, 3). Returns out (W*H,), arg, and the ray buffers (entry, exit, rays, n)."""
    e, x, r, n = CG.ray_setup(cam, W, H, tuple(vol.shape), sr, fov_deg, near, jitter_seed, view)
    out, arg = project(vol, cam, e, x, r, n, max_samples, mode)
    return out, arg, (e, x, r, n)
