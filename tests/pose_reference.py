"""Float64 reference of the free camera: look_from, look_at, up and a per-view fov, and their gradients.

A PyTorch transliteration of the pose ray setup -- view_dir = normalize(look_at - look_from), right = normalize(view_dir x up),
up' = normalize(right x view_dir), near_h = 2 tan(fov) near, near_w = near_h img_W / H, then the slab clipping, sample count and
jitter of tests/golden/make_camgrad_golden.ray_setup -- feeding `raycast` of make_autograd_golden.py, under that file's driver
`render_view`, and `project` of proj_reference.py (imported, not copied). run_march is the driver for any march of the posed
rays; tests/rgba_pose_reference.py uses it too. torch.autograd differentiates the whole program w.r.t. the ten pose parameters;
nothing is derived by hand. Each ray gets its own leaf copy of the pose, so a run holds every ray's contribution as well as the
total. The fov leaf is in RADIANS, as the C ABI's fov_v and its d_pose column 9 are.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_autograd_golden as G  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402

ORIGIN, UP_Y, FOV_DEG = (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 30.0


def ray_setup(look_from, look_at, up, fov_rad, W, H, vol_shape, sr, near=0.1, jitter_seed=0, view=0):
    """The pose ray setup for all W*H pixels as torch functions of look_from, look_at, up ((3,) or one row per pixel (W*H, 3))
    and fov_rad (a float, a 0-d tensor or one entry per pixel (W*H,)). Returns entry, exit (P,), rays (P,3), n (P,) int64."""
    dt = look_from.dtype
    P = W * H
    row = lambda a: a.expand(P, 3) if a.ndim == 1 else a
    lf, la, up0 = row(look_from), row(look_at.to(dt)), row(up.to(dt))
    fov = torch.as_tensor(fov_rad, dtype=dt)
    near_h = (2.0 * torch.tan(fov) * near).reshape(-1, 1)
    near_w = near_h * (W / H)
    VX, VY, VZ = vol_shape
    diag = math.sqrt((VX - 1) ** 2 + (VY - 1) ** 2 + (VZ - 1) ** 2)
    ii, jj = torch.meshgrid(torch.arange(W, dtype=dt), torch.arange(H, dtype=dt), indexing="ij")
    u = ((ii.reshape(-1) + 0.5) / W - 0.5)[:, None]
    v = ((jj.reshape(-1) + 0.5) / H - 0.5)[:, None]
    view_dir = CG._normalized(la - lf)
    right = CG._normalized(torch.cross(view_dir, up0, dim=-1))
    upp = CG._normalized(torch.cross(right, view_dir, dim=-1))
    near_m = lf + near * view_dir
    near_pos = near_m + (u * near_w) * right + (v * near_h) * upp
    vd = CG._normalized(near_pos - lf)
    # (the slab arithmetic of make_camgrad_golden.ray_setup, with its safe denominators for axial rays)
    axial = (vd == 0).detach()
    vd_safe = torch.where(axial, torch.ones_like(vd), vd)
    t_lo = torch.where(axial, ((-1.0 - lf) / vd).detach(), (-1.0 - lf) / vd_safe)
    t_hi = torch.where(axial, ((1.0 - lf) / vd).detach(), (1.0 - lf) / vd_safe)
    tmin = torch.minimum(t_lo, t_hi).max(dim=-1).values
    tmax = torch.maximum(t_lo, t_hi).min(dim=-1).values
    hit = ~((tmax < 0) | (tmin > tmax))
    ray_len = tmax - tmin
    n = torch.where(hit, torch.floor(sr * ray_len.detach() * diag) + 1.0, torch.zeros_like(ray_len)).detach()
    entry = tmin
    if jitter_seed != 0:
        uu = torch.from_numpy(CG.jitter_u(jitter_seed, view, np.arange(P))).to(dt)
        entry = tmin + uu * ray_len / torch.where(n > 0, n, torch.ones_like(n))
    return entry, tmax, vd, n.long()


def face_margin(look_from, rays, lo=True):
    """Per ray, the gap between the slab distance that decides tmin (lo) or tmax and the runner-up: rays near a face tie (an
    edge of the box) have a kink there and no gradient to pin."""
    lf = np.asarray(look_from, np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (-1.0 - lf) / rays, (1.0 - lf) / rays
    t = np.sort(np.minimum(a, b) if lo else np.maximum(a, b), axis=-1)
    return (t[..., 2] - t[..., 1]) if lo else (t[..., 1] - t[..., 0])


def _leaves(inp, dtype, P):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    lf = T(inp["look_from"]).expand(P, 3).clone().requires_grad_(True)
    la = T(inp.get("look_at", ORIGIN)).expand(P, 3).clone().requires_grad_(True)
    up = T(inp.get("up", UP_Y)).expand(P, 3).clone().requires_grad_(True)
    fov = T(inp.get("fov_rad", math.radians(FOV_DEG))).expand(P).clone().requires_grad_(True)
    return T, lf, la, up, fov


def _result(W, H, e, x, r, n, leaves):
    d_ray = np.concatenate([G.grad_or_zero(leaf).reshape(W * H, -1) for leaf in leaves], 1)   # (zeros: a leaf no ray depends on)
    return dict(entry=e.detach().double().numpy().reshape(W, H), exit=x.detach().double().numpy().reshape(W, H),
                rays=r.detach().double().numpy().reshape(W, H, 3), n=n.numpy().astype(np.int32).reshape(W, H),
                dpose_ray=d_ray.reshape(W, H, 10), dpose=d_ray.sum(0))


def run_march(inp, dtype, pixels, march):
    """run_case for any march of the rays: march(T, cam, entry, exit, rays, n), with T the conversion to `dtype` and one camera
    row per ray, returns their pixels (P, 4) and live-sample counts."""
    W, H = inp["grad_out"].shape[:2]
    P = W * H
    T, lf, la, up, fov = _leaves(inp, dtype, P)
    e, x, r, n = ray_setup(lf, la, up, fov, W, H, inp["vol"].shape[-3:], float(inp["sr"]), jitter_seed=int(inp["jitter_seed"]),
                           view=int(inp["view"]))

    def march_rays(sel):
        out, cnt = march(T, lf[sel], e[sel], x[sel], r[sel], n[sel])
        return out, dict(steps=cnt.int())

    loss, res = G.render_view((W, H), n, pixels, T(inp["grad_out"]).reshape(P, 4), march_rays)
    if torch.is_tensor(loss):   # (else no ray marched: a view that misses the box)
        loss.backward()
    return dict(res, **_result(W, H, e, x, r, n, (lf, la, up, fov)))


def run_case(inp, dtype=torch.float64, pixels=None):
    """Per-ray and total d (look_from, look_at, up, fov_rad) of sum(raycast(...) * grad_out), the forward in `dtype`.
    inp: vol, tf, look_from, grad_out (W,H,4), sr, max_samples, jitter_seed, view; optional look_at, up, fov_rad.
    pixels: flat indices of the rays to march (default all)."""
    return run_march(inp, dtype, pixels, lambda T, cam, e, x, r, n: G.raycast(
        T(inp["vol"]), T(inp["tf"]), cam, e, x, r, n, int(inp["max_samples"]), float(inp["sr"])))


def run_projection(inp, mode, dtype=torch.float64, arg_max=None):
    """The same for sum(project(...) * grad_out), grad_out (W,H); sr is 1 (the projections' fixed rate). mode "max" with
    arg_max (W,H): the gradient through those samples (the kernel's frozen argmax) instead of the run's own."""
    import proj_reference as PR
    W, H = inp["grad_out"].shape[:2]
    P = W * H
    T, lf, la, up, fov = _leaves(inp, dtype, P)
    e, x, r, n = ray_setup(lf, la, up, fov, W, H, inp["vol"].shape, 1.0, jitter_seed=int(inp["jitter_seed"]),
                           view=int(inp["view"]))
    S = inp.get("max_samples")
    vol = T(inp["vol"])
    out, arg = PR.project(vol, lf, e, x, r, n, S, mode)
    if mode == "max" and arg_max is not None:
        out = PR.sample_at(vol, lf, e, x, r, n, torch.from_numpy(np.asarray(arg_max).reshape(-1)))
    (out * T(inp["grad_out"]).reshape(P)).sum().backward()
    res = _result(W, H, e, x, r, n, (lf, la, up, fov))
    res.update(out=out.detach().double().numpy().reshape(W, H), arg=None if arg is None else arg.numpy().reshape(W, H))
    return res
