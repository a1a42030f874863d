"""Float64 reference of the RGBA march's camera gradient: d (look_from, look_at, up, fov) of
sum(raycast_rgba(...) * grad_out), per ray and in total.

A composition, nothing here is written anew: the free camera's ray setup and its per-ray leaves (tests/pose_reference.py), the
RGBA march (tests/rgba_reference.py) with one camera row per ray (make_camgrad_golden._PerRayCam), and torch.autograd, which
differentiates the whole program with its branch predicates frozen. The fov leaf is in RADIANS, as the C ABI's column 9 is.
"""
import numpy as np
import torch

import pose_reference as PR
import rgba_reference as RR
from pose_reference import CG


def run_case(inp, dtype=torch.float64, pixels=None):
    """pose_reference.run_case for an RGBA volume: entry, exit, rays, n, steps, rgba, dpose_ray (W,H,10), dpose; the forward in
    `dtype`. inp: vol (4,VX,VY,VZ), look_from, grad_out (W,H,4), sr, max_samples, jitter_seed, view; optional look_at, up,
    fov_rad."""
    W, H = inp["grad_out"].shape[:2]
    P = W * H
    T, lf, la, up, fov = PR._leaves(inp, dtype, P)
    e, x, r, n = PR.ray_setup(lf, la, up, fov, W, H, inp["vol"].shape[-3:], float(inp["sr"]), jitter_seed=int(inp["jitter_seed"]),
                              view=int(inp["view"]))
    live = n > 1
    if pixels is not None:
        live &= torch.zeros_like(live).index_fill_(0, torch.as_tensor(pixels), True)
    sel = torch.nonzero(live)[:, 0]
    out_sel, cnt, _ = RR.raycast_rgba(T(inp["vol"]), CG._PerRayCam(lf[sel]), e[sel], x[sel], r[sel], n[sel],
                                      int(inp["max_samples"]), float(inp["sr"]))
    leaves = (lf, la, up, fov)
    if out_sel.requires_grad:
        (out_sel * T(inp["grad_out"]).reshape(P, 4)[sel]).sum().backward()
    for leaf in leaves:   # (no ray marched, or a leaf no ray depends on)
        if leaf.grad is None:
            leaf.grad = torch.zeros_like(leaf)
    res = PR._result(W, H, e, x, r, n, leaves)
    steps = np.zeros(P, np.int32); steps[sel.numpy()] = cnt.numpy()
    out = np.zeros((P, 4)); out[sel.numpy()] = out_sel.detach().double().numpy()
    res.update(steps=steps.reshape(W, H), rgba=out.reshape(W, H, 4))
    return res
