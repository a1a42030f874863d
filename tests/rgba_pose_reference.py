"""Float64 reference of the RGBA march's camera gradient: d (look_from, look_at, up, fov) of
sum(raycast_rgba(...) * grad_out), per ray and in total.

A composition, nothing here is written anew: the free camera's ray setup, its per-ray leaves and its driver
(tests/pose_reference.run_march), the RGBA march (tests/rgba_reference.py) with one camera row per ray, and torch.autograd, which
differentiates the whole program with its branch predicates frozen. The fov leaf is in RADIANS, as the C ABI's column 9 is.
"""
import torch

import pose_reference as PR
import rgba_reference as RR


def run_case(inp, dtype=torch.float64, pixels=None):
    """pose_reference.run_case for an RGBA volume: entry, exit, rays, n, steps, rgba, dpose_ray (W,H,10), dpose; the forward in
    `dtype`. inp: vol (4,VX,VY,VZ), look_from, grad_out (W,H,4), sr, max_samples, jitter_seed, view; optional look_at, up,
    fov_rad."""
    return PR.run_march(inp, dtype, pixels, lambda T, cam, e, x, r, n: RR.raycast_rgba(
        T(inp["vol"]), cam, e, x, r, n, int(inp["max_samples"]), float(inp["sr"]))[:2])
