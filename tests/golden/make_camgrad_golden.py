#!/usr/bin/env python3
"""Reference camera gradients (d look_from): tests/golden/camgrad_*.npz.

A float64 PyTorch transliteration of the reference's ray setup -- compute_entry_exit + get_ray_direction +
get_entry_exit_points (differender/volume_raycaster.py:221-259, 127-151, 28-53) -- feeding `raycast` of
make_autograd_golden.py under that file's driver `render_view` (imported, not copied), which takes one camera row per ray as
it takes one camera. torch.autograd differentiates the whole program w.r.t. the camera; nothing
is derived by hand. Frozen, as in any reverse-mode AD of a program with branches: the sample count n (a floor), the jitter
draw u (recomputed from the counter hash the oracle and the kernels share), the slab faces max/min pick, and everything
make_autograd_golden.py freezes.

Each ray gets its own leaf copy of the camera (cam.expand(P, 3) made a leaf), so the fixtures hold every ray's contribution
as well as the total. Single-sample rays (0/0 position in the reference, H6) contribute nothing.
Run:  python tests/golden/make_camgrad_golden.py [case names]
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_autograd_golden as G  # noqa: E402


def _hash_u32(x):
    x = np.uint32(x)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x = np.uint32(x * np.uint32(0x7feb352d)); x ^= x >> np.uint32(15)
        x = np.uint32(x * np.uint32(0x846ca68b)); x ^= x >> np.uint32(16)
    return x


def jitter_u(seed, view, pix):
    """U[0,1) of (seed, view, pixel): the counter hash of oracle/dr_oracle_impl.inc and csrc/dr_device.h (24 bits)."""
    with np.errstate(over="ignore"):
        h = _hash_u32(np.uint32(seed) ^ np.uint32(0x9E3779B9))
        h = _hash_u32(h ^ np.uint32(np.uint32(view) * np.uint32(0x85EBCA6B) + np.uint32(0xC2B2AE35)))
        h = _hash_u32(h ^ np.uint32(pix).astype(np.uint32))
    return (h >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)


def _normalized(a):
    return a / torch.sqrt((a * a).sum(-1, keepdim=True))


def ray_setup(cam, W, H, vol_shape, sr, fov_deg=30.0, near=0.1, jitter_seed=0, view=0):
    """VR.py:221-259 (+127-151, 28-53) for all W*H pixels, as torch functions of `cam` ((3,) or one row per pixel (W*H, 3)).
    Returns entry, exit (P,), rays (P,3) and n (P,) int64 (frozen)."""
    dt = cam.dtype
    cam = cam.expand(W * H, 3) if cam.ndim == 1 else cam
    near_h = 2.0 * math.tan(math.radians(fov_deg)) * near
    near_w = near_h * (W / H)
    VX, VY, VZ = vol_shape
    diag = math.sqrt((VX - 1) ** 2 + (VY - 1) ** 2 + (VZ - 1) ** 2)
    ii, jj = torch.meshgrid(torch.arange(W, dtype=dt), torch.arange(H, dtype=dt), indexing="ij")
    u = ((ii.reshape(-1) + 0.5) / W - 0.5)[:, None]
    v = ((jj.reshape(-1) + 0.5) / H - 0.5)[:, None]
    view_dir = _normalized(-cam)
    up0 = torch.tensor([0.0, 1.0, 0.0], dtype=dt).expand_as(view_dir)
    right = _normalized(torch.cross(view_dir, up0, dim=-1))
    up = _normalized(torch.cross(right, view_dir, dim=-1))
    near_m = cam + near * view_dir
    near_pos = near_m + (u * near_w) * right + (v * near_h) * up
    vd = _normalized(near_pos - cam)
    # A ray along a coordinate plane has vd_a == 0: its slab distances on that axis are +-inf and never picked. Their values
    # stay (detached), but the division autograd sees has a safe denominator there, so the zero cotangent of the unpicked face
    # never meets an infinite slope (0 * inf = NaN otherwise).
    axial = (vd == 0).detach()
    vd_safe = torch.where(axial, torch.ones_like(vd), vd)
    t_lo = torch.where(axial, ((-1.0 - cam) / vd).detach(), (-1.0 - cam) / vd_safe)
    t_hi = torch.where(axial, ((1.0 - cam) / vd).detach(), (1.0 - cam) / vd_safe)
    tmin = torch.minimum(t_lo, t_hi).max(dim=-1).values
    tmax = torch.maximum(t_lo, t_hi).min(dim=-1).values
    hit = ~((tmax < 0) | (tmin > tmax))
    ray_len = tmax - tmin
    n = torch.where(hit, torch.floor(sr * ray_len.detach() * diag) + 1.0, torch.zeros_like(ray_len)).detach()
    entry = tmin
    if jitter_seed != 0:
        uu = torch.from_numpy(jitter_u(jitter_seed, view, np.arange(W * H))).to(dt)
        entry = tmin + uu * ray_len / torch.where(n > 0, n, torch.ones_like(n))   # (a missed ray's entry is never used)
    return entry, tmax, vd, n.long()


CASES = {
    # name: (volume shape, image, R, sampling rate, max_samples, TF kind, camera, jitter seed[, volume kind])
    "a_orbit_sr1": ((16, 16, 16), (16, 16), 8, 1.0, 4096, "thin", ("orbit", 0.8), 0),
    "b_sr2_ert": ((20, 16, 24), (16, 12), 16, 2.0, 4096, "opaque", ("orbit", 2.1), 0),
    "c_clip": ((24, 24, 24), (12, 16), 12, 1.0, 23, "thin", ("orbit", 4.0), 0),
    "d_jitter": ((18, 22, 16), (16, 16), 32, 1.0, 4096, "opaque", ("orbit", 5.2), 4242),
    "e_nonsquare": ((16, 20, 16), (20, 12), 8, 1.0, 4096, "thin", ("orbit", 1.3), 0),
    "f_near_face": ((16, 16, 16), (16, 16), 8, 1.0, 4096, "thin", ("point", (1.2, 0.35, 1.25)), 0),
    # rays with a direction component of exactly 0: the camera in the plane y = 0 and an odd H (a row), x = 0 and an odd W (a
    # column), on the x axis with both odd (the centre ray has two). On the axis the rays of the image's diagonals have
    # |vd.y| == |vd.z|: from outside the box about 5 % of the rays leave it through an edge, a tie of two faces where tmax has
    # a kink and no gradient to pin; from x = 0.7 all of them leave through the face x = -1.
    "g_plane_y0": ((16, 20, 18), (16, 15), 8, 1.0, 4096, "thin", ("point", (2.4, 0.0, 0.7)), 0),
    "h_plane_x0": ((18, 16, 20), (15, 16), 8, 1.0, 4096, "thin", ("point", (0.0, 0.6, 2.4)), 0),
    "i_on_x_axis": ((16, 16, 16), (19, 17), 8, 1.0, 4096, "thin", ("point", (0.7, 0.0, 0.0)), 0),
    # the camera inside the box: every entry distance is negative
    "j_inside": ((18, 16, 20), (16, 14), 8, 1.0, 4096, "thin", ("point", (0.3, 0.2, -0.4)), 0),
    "k_inside_sr2_ert": ((18, 16, 20), (18, 16), 16, 2.0, 4096, "opaque", ("point", (0.3, 0.2, -0.4)), 31),
    "l_anisotropic": ((40, 12, 20), (18, 14), 12, 1.0, 4096, "thin", ("point", (1.7, 1.1, -1.6)), 0),
    # an object in air: exact zeros outside a ball, four exact plateaus inside, alpha(0) = 0 -- flat normals (D1) on every ray
    "m_object_in_air": ((24, 24, 24), (20, 20), 16, 1.0, 4096, "air", ("orbit", 3.3), 0, "plateaus"),
    # the volume of case a with a few dozen voxels outside [0, 1]
    "n_out_of_range": ((16, 16, 16), (16, 16), 8, 1.0, 4096, "thin", ("orbit", 0.8), 0, "out_of_range"),
    # `right` is along z for a camera with z = 0, so the rays of an image row share their projection onto the x-y plane; from
    # this height row 12 leaves through the face x = -1 at y = 0.9995, within the normal's tap distance (1e-3) of the edge to
    # y = 1: the +y tap of the last sample lies outside the box, where clamp holds the position and its slope is 0
    "o_edge_grazing": ((16, 18, 16), (16, 16), 8, 1.0, 4096, "thin", ("point", (2.4, 0.1994, 0.0)), 0),
}
VIEW = 2   # view index of the jitter hash


def plateau_ball(vshape, rng):
    """Exact 0 outside a (slightly lumpy) ball, the plateaus 0.125, 0.25, 0.5 and 1 in shells inside it. Powers of two: the
    trilinear mix of eight equal voxels returns them exactly in float32 and float64, with an fma or without, so the six taps
    of the normal cancel to an exact 0 there in the kernel and in the reference alike."""
    ax = [np.linspace(-1.0, 1.0, n) for n in vshape]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    r = np.sqrt(X * X + Y * Y + Z * Z) + 0.06 * np.sin(4.0 * X + 1.0) * np.cos(3.0 * Y) + 0.03 * rng.standard_normal(vshape)
    return np.select([r < 0.28, r < 0.52, r < 0.76, r < 0.98], [1.0, 0.5, 0.25, 0.125], 0.0)


def make_inputs(name):
    from oracle import oracle as O
    vshape, WH, R, sr, S, kind, (ck, cv), seed = CASES[name][:8]
    vkind = CASES[name][8] if len(CASES[name]) > 8 else "synth"
    rng = np.random.RandomState(sorted(CASES).index(name) + 11)
    if vkind == "plateaus":
        vol = plateau_ball(vshape, rng)
    elif vkind == "out_of_range":
        # case a's volume; 2 x 2 x 1 plates (no cell with eight equal corners: those would be flat up to rounding noise only)
        vol = make_inputs("a_orbit_sr1")["vol"].copy()
        for k in range(12):
            x, y, z = rng.randint(3, vshape[0] - 4, size=3)
            vol[x:x + 2, y:y + 2, z] = 1.3 if k % 2 == 0 else -0.2
    else:
        vol = O.synth_volume(vshape, dtype=np.float64)
        vol = np.clip(vol + 0.02 * rng.standard_normal(vshape), 0.0, 1.0)
    tf = rng.uniform(0.05, 0.95, size=(R, 4))
    if kind == "air":
        tf[:, 3] = np.linspace(0.0, 0.25, R)
    else:
        tf[:, 3] = np.linspace(0.01, 0.06, R) if kind == "thin" else np.linspace(0.0, 0.9, R) ** 2 + 0.05
    cam = O.in_circles(cv).astype(np.float64) if ck == "orbit" else np.array(cv, np.float64)
    g = rng.standard_normal((*WH, 4))
    return dict(vol=vol, tf=tf, cam=cam, grad_out=g, sr=np.float64(sr), max_samples=np.int32(S), jitter_seed=np.int64(seed),
                view=np.int32(VIEW))


def run_case(inp, dtype=torch.float64, pixels=None):
    """Per-ray and total d look_from of sum(out * grad_out), the forward in `dtype` (float32: the same program in f32).
    pixels: flat indices of the rays to march (default all; rays are independent, the others get zeros)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    W, H = inp["grad_out"].shape[:2]
    P = W * H
    cam_pp = T(inp["cam"]).expand(P, 3).clone().requires_grad_(True)
    vshape = inp["vol"].shape
    e, x, r, n = ray_setup(cam_pp, W, H, vshape, float(inp["sr"]), jitter_seed=int(inp["jitter_seed"]), view=int(inp["view"]))

    def march_rays(sel):
        out, cnt = G.raycast(T(inp["vol"]), T(inp["tf"]), cam_pp[sel], e[sel], x[sel], r[sel], n[sel], int(inp["max_samples"]),
                             float(inp["sr"]))
        return out, dict(steps=cnt.int())

    loss, res = G.render_view((W, H), n, pixels, T(inp["grad_out"]).reshape(P, 4), march_rays)
    if torch.is_tensor(loss):
        loss.backward()
    d_ray = G.grad_or_zero(cam_pp)
    return dict(res, entry=e.detach().double().numpy().reshape(W, H), exit=x.detach().double().numpy().reshape(W, H),
                rays=r.detach().double().numpy().reshape(W, H, 3), n=n.numpy().astype(np.int32).reshape(W, H),
                dcam_ray=d_ray.reshape(W, H, 3), dcam=d_ray.sum(0))


def sample_stats(inp, res):
    """Per ray, over the live samples of the forward: how many have a flat normal (get_volume_normal's flag, D1) and how many
    an intensity outside [0, 1] -- what cases m and n are named for."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    W, H = res["n"].shape
    vol, cam = T(inp["vol"]), T(inp["cam"])
    e, x, r = T(res["entry"]).reshape(-1), T(res["exit"]).reshape(-1), T(res["rays"]).reshape(-1, 3)
    n, steps = torch.from_numpy(res["n"].reshape(-1)).long(), torch.from_numpy(res["steps"].reshape(-1)).long()
    flat, outside = torch.zeros_like(n), torch.zeros_like(n)
    for s in range(int(steps.max())):
        live = (s < steps) & (n > 1)
        pos = G.sample_pos(cam, e, x, r, n, s, live)
        I = G.sample_volume_trilinear(vol, pos)
        flat += live & G.get_volume_normal(vol, pos)[1]
        outside += live & ((I < 0) | (I > 1))
    return flat.numpy().reshape(W, H), outside.numpy().reshape(W, H)


def main(names=None):
    for name in names or CASES:
        inp = make_inputs(name)
        res = run_case(inp)
        path = os.path.join(HERE, f"camgrad_{name}.npz")
        np.savez_compressed(path, **inp, **res)
        print("wrote", path, os.path.getsize(path), "bytes; rays n>1:", int((res["n"] > 1).sum()), "terminated early:",
              int(((res["steps"] < np.minimum(res["n"], inp["max_samples"])) & (res["n"] > 1)).sum()),
              "clipped:", int((res["n"] > inp["max_samples"]).sum()), "dcam", res["dcam"])


if __name__ == "__main__":
    main(sys.argv[1:])   # no arguments: every case
