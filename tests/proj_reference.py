"""Float64 (or float32) PyTorch transliteration of the X-ray line-integral and maximum intensity projections, DESIGN.md D13.

The samples are those of the march: the ray setup of tests/golden/make_camgrad_golden.py and the trilinear sample of
tests/golden/make_autograd_golden.py, both imported, not copied.
    s < m = min(n, max_samples) (m = 0 for n <= 1), t0 = entry + 0.5 (exit - entry)/n, pos_s = cam + mix(t0, exit, s/(n-1)) vd
    sum: D * sum_s mu(pos_s), D = (exit - entry)/n;   max: the first maximum over s (strict >), 0 when there is no sample
Nothing of the backward is written here: torch.autograd differentiates the program with its branches frozen (n, the jitter
draw, the slab faces, the trilinear cells, the argmax).

Beside the program: sample_at (one sample of every ray, for the MIP at a given argmax), project_top2 (how clear a maximum is),
window_plan (which path the windowed SUM backward takes: a float32 model of its decisions, not of its arithmetic) and the case
tables of tests/test_gpu_projection_edges.py, which tests/test_projection.py checks on the CPU.
"""
import collections
import math
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_autograd_golden as G  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402


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
        mu = torch.zeros(P, dtype=dt).index_put((idx,), G.sample_volume_trilinear(vol, pos))
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


def sample_at(vol, cam, entry, exit_, rays, n, s):
    """The trilinear value of each ray's sample number s (P,) -- project's own position arithmetic, differentiable in vol (and
    in cam, entry, exit_, rays). A ray without samples (n <= 1) or with s < 0 gives 0. s is not clipped by any max_samples."""
    dt = vol.dtype
    P = n.shape[0]
    cam = cam.expand(P, 3) if cam.ndim == 1 else cam
    n, s = n.long(), s.long()
    idx = torch.nonzero((n > 1) & (s >= 0))[:, 0]
    nf = n[idx].to(dt)
    t0 = entry[idx] + 0.5 * (exit_[idx] - entry[idx]) / nf
    f = s[idx].to(dt) / (nf - 1.0)
    t = G.mix(t0, exit_[idx], f)
    pos = cam[idx] + t[:, None] * rays[idx]
    return torch.zeros(P, dtype=dt).index_put((idx,), G.sample_volume_trilinear(vol, pos))


# ---- which path the windowed SUM backward takes (a model of its decisions only, to choose test cases) ----------------------------

KERNEL_SOURCE = os.path.join(os.path.dirname(HERE), "differender_amd", "csrc", "projection.hip")
WindowPlan = collections.namedtuple("WindowPlan", "lds_full lds_halved fallback dead_tiles live_tiles")


def window_constants():
    """PW_TILE, PW_BOX, PW_WIN_VOX, PW_MIN_VOX as projection.hip defines them today."""
    text = open(KERNEL_SOURCE).read()
    out = {}
    for name in ("PW_TILE", "PW_BOX", "PW_WIN_VOX", "PW_MIN_VOX"):
        m = re.search(r"constexpr\s+(?:int|float)\s+%s\s*=\s*([0-9.]+)f?\s*;" % name, text)
        assert m, name
        out[name] = float(m.group(1))
    return out


def _fma32(a, b, c):
    # (a product of two float32 is exact in float64; the sum is rounded twice, which a path count does not see)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _cells32(cam, t0, exit_, rays, n, s, vshape):
    """sample_pos + tri_cell of dr_device.h in float32: the low and high cell index per axis, (P, 3) each."""
    f32 = np.float32
    f = s.astype(f32) / (n - 1).astype(f32)
    t = _fma32(exit_, f, t0 * (f32(1.0) - f))
    lo, hi = [], []
    for a in range(3):
        p = _fma32(t, rays[:, a], np.full_like(t, cam[a]))
        sc = f32(float(vshape[a]) - 1.0 - 1e-4)
        q = np.minimum(f32(1.0), np.maximum(f32(0.0), _fma32(np.full_like(p, 0.5), p, np.full_like(p, 0.5)))) * sc
        c0 = np.minimum(np.floor(np.maximum(q, f32(0.0))).astype(np.int64), vshape[a] - 1)
        lo.append(c0)
        hi.append(np.minimum(c0 + 1, vshape[a] - 1))
    return np.stack(lo, 1), np.stack(hi, 1)


def window_plan(cam, entry, exit_, rays, n, vshape, max_samples, W, H):
    """project_bwd_window_kernel's choice of path, window by window, for one view: cam (3,), entry, exit_, n (W*H,) or (W, H),
    rays (W*H, 3) or (W, H, 3), anything numpy can read. A plain float32 model of the tile's depth range, the window walk, the
    box of the first and last sample's cells and the `continue` / `if` / `else if` that follow -- no scatter, no weights (every
    ray with samples is taken as live: a zero or NaN upstream gradient is not modelled). Returns WindowPlan: windows that went
    to LDS at the first depth, to LDS at a halved depth, to global atomics; tiles without a live ray; tiles with one."""
    f32 = np.float32
    K = window_constants()
    T, BOX = int(K["PW_TILE"]), int(K["PW_BOX"])
    cam = np.asarray(cam, dtype=f32).reshape(3)
    entry = np.asarray(entry, dtype=f32).reshape(W, H)
    exit_ = np.asarray(exit_, dtype=f32).reshape(W, H)
    rays = np.asarray(rays, dtype=f32).reshape(W, H, 3)
    n = np.asarray(n).astype(np.int64).reshape(W, H)
    S = (1 << 31) - 1 if max_samples is None else int(max_samples)
    vox = f32(2.0) / f32(max(vshape) - 1)
    win_t0, win_tmin = f32(K["PW_WIN_VOX"]) * vox, f32(K["PW_MIN_VOX"]) * vox
    full = halved = fallback = dead = alive = 0
    for i0 in range(0, W, T):
        for j0 in range(0, H, T):
            sl = (slice(i0, min(i0 + T, W)), slice(j0, min(j0 + T, H)))
            nn = n[sl].reshape(-1)
            keep = nn > 1
            if not keep.any():
                dead += 1
                continue
            alive += 1
            nn = nn[keep]
            en, ex, rr = entry[sl].reshape(-1)[keep], exit_[sl].reshape(-1)[keep], rays[sl].reshape(-1, 3)[keep]
            m = np.minimum(nn, S)
            t0 = en + f32(0.5) * (ex - en) / nn.astype(f32)
            s_per_t = (nn - 1).astype(f32) / (ex - t0)
            tlo, thi = t0.min(), ex.max()
            s_cur = np.zeros_like(nn)
            tw0, d = tlo, win_t0
            while True:
                tw1 = f32(tw0 + d)
                last = (not tw1 < thi) or (not tw1 > tw0)
                s_end = m.copy()
                if not last:
                    k = np.minimum(np.maximum((tw1 - t0) * s_per_t, f32(0.0)), m.astype(f32))
                    s_end = np.maximum(s_cur, np.ceil(k).astype(np.int64))
                act = s_cur < s_end
                nvox = 0
                if act.any():
                    a = (cam, t0[act], ex[act], rr[act], nn[act])
                    lo0, hi0 = _cells32(*a, s_cur[act], vshape)
                    lo1, hi1 = _cells32(*a, s_end[act] - 1, vshape)
                    ext = np.maximum(hi0, hi1).max(0) - np.minimum(lo0, lo1).min(0) + 1
                    nvox = int(ext[0]) * int(ext[1]) * int(ext[2])
                if nvox > BOX and d > win_tmin:
                    d = f32(d * f32(0.5))
                    continue
                if 0 < nvox <= BOX:
                    if d == win_t0:
                        full += 1
                    else:
                        halved += 1
                elif nvox > 0:
                    fallback += 1
                s_cur, tw0 = s_end, tw1
                if last:
                    break
    return WindowPlan(full, halved, fallback, dead, alive)


def project_top2(vol, cam, entry, exit_, rays, n, max_samples):
    """The MIP's maximum, its first index and the gap to the largest OTHER sample (inf for a ray with one sample), (P,) each;
    rays without samples give 0, -1, inf. For choosing which argmax comparisons are well-posed, not differentiated."""
    P = n.shape[0]
    n = n.long()
    S = (1 << 62) if max_samples is None else int(max_samples)
    m = torch.where(n > 1, torch.clamp(n, max=S), torch.zeros_like(n))
    best, arg = project(vol.detach(), cam, entry, exit_, rays, n, max_samples, "max")
    second = torch.full((P,), -math.inf, dtype=vol.dtype)
    with torch.no_grad():
        for s in range(int(m.max()) if P else 0):
            v = sample_at(vol, cam, entry, exit_, rays, n, torch.full((P,), s))
            second = torch.where((s < m) & (arg != s), torch.maximum(second, v), second)
    return best, arg, best - second


def orbit(theta, phi, r):
    return [r * math.cos(phi) * math.sin(theta), r * math.sin(phi), r * math.cos(phi) * math.cos(theta)]


def layout_volume(vals, layout):
    """vals ([V,] VX, VY, VZ) -> the same values and shape with the memory layout "z" (field order, z contiguous), "x" (what
    Projector hands over), "y", or "strided": every second element along x of a twice larger x-innermost tensor whose other
    elements are NaN, so that no stride is 1 and a dense d_vol's strides differ from the volume's."""
    lead = tuple(range(vals.ndim - 3))
    k = len(lead)
    perm = lambda *p: lead + tuple(k + q for q in p)
    if layout == "z":
        return vals.contiguous()
    if layout == "x":
        return vals.permute(perm(1, 2, 0)).contiguous().permute(perm(2, 0, 1))
    if layout == "y":
        return vals.permute(perm(2, 0, 1)).contiguous().permute(perm(1, 2, 0))
    if layout == "strided":
        src = vals.permute(perm(1, 2, 0))
        big = torch.full(src.shape[:-1] + (2 * src.shape[-1],), math.nan, dtype=vals.dtype, device=vals.device)
        big[..., ::2] = src
        return big[..., ::2].permute(perm(2, 0, 1))
    raise ValueError(layout)


# The windowed / plain SUM backward cases of tests/test_gpu_projection_edges.py. paths: the window kernel's paths the case is
# there for ("lds_full", "lds_halved", "fallback": WindowPlan's fields); tests/test_projection.py holds every claim to
# window_plan on float32 rays from the transliterated ray setup. max_samples clips more than a third of the live rays where set.
EDGE_CASES = {
    "full_strided": dict(vshape=(32, 28, 36), WH=(53, 45), sr=1.0, seed=0, cams=[orbit(0.6, 0.3, 2.7)], fov=30.0, S=None,
                         dtype=torch.float32, own=False, layout="strided", paths=("lds_full", "lds_halved")),
    "halved_x_clipped": dict(vshape=(64, 56, 48), WH=(41, 37), sr=1.5, seed=0, cams=[orbit(0.4, 0.4, 2.6)], fov=30.0, S=160,
                             dtype=torch.float32, own=False, layout="x", paths=("lds_halved", "fallback")),
    "inside_near_wide": dict(vshape=(64, 64, 64), WH=(35, 37), sr=1.0, seed=0, cams=[[0.1, 0.2, 0.6]], fov=60.0, S=None,
                             dtype=torch.float32, own=False, layout="z", paths=("lds_full", "lds_halved", "fallback")),
    "far_f16": dict(vshape=(40, 40, 40), WH=(50, 45), sr=1.0, seed=0, cams=[orbit(0.3, 0.2, 6.0)], fov=30.0, S=None,
                    dtype=torch.float16, own=False, layout="x", paths=("fallback",), dead_tiles=True),
    "views_own_y": dict(vshape=(36, 32, 40), WH=(37, 35), sr=1.3, seed=77, cams=[orbit(k + 0.3, 0.1 * k, 2.8) for k in range(3)],
                        fov=30.0, S=None, dtype=torch.float32, own=True, layout="y", paths=("lds_full", "lds_halved")),
    "aniso_z": dict(vshape=(72, 24, 36), WH=(41, 38), sr=1.0, seed=5, cams=[orbit(0.9, -0.3, 2.9)], fov=30.0, S=None,
                    dtype=torch.float32, own=False, layout="z", paths=("lds_halved", "fallback")),
    "f16_clipped": dict(vshape=(44, 40, 36), WH=(39, 45), sr=1.2, seed=31, cams=[orbit(2.2, -0.35, 2.6)], fov=30.0, S=100,
                        dtype=torch.float16, own=False, layout="z", paths=("lds_full", "lds_halved")),
    "views_own_strided_f16": dict(vshape=(28, 30, 26), WH=(35, 34), sr=1.0, seed=3, cams=[orbit(1.1 * k, 0.2, 2.7) for k in range(2)],
                                  fov=30.0, S=None, dtype=torch.float16, own=True, layout="strided", paths=("lds_full",)),
}

# The camera backward cases: small enough for one camera leaf per ray in float64. view_base: the jitter hash's first view.
CAM_CASES = {
    "clipped": dict(vshape=(20, 18, 22), WH=(13, 11), sr=1.5, seed=0, cams=[orbit(0.5, 0.3, 2.7)], fov=30.0, S=30,
                    dtype=torch.float32, view_base=0),
    "f16": dict(vshape=(16, 20, 18), WH=(11, 13), sr=1.0, seed=21, cams=[orbit(2.4, -0.3, 2.9)], fov=30.0, S=None,
                dtype=torch.float16, view_base=0),
    "fov50": dict(vshape=(18, 16, 20), WH=(18, 10), sr=1.0, seed=0, cams=[orbit(-0.8, 0.25, 1.9)], fov=50.0, S=None,
                  dtype=torch.float32, view_base=0),
    "views4_jitter": dict(vshape=(14, 16, 12), WH=(10, 9), sr=1.2, seed=4711, cams=[orbit(0.9 * k, 0.3 - 0.2 * k, 2.8) for k in range(4)],
                          fov=30.0, S=None, dtype=torch.float32, view_base=5),
    "odd_missed": dict(vshape=(16, 16, 16), WH=(21, 19), sr=1.0, seed=8, cams=[orbit(0.3, 0.2, 4.5)], fov=30.0, S=None,
                       dtype=torch.float32, view_base=2),
}

# The MIP cases (arg_max and the MAX d_vol): rates 1 - 2.5 on random volumes of at most 44 voxels per axis -- the MAX forward's
# tolerance (1e-5 of the scale) is that of one sample whose float32 position moves its value by slope x 2e-7, and the slope
# grows with the voxel count: the cases stay where tests/test_gpu_projection.py applies it (40 voxels).
MIP_CASES = {
    "f32": dict(vshape=(40, 36, 44), WH=(23, 19), sr=1.0, seed=0, cams=[orbit(0.7, 0.3, 2.7)], fov=30.0, S=None,
                dtype=torch.float32, own=False),
    "f16": dict(vshape=(36, 40, 38), WH=(19, 21), sr=2.5, seed=12, cams=[orbit(-1.3, 0.5, 2.5)], fov=30.0, S=None,
                dtype=torch.float16, own=False),
    "clipped": dict(vshape=(44, 40, 36), WH=(21, 18), sr=2.0, seed=0, cams=[orbit(2.0, -0.2, 2.8)], fov=30.0, S=90,
                    dtype=torch.float32, own=False),
    "views_own": dict(vshape=(36, 36, 36), WH=(17, 15), sr=2.0, seed=99, cams=[orbit(k + 0.2, 0.15, 2.9) for k in range(3)],
                      fov=30.0, S=None, dtype=torch.float32, own=True),
}


def case_values(case, seed, views=None, lo=0.0):
    """The case's volume values on the CPU, ([views,] VX, VY, VZ) float32 already rounded to the case's dtype."""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(case["vshape"]) if views is None else (views,) + tuple(case["vshape"])
    return (lo + torch.rand(shape, generator=g)).to(case["dtype"]).float()
