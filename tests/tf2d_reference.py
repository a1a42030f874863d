"""Float64 (or float32) PyTorch transliteration of the march with a 2-D (value, gradient-magnitude) transfer function, DESIGN.md D12.

The 1-D program of tests/golden/make_autograd_golden.py -- the reference's `raycast` + `get_final_image`: its sample loop
(`march`), its lighting (`fixed_lighting`), its helpers and its per-view driver (`render_view`) are imported here, not copied --
with one change, the classification:
    I = trilinear(pos); (dx, dy, dz) = the six normal taps (delta 1e-3); u = |(dx, dy, dz)| * g_scale
    xv = I (RV - 1), xg = u (RG - 1); low_high_frac and the index clamp on each axis
    rgba = mix(mix(T[v0][g0], T[v1][g0], fv), mix(T[v0][g1], T[v1][g1], fv), fg)
Nothing of the backward is written here: torch.autograd differentiates the program, with its branch predicates frozen (max(x, 0)
passes the gradient iff 0 < x). Flat samples (|grad| = 0) send nothing through the normal or through u (D1, extended).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_autograd_golden as G  # noqa: E402


def taps(vol, pos):
    """(dx, dy, dz) (P, 3) of the shading normal, get_volume_normal's central differences."""
    dt = vol.dtype
    d = 1e-3
    out = []
    for axis in range(3):
        e = torch.zeros(3, dtype=dt)
        e[axis] = d
        out.append(G.sample_volume_trilinear(vol, pos + e) - G.sample_volume_trilinear(vol, pos - e))
    return torch.stack(out, dim=1)


def classify_2d(tf2d, intensity, u):
    """rgba (P, 4) of a (RV, RG, 4) table at value `intensity` and scaled gradient magnitude `u`."""
    RV, RG = tf2d.shape[0], tf2d.shape[1]
    v0, v1, fv = G.low_high_frac(intensity * float(RV - 1))
    g0, g1, fg = G.low_high_frac(u * float(RG - 1))
    v0 = torch.clamp(v0, max=RV - 1); v1 = torch.clamp(v1, max=RV - 1)
    g0 = torch.clamp(g0, max=RG - 1); g1 = torch.clamp(g1, max=RG - 1)
    fv, fg = fv[:, None], fg[:, None]
    lo = G.mix(tf2d[v0, g0], tf2d[v1, g0], fv)
    hi = G.mix(tf2d[v0, g1], tf2d[v1, g1], fv)
    return G.mix(lo, hi, fg)


def raycast_tf2d(vol, tf2d, g_scale, cam, entry, exit_, rays, n, max_samples, sampling_rate, nondiff=False):
    """G.march with G.raycast's sample under the 2-D classification, for all pixels at once (one view). Returns (P, 4), the
    live-sample counts, a mask of the rays with a live sample whose alpha lies within 1e-5 of 1e-3, and the per-ray count of
    live flat samples (|grad| = 0 exactly).
    nondiff: the non-differentiable march (VR.py:308-361) -- no max_samples clip, samples with alpha <= 1e-3 are counted but
    not composited, unclamped lighting, the result clamped to <= 1."""
    light_pos = G.light_position(cam)

    def sample(pos):
        intensity = G.sample_volume_trilinear(vol, pos)
        g = taps(vol, pos)
        n2 = (g * g).sum(1)
        flat = (n2 == 0).detach()
        gnorm = torch.where(flat, torch.zeros_like(n2), torch.sqrt(torch.where(flat, torch.ones_like(n2), n2)))
        normal = torch.where(flat[:, None], torch.zeros_like(g), g / torch.where(flat, torch.ones_like(gnorm), gnorm)[:, None])
        sample_color = classify_2d(tf2d, intensity, gnorm * g_scale)
        opacity = 1.0 - torch.pow(1.0 - sample_color[:, 3], 1.0 / sampling_rate)
        Lraw = G.fixed_lighting(pos, normal, flat, rays, light_pos)
        L = Lraw if nondiff else torch.where(Lraw > 1.0, torch.ones_like(Lraw), Lraw)
        shaded = torch.cat([(L * opacity)[:, None] * sample_color[:, :3], opacity[:, None]], dim=1)
        return shaded, sample_color[:, 3], dict(near=(sample_color[:, 3] - 1e-3).abs() < 1e-5, flat=flat)

    out, _, count, counts = G.march(cam, entry, exit_, rays, n, max_samples, nondiff, sample)
    return out, count, counts["near"] > 0, counts["flat"]


def run(vol, tf2d, g_scale, cam, entry, exit_, rays, n, grad_out, max_samples, sampling_rate, dtype=torch.float64,
        want_grad=True, pixels=None, want_vol=True, nondiff=False, count_flat=False):
    """The transliteration over views. vol (VX,VY,VZ) or (V,VX,VY,VZ), tf2d (RV,RG,4) or (V,RV,RG,4), cam (V,3), ray buffers
    (V,W,H[,3]) and grad_out (V,W,H,4): numpy arrays (the GPU's ray buffers, copied). Rays with n <= 1 are not marched (0/0 in
    the reference, H6) and `pixels` (a (V,W,H) mask) restricts the march further. Returns rgba, steps, d_vol, d_tf2d as float64
    numpy arrays in the shapes of the inputs (the gradients of sum(out * grad_out); want_vol=False leaves d_vol out), and `near`,
    the (V,W,H) mask of rays with a sample whose alpha lies within 1e-5 of the non-differentiable march's 1e-3 threshold.
    count_flat: also return "flat", the (V,W,H) count of each ray's live samples whose six taps cancel exactly (|grad| = 0 in
    `dtype`)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    V, W, H = n.shape
    volt = T(vol).requires_grad_(want_grad and want_vol)
    tft = T(tf2d).requires_grad_(want_grad)
    views, total = [], 0.0
    for v in range(V):
        def march_rays(sel):
            out, cnt, nr, nf = raycast_tf2d(volt[v] if vol.ndim == 4 else volt, tft[v] if tf2d.ndim == 4 else tft, float(g_scale),
                                            T(cam[v]), T(entry[v]).reshape(-1)[sel], T(exit_[v]).reshape(-1)[sel],
                                            T(rays[v]).reshape(-1, 3)[sel], torch.from_numpy(n[v].astype(np.int64)).reshape(-1)[sel],
                                            int(max_samples), float(sampling_rate), nondiff)
            return out, dict(steps=cnt.int(), near=nr, flat=nf)

        loss, res = G.render_view((W, H), n[v], None if pixels is None else pixels[v], T(grad_out[v]).reshape(-1, 4), march_rays)
        total = total + loss
        views.append(res)
    res = {k: np.stack([r[k] for r in views]) for k in ("rgba", "steps", "near") + (("flat",) if count_flat else ())}
    if want_grad:
        if torch.is_tensor(total):
            total.backward()
        if want_vol:
            res["dvol"] = G.grad_or_zero(volt)
        res["dtf"] = G.grad_or_zero(tft)
    return res


def plateau_volume(shape, seed=0, lo=-0.25, hi=2.0):
    """A field-order (VX, VY, VZ) float32 object in air with exact plateaus, by Chebyshev distance m = max(|x|, |y|, |z|) from
    the centre ([-1, 1] on every axis): air exactly 0 (m >= 0.72), a plateau at exactly 0.25 (0.48 <= m < 0.72), a shell with
    structure in [0.1, 0.9] (0.26 <= m < 0.48), a core plateau at exactly 0.5 (m < 0.26); and two blocks outside the value
    range, `hi` (> 1) and `lo` (< 0), cut into the 0.25 plateau. No voxel lies in (0, 1e-3) or (-1e-3, 0).

    The plateau values are powers of two: there mix(x, x, a) = x exactly both with an fma and with a product sum, so the six
    taps of a sample whose eight voxels all hold x cancel exactly in float32 and float64 -- the kernel and the transliteration
    see the same flat samples. (At a generic value such as 1.3 both give rounding-noise taps, each with its own direction; the
    defaults of `lo` and `hi` are powers of two for that reason.)"""
    rng = np.random.RandomState(seed)
    axes = [np.linspace(-1.0, 1.0, s) for s in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    m = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
    shell = 0.5 + 0.3 * np.sin(5.1 * x + 0.7) * np.cos(4.3 * y - 0.2) * np.sin(3.7 * z + 1.1) + 0.08 * rng.standard_normal(shape)
    shell = np.clip(shell, 0.1, 0.9)
    vol = np.where(m < 0.26, 0.5, np.where(m < 0.48, shell, np.where(m < 0.72, 0.25, 0.0)))
    vol = np.where((m >= 0.48) & (m < 0.72) & (x > 0.2) & (y > 0.2), hi, vol)
    vol = np.where((m >= 0.48) & (m < 0.72) & (x < -0.2) & (y < -0.2), lo, vol)
    return vol.astype(np.float32)
