"""Float64 (or float32) PyTorch transliteration of the march with a 2-D (value, gradient-magnitude) transfer function, DESIGN.md D12.

The 1-D program of tests/golden/make_autograd_golden.py -- the reference's `raycast` + `get_final_image`, whose helpers are
imported here, not copied -- with one change, the classification:
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


def _trilinear(vol, pos, dtype):
    old = G.F64
    G.F64 = dtype   # the helpers read their float type at call time
    try:
        return G.sample_volume_trilinear(vol, pos)
    finally:
        G.F64 = old


def taps(vol, pos):
    """(dx, dy, dz) (P, 3) of the shading normal, get_volume_normal's central differences."""
    dt = vol.dtype
    d = 1e-3
    out = []
    for axis in range(3):
        e = torch.zeros(3, dtype=dt)
        e[axis] = d
        out.append(_trilinear(vol, pos + e, dt) - _trilinear(vol, pos - e, dt))
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
    """G.raycast with the 2-D classification, for all pixels at once (one view). Returns (P, 4), the live-sample counts,
    a mask of the rays with a live sample whose alpha lies within 1e-5 of 1e-3, and the per-ray count of live flat samples
    (|grad| = 0 exactly).
    nondiff: the non-differentiable march (VR.py:308-361) -- no max_samples clip, samples with alpha <= 1e-3 are counted but
    not composited, unclamped lighting, the result clamped to <= 1."""
    dt = vol.dtype
    P = entry.shape[0]
    tape = torch.zeros((P, 4), dtype=dt)
    count = torch.zeros(P, dtype=torch.long)
    near = torch.zeros(P, dtype=torch.bool)
    nflat = torch.zeros(P, dtype=torch.long)
    ambient, diffuse_k, specular_k, shininess = 0.4, 0.8, 0.3, 32.0
    light_pos = cam + torch.tensor([0.0, 1.0, 0.0], dtype=dt)
    nf = n.to(dt)
    for s in range(int(n.max()) if P else 0):
        active = ((s < n) & (tape[:, 3] < 0.99) & (nondiff or s < max_samples)).detach()
        if not bool(active.any()):
            continue
        ray_len = exit_ - entry
        tmin = entry + 0.5 * ray_len / nf
        frac = torch.where(n > 1, float(s) / torch.clamp(nf - 1.0, min=1.0), torch.zeros_like(nf))
        pos = cam[None, :] + G.mix(tmin, exit_, frac)[:, None] * rays
        pos = torch.where(active[:, None], pos, torch.zeros_like(pos))
        intensity = _trilinear(vol, pos, dt)
        g = taps(vol, pos)
        n2 = (g * g).sum(1)
        flat = (n2 == 0).detach()
        gnorm = torch.where(flat, torch.zeros_like(n2), torch.sqrt(torch.where(flat, torch.ones_like(n2), n2)))
        normal = torch.where(flat[:, None], torch.zeros_like(g), g / torch.where(flat, torch.ones_like(gnorm), gnorm)[:, None])
        u = gnorm * g_scale
        sample_color = classify_2d(tf2d, intensity, u)
        opacity = 1.0 - torch.pow(1.0 - sample_color[:, 3], 1.0 / sampling_rate)
        ld = pos - light_pos[None, :]
        light_dir = ld / ld.norm(dim=1, keepdim=True)
        ndl_raw = (normal * light_dir).sum(1)
        n_dot_l = torch.where(ndl_raw > 0, ndl_raw, torch.zeros_like(ndl_raw))
        r = light_dir - 2.0 * (normal * light_dir).sum(1, keepdim=True) * normal
        rdv_raw = (r * (-rays)).sum(1)
        r_dot_v = torch.where(rdv_raw > 0, rdv_raw, torch.zeros_like(rdv_raw))
        r_dot_v = torch.where(flat, torch.zeros_like(r_dot_v), r_dot_v)
        specular = specular_k * torch.pow(r_dot_v, shininess)
        Lraw = diffuse_k * n_dot_l + specular + ambient
        L = Lraw if nondiff else torch.where(Lraw > 1.0, torch.ones_like(Lraw), Lraw)
        shaded = torch.cat([(L * opacity)[:, None] * sample_color[:, :3], opacity[:, None]], dim=1)
        new = (1.0 - tape[:, 3:4]) * shaded + tape
        near |= active & ((sample_color[:, 3] - 1e-3).abs() < 1e-5).detach()
        lit = (active & (sample_color[:, 3] > 1e-3)) if nondiff else active
        tape = torch.where(lit[:, None], new, tape)
        count = count + active.long()
        nflat = nflat + (active & flat).long()
    if nondiff:
        tape = torch.clamp(tape, max=1.0)
    return tape, count, near, nflat


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
    rgba = np.zeros((V, W, H, 4))
    steps = np.zeros((V, W, H), np.int32)
    near = np.zeros((V, W, H), bool)
    nflat = np.zeros((V, W, H), np.int64)
    total = 0.0
    for v in range(V):
        live = n[v].reshape(-1) > 1
        if pixels is not None:
            live &= pixels[v].reshape(-1)
        sel = torch.from_numpy(np.nonzero(live)[0])
        if sel.numel() == 0:
            continue
        out, cnt, nr, nf = raycast_tf2d(volt[v] if vol.ndim == 4 else volt, tft[v] if tf2d.ndim == 4 else tft, float(g_scale),
                                T(cam[v]), T(entry[v]).reshape(-1)[sel], T(exit_[v]).reshape(-1)[sel],
                                T(rays[v]).reshape(-1, 3)[sel], torch.from_numpy(n[v].astype(np.int64)).reshape(-1)[sel],
                                int(max_samples), float(sampling_rate), nondiff)
        flat = np.zeros((W * H, 4)); flat[sel.numpy()] = out.detach().double().numpy()
        rgba[v] = flat.reshape(W, H, 4)
        st = np.zeros(W * H, np.int32); st[sel.numpy()] = cnt.numpy()
        steps[v] = st.reshape(W, H)
        nm = np.zeros(W * H, bool); nm[sel.numpy()] = nr.numpy()
        near[v] = nm.reshape(W, H)
        fl = np.zeros(W * H, np.int64); fl[sel.numpy()] = nf.numpy()
        nflat[v] = fl.reshape(W, H)
        total = total + (out * T(grad_out[v]).reshape(-1, 4)[sel]).sum()
    res = dict(rgba=rgba, steps=steps, near=near)
    if count_flat:
        res["flat"] = nflat
    if want_grad:
        if torch.is_tensor(total):
            total.backward()
        if want_vol:
            res["dvol"] = volt.grad.double().numpy() if volt.grad is not None else np.zeros(vol.shape)
        res["dtf"] = tft.grad.double().numpy() if tft.grad is not None else np.zeros(tf2d.shape)
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
