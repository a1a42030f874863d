"""Float64 / float32 reference of the lit march: the 1-D TF march with a free light and Phong material.

A PyTorch transliteration of the program dr_march_lit_fwd specifies -- `raycast` of tests/golden/make_autograd_golden.py with
its lighting literals (VR.py:91-95, 281-299) replaced by ten parameters per view: the light's world position p and colour lc,
the ambient, diffuse and specular weights ka, kd, ks and the shininess sh. The trilinear sample, the normal and the TF lookup
are imported from that file, not copied. The backward is torch.autograd's; nothing is derived by hand. Every ray gets its own
leaf copy of its view's ten parameters, so one run holds each ray's contribution to d_light as well as the views' totals.

Branch predicates are frozen as in make_autograd_golden.py: max(x, 0) passes the gradient iff 0 < x, min(1, L) iff not 1 < L.
`near` flags the rays with a live sample within 1e-4 of one of these kinks (Lraw = 1; n.l = 0 or r.v = 0 on a sample with a
normal), where the gradient is discontinuous and two precisions may stand on different sides.

raycast_lit_nondiff is the non-differentiable march (dr_march_lit_fwd with DR_MODE_NONDIFF), forward only: `raycast_nondiff` of
tests/golden/make_setup_nondiff_golden.py (VR.py:308-361) with the same ten parameters in place of its literals. Every active
sample is counted, but composited only where the TF's alpha is > 1e-3; the lighting is not clamped; there is no max_samples clip;
the pixel is min(1, .). The lighting kinks do not matter there (no gradient, and the forward is continuous across them); the
skip threshold does, and `near` flags the rays with a live sample whose alpha lies within SKIP_BAND of it.

vol and tf may carry a leading view axis ((V, VX, VY, VZ), (V, R, 4)): view v then reads its own, and dvol / dtf come back
with the same axis.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))

import make_autograd_golden as G  # noqa: E402

KINK = 1e-4
SKIP = 1e-3        # VR.py:334: the non-differentiable march composites a sample only where its alpha is > 1e-3
# the alpha is a lerp x (1 - a) + y a of table entries <= 1: three float32 roundings of values <= 1, at most 1.5 x 2^-23 = 1.8e-7
# with the fraction's own error of a few ulp on top. Ten times that: inside the band, float32 and float64 may stand on
# different sides of the threshold.
SKIP_BAND = 1e-6


def reference_light(cam):
    """The reference's lighting for the cameras cam (views, 3) as (views, 10) rows: a white light at look_from + (0, 1, 0),
    0.4, 0.8, 0.3, 32."""
    cam = np.asarray(cam, np.float64).reshape(-1, 3)
    return np.concatenate([cam + np.array([0.0, 1.0, 0.0]), np.tile([1.0, 1.0, 1.0, 0.4, 0.8, 0.3, 32.0], (cam.shape[0], 1))], 1)


def _shade(vol, tf, pos, rays, light, sampling_rate):
    """One sample per ray at pos: the classified colour (P, 4), its opacity at this rate, the unclamped Phong term Lraw, the
    flat-normal flag and the two dot products m = n.l and q = r.v the kinks hang on."""
    p = light[:, 0:3]
    ka, kd, ks, sh = light[:, 6], light[:, 7], light[:, 8], light[:, 9]
    intensity = G.sample_volume_trilinear(vol, pos)
    color = G.apply_transfer_function(tf, intensity)
    opacity = 1.0 - torch.pow(1.0 - color[:, 3], 1.0 / sampling_rate)
    normal, flat = G.get_volume_normal(vol, pos)
    lv = pos - p
    ld = lv / lv.norm(dim=1, keepdim=True)
    m = (normal * ld).sum(1)
    ndl = torch.where(m > 0, m, torch.zeros_like(m))
    rf = ld - 2.0 * m[:, None] * normal
    q = (rf * (-rays)).sum(1)
    rdv = torch.where((q > 0) & ~flat, q, torch.zeros_like(q))       # flat normal: ndl = rdv = 0 (D1)
    lit = (rdv > 0).detach()
    spec_pow = torch.where(lit, torch.pow(torch.where(lit, rdv, torch.ones_like(rdv)), sh), torch.zeros_like(rdv))
    return color, opacity, kd * ndl + ks * spec_pow + ka, flat, m, q


def _sample_pos(cam, entry, exit_, rays, n, nf, s, active):
    tmin = entry + 0.5 * (exit_ - entry) / nf
    frac = torch.where(n > 1, float(s) / torch.clamp(nf - 1.0, min=1.0), torch.zeros_like(nf))
    pos = cam[None, :] + G.mix(tmin, exit_, frac)[:, None] * rays
    return torch.where(active[:, None], pos, torch.zeros_like(pos))


def raycast_lit(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, clamp=True):
    """The lit march for P rays of one view. light (P, 10): each ray's own copy of the parameters.
    Returns the (P, 4) pixels, the live-sample counts, the rays' `near` flags and their counts of samples with Lraw > 1."""
    dt = entry.dtype
    P = entry.shape[0]
    tape = torch.zeros((P, 4), dtype=dt)
    count = torch.zeros(P, dtype=torch.long)
    near = torch.zeros(P, dtype=torch.bool)
    clamped = torch.zeros(P, dtype=torch.long)
    lc = light[:, 3:6]
    nf = n.to(dt)
    for s in range(int(n.max())):
        active = ((s < n) & (tape[:, 3] < 0.99) & (s < max_samples)).detach()
        if not bool(active.any()):
            continue
        pos = _sample_pos(cam, entry, exit_, rays, n, nf, s, active)
        color, opacity, Lraw, flat, m, q = _shade(vol, tf, pos, rays, light, sampling_rate)
        L = torch.where(Lraw > 1.0, torch.ones_like(Lraw), Lraw) if clamp else Lraw
        shaded = torch.cat([(L * opacity)[:, None] * color[:, :3] * lc, opacity[:, None]], dim=1)
        new = (1.0 - tape[:, 3:4]) * shaded + tape
        tape = torch.where(active[:, None], new, tape)
        count = count + active.long()
        kink = ((Lraw - 1.0).abs() < KINK) | (~flat & ((m.abs() < KINK) | (q.abs() < KINK)))
        near = near | (active & kink.detach())
        clamped = clamped + (active & (Lraw > 1.0).detach()).long()
    return tape, count, near, clamped


def raycast_lit_nondiff(vol, tf, cam, light, entry, exit_, rays, n, sampling_rate):
    """The non-differentiable lit march for P rays of one view, forward only (VR.py:308-361 with light (P, 10) for its literals).
    Returns the (P, 4) pixels min(1, .), the pixels before that clamp, the live-sample counts (every active sample, composited or
    not), the rays' `near` flags (a live sample's alpha within SKIP_BAND of the skip threshold) and, for the tests of the scenes,
    the rays' counts of skipped samples and of composited samples with Lraw > 1."""
    dt = entry.dtype
    P = entry.shape[0]
    tape = torch.zeros((P, 4), dtype=dt)
    count = torch.zeros(P, dtype=torch.long)
    near = torch.zeros(P, dtype=torch.bool)
    skipped = torch.zeros(P, dtype=torch.long)
    bright = torch.zeros(P, dtype=torch.long)
    lc = light[:, 3:6]
    nf = n.to(dt)
    with torch.no_grad():
        for s in range(int(n.max())):
            active = (s < n) & (tape[:, 3] < 0.99)                       # no max_samples clip (VR.py:317-318)
            if not bool(active.any()):
                continue
            pos = _sample_pos(cam, entry, exit_, rays, n, nf, s, active)
            color, opacity, Lraw, _, _, _ = _shade(vol, tf, pos, rays, light, sampling_rate)
            shade = active & (color[:, 3] > SKIP)                        # VR.py:334
            shaded = torch.cat([(Lraw * opacity)[:, None] * color[:, :3] * lc, opacity[:, None]], dim=1)   # not clamped (:345)
            new = (1.0 - tape[:, 3:4]) * shaded + tape
            tape = torch.where(shade[:, None], new, tape)
            count = count + active.long()
            near = near | (active & ((color[:, 3] - SKIP).abs() < SKIP_BAND))
            skipped = skipped + (active & ~shade).long()
            bright = bright + (shade & (Lraw > 1.0)).long()
    return torch.clamp(tape, max=1.0), tape, count, near, skipped, bright


def run(inp, light, dtype=torch.float64, want_grad=True, pixels=None, mode="diff"):
    """inp: vol (VX,VY,VZ), tf (R,4) (both shared by the views) or vol (V,VX,VY,VZ), tf (V,R,4) (each view its own), cam (V,3),
    entry, exit, n (V,W,H), rays (V,W,H,3), grad_out (V,W,H,4), sr, max_samples; light (V,10). The forward runs in `dtype`.
    Returns rgba (V,W,H,4), steps, near and clamped (the ray's samples with Lraw > 1) (V,W,H), and with want_grad dvol, dtf (with
    the views' axis where the input has it), dlight_ray (V,W,H,10) and dlight (V,10), as float64 numpy arrays. Rays with n <= 1
    (0/0 in the reference, H6) render 0 and contribute nothing; pixels (V,W,H) bool: only these rays are marched.
    mode "nondiff": raycast_lit_nondiff, forward only (grad_out and max_samples are not read) -> rgba, raw (rgba before the final
    min(1, .)) (V,W,H,4), steps, near, skipped, bright (V,W,H)."""
    assert mode in ("diff", "nondiff")
    nondiff = mode == "nondiff"
    want_grad = want_grad and not nondiff
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    V, W, H = np.asarray(inp["n"]).shape
    vol, tf = T(inp["vol"]).requires_grad_(want_grad), T(inp["tf"]).requires_grad_(want_grad)
    assert vol.ndim in (3, 4) and tf.ndim in (2, 3) and (vol.ndim == 3 or vol.shape[0] == V) and (tf.ndim == 2 or tf.shape[0] == V)
    rgba = np.zeros((V, W * H, 4)); raw = np.zeros((V, W * H, 4))
    ints = {k: np.zeros((V, W * H), np.int32) for k in (("steps", "skipped", "bright") if nondiff else ("steps", "clamped"))}
    near = np.zeros((V, W * H), bool)
    dray = np.zeros((V, W * H, 10))
    old = G.F64
    G.F64 = dtype   # the imported helpers read their float type at call time
    try:
        for v in range(V):
            n = torch.from_numpy(np.asarray(inp["n"][v]).reshape(-1)).long()
            live = n > 1
            if pixels is not None:
                live &= torch.from_numpy(np.asarray(pixels[v]).reshape(-1))
            sel = torch.nonzero(live)[:, 0]
            if sel.numel() == 0:
                continue
            leaf = T(light[v]).expand(sel.numel(), 10).clone().requires_grad_(want_grad)
            args = (vol if vol.ndim == 3 else vol[v], tf if tf.ndim == 2 else tf[v], T(inp["cam"][v]), leaf,
                    T(inp["entry"][v]).reshape(-1)[sel], T(inp["exit"][v]).reshape(-1)[sel], T(inp["rays"][v]).reshape(-1, 3)[sel],
                    n[sel])
            if nondiff:
                out, pre, cnt, nr, sk, br = raycast_lit_nondiff(*args, float(inp["sr"]))
                raw[v, sel.numpy()] = pre.double().numpy()
                counts = dict(steps=cnt, skipped=sk, bright=br)
            else:
                out, cnt, nr, cl = raycast_lit(*args, int(inp["max_samples"]), float(inp["sr"]))
                counts = dict(steps=cnt, clamped=cl)
            rgba[v, sel.numpy()] = out.detach().double().numpy()
            near[v, sel.numpy()] = nr.numpy()
            for k, c in counts.items():
                ints[k][v, sel.numpy()] = c.numpy()
            if want_grad:
                (out * T(inp["grad_out"][v]).reshape(-1, 4)[sel]).sum().backward()
                dray[v, sel.numpy()] = leaf.grad.double().numpy()
    finally:
        G.F64 = old
    res = dict(rgba=rgba.reshape(V, W, H, 4), near=near.reshape(V, W, H), **{k: a.reshape(V, W, H) for k, a in ints.items()})
    if nondiff:
        res["raw"] = raw.reshape(V, W, H, 4)
    if want_grad:
        zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
        res.update(dvol=zero(vol), dtf=zero(tf), dlight_ray=dray.reshape(V, W, H, 10),
                   dlight=dray.sum(1))
    return res

