"""Float64 / float32 reference of the lit march: the 1-D TF march with a free light and Phong material.

A PyTorch transliteration of the program dr_march_lit_fwd specifies -- `raycast` of tests/golden/make_autograd_golden.py with
its lighting literals (VR.py:91-95, 281-299) replaced by ten parameters per view: the light's world position p and colour lc,
the ambient, diffuse and specular weights ka, kd, ks and the shininess sh. The sample loop (`march`), the trilinear sample, the
normal, the TF lookup and the per-view driver (`render_view`) are imported from that file, not copied; `_shade`, the lighting
under test, is this file's own. The backward is torch.autograd's; nothing is derived by hand. Every ray gets its own
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
    return np.concatenate([cam + np.array(G.LIGHT_OFFSET), np.tile([1.0, 1.0, 1.0, G.AMBIENT, G.DIFFUSE, G.SPECULAR, G.SHININESS],
                                                                    (cam.shape[0], 1))], 1)


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


def _march_lit(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, nondiff, clamp):
    """G.march with _shade's sample. Its per-ray counts: "kink" and "over" (Lraw > 1) over the live samples, or with nondiff
    "band" (alpha within SKIP_BAND of SKIP) over the live samples and "bright" (Lraw > 1) over the composited ones."""
    lc = light[:, 3:6]

    def sample(pos):
        color, opacity, Lraw, flat, m, q = _shade(vol, tf, pos, rays, light, sampling_rate)
        L = torch.where(Lraw > 1.0, torch.ones_like(Lraw), Lraw) if clamp else Lraw
        shaded = torch.cat([(L * opacity)[:, None] * color[:, :3] * lc, opacity[:, None]], dim=1)
        if nondiff:
            return shaded, color[:, 3], dict(band=(color[:, 3] - SKIP).abs() < SKIP_BAND, bright=(color[:, 3] > SKIP) & (Lraw > 1.0))
        kink = ((Lraw - 1.0).abs() < KINK) | (~flat & ((m.abs() < KINK) | (q.abs() < KINK)))
        return shaded, color[:, 3], dict(kink=kink, over=Lraw > 1.0)

    return G.march(cam, entry, exit_, rays, n, max_samples, nondiff, sample)


def raycast_lit(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, clamp=True):
    """The lit march for P rays of one view. light (P, 10): each ray's own copy of the parameters.
    Returns the (P, 4) pixels, the live-sample counts, the rays' `near` flags and their counts of samples with Lraw > 1."""
    out, _, count, c = _march_lit(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, False, clamp)
    return out, count, c["kink"] > 0, c["over"]


def raycast_lit_nondiff(vol, tf, cam, light, entry, exit_, rays, n, sampling_rate):
    """The non-differentiable lit march for P rays of one view, forward only (VR.py:308-361 with light (P, 10) for its literals;
    the lighting is not clamped, :345).
    Returns the (P, 4) pixels min(1, .), the pixels before that clamp, the live-sample counts (every active sample, composited or
    not), the rays' `near` flags (a live sample's alpha within SKIP_BAND of the skip threshold) and, for the tests of the scenes,
    the rays' counts of skipped samples and of composited samples with Lraw > 1."""
    with torch.no_grad():
        out, raw, count, c = _march_lit(vol, tf, cam, light, entry, exit_, rays, n, None, sampling_rate, True, False)
    return out, raw, count, c["band"] > 0, c["skipped"], c["bright"]


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
    views = []
    for v in range(V):
        leaf = T(light[v]).expand(W * H, 10).clone().requires_grad_(want_grad)   # every ray its own copy

        def march_rays(sel):
            args = (vol if vol.ndim == 3 else vol[v], tf if tf.ndim == 2 else tf[v], T(inp["cam"][v]), leaf[sel],
                    T(inp["entry"][v]).reshape(-1)[sel], T(inp["exit"][v]).reshape(-1)[sel], T(inp["rays"][v]).reshape(-1, 3)[sel],
                    torch.from_numpy(np.asarray(inp["n"][v]).reshape(-1)).long()[sel])
            if nondiff:
                out, raw, cnt, nr, sk, br = raycast_lit_nondiff(*args, float(inp["sr"]))
                return out, dict(raw=raw, steps=cnt.int(), near=nr, skipped=sk.int(), bright=br.int())
            out, cnt, nr, cl = raycast_lit(*args, int(inp["max_samples"]), float(inp["sr"]))
            return out, dict(steps=cnt.int(), near=nr, clamped=cl.int())

        loss, res = G.render_view((W, H), np.asarray(inp["n"][v]), None if pixels is None else np.asarray(pixels[v]),
                                  T(inp["grad_out"][v]).reshape(-1, 4) if want_grad else None, march_rays)
        if torch.is_tensor(loss):
            loss.backward()
        if want_grad:
            res["dlight_ray"] = G.grad_or_zero(leaf).reshape(W, H, 10)
        views.append(res)
    res = {k: np.stack([r[k] for r in views]) for k in views[0]}
    if want_grad:
        res.update(dvol=G.grad_or_zero(vol), dtf=G.grad_or_zero(tf), dlight=res["dlight_ray"].reshape(V, W * H, 10).sum(1))
    return res
