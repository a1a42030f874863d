"""The lit march (csrc/march_lit.hip) where the scenes of test_gpu_lighting.py do not reach: the
non-differentiable mode at lights other than the reference's (unclamped lighting, the 1e-3 skip, no max_samples clip, the final
min(1, .)), tables shorter than the backward's reduction scratch, per-view volumes and TFs, shininess 0, 0.5, 1 and 200, zero
material weights, a light inside the box and one far away, images smaller than a tile, and a NaN upstream gradient (D5).
Every comparison is with the float64 transliteration of tests/light_reference.py on the kernels' own ray buffers, by D8's rule
(light_gpu.bound: 3 x the float32 transliteration's own error + 1e-5 of the largest reference element) -- no other tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import light_cases as LC  # noqa: E402
import light_gpu as LG  # noqa: E402
from light_gpu import C, DEV  # noqa: E402

pytestmark = pytest.mark.gpu


# --- 1. the differentiable edge scenes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LC.EDGE_CASES))
def test_edge_scene_against_the_f64_transliteration(hiplib, name):
    sc, st, got = LG.compare(name)
    mask, n = st["mask"], got["n"]
    if name == "sh_half_opaque_sr2":
        assert (got["steps"] < np.minimum(n, sc["max_samples"]))[mask].any()          # a kept ray stops early
    if name.startswith("image_"):
        assert mask.all() and mask.size < 64                                           # less than one wave of rays, all kept
    if len(sc["light"]) > 1:
        rows = got["d_light"]
        assert all(np.abs(rows[a] - rows[b]).max() > 1e-3 * np.abs(rows).max() for a in range(len(rows)) for b in range(a))


# --- 2. tables shorter than the reduction's scratch: each output alone ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["R2", "R6_three_views"])
def test_short_tables_each_output_alone(hiplib, name):
    """R = 2 and 6: TF + double d_tf table take 48 R < 320 B, and the launch must ask for the reduction's 320 B itself; the
    reduction's scratch then overlays the TF and the whole d_tf table. d_light alone, the per-ray output alone and d_tf + d_light
    are what the call with all four outputs gives, within test_nullable_outputs_and_accumulation's bars: 1e-5 of the largest
    element for float atomics, 1e-12 for the f64 sums, bits per ray. (That call is held to the float64 transliteration by
    test_edge_scene_against_the_f64_transliteration.)"""
    fs = LG.forward_state(name)
    sc, vol, tf, cam, light, rays, out = (fs[k] for k in ("sc", "vol", "tf", "cam", "light", "rays", "out"))
    assert 48 * tf.shape[0] < 320
    S, sr = sc["max_samples"], sc["sr"]
    V, (W, H) = cam.shape[0], sc["WH"]
    go = torch.from_numpy(LC.upstream(sc, V)).float().to(DEV)
    new = lambda: (torch.zeros_like(vol), torch.zeros_like(tf), torch.zeros((V, 10), dtype=torch.float64, device=DEV),
                   torch.full((V, W, H, 10), float("nan"), device=DEV))
    run = lambda **outputs: LG.raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, **outputs)
    dv, dt, dl, dr = new()
    run(d_vol=dv, d_tf=dt, d_light=dl, d_ray=dr)
    assert dv.abs().max() > 0 and dt.abs().max() > 0 and (dl != 0).all() and torch.isfinite(dr).all()
    same_sums = lambda a: bool(((a - dl).abs() <= 1e-12 * dl.abs().max(0).values).all())
    _, dt1, dl1, dr1 = new()
    run(d_light=dl1)
    assert same_sums(dl1)
    run(d_ray=dr1)
    assert torch.equal(dr1.view(torch.int32), dr.view(torch.int32))
    dl2 = new()[2]
    run(d_tf=dt1, d_light=dl2)
    assert (dt1 - dt).abs().max() <= 1e-5 * dt.abs().max() and same_sums(dl2)
    assert ((dr.double().sum((1, 2)) - dl).abs() <= 1e-9 * dl.abs().max(0).values).all()   # d_light is the rays' sum


# --- 3. the non-differentiable march ----------------------------------------------------------------------------------------------

def _module_volume(vol):
    """The kernels' (V, VX, VY, VZ) = (V, W, D, H) volume as the user's (BS, 1, D, H, W), contiguous in that layout."""
    return vol.permute(0, 2, 3, 1)[:, None].contiguous()


@pytest.mark.parametrize("name", list(LC.NONDIFF_CASES))
def test_nondiff_scene_against_the_f64_transliteration(hiplib, name):
    """march_lit_fwd(mode=DR_MODE_NONDIFF) on the rays whose live count the f64, the f32 transliteration and the kernel agree on
    and that are not `near` the skip threshold in either precision (at least 80 % of the live rays, asserted by kept_rays)."""
    F, N = LG.functional(), LG.native()
    sc = LC.scene(name)
    vol, tf, cam, light = LG.upload(sc)
    S, sr = sc["max_samples"], sc["sr"]
    rays = F.ray_setup(cam, sc["WH"], vol.shape[-3:], sr, jitter_seed=sc["jitter"])
    out, steps = F.march_lit_fwd(vol, tf, cam, light, *rays, S, sr, mode=N.DR_MODE_NONDIFF)
    e, x, r, n = rays
    inp = LC.inputs(sc, C(e), C(x), C(r), n.cpu().numpy())
    mask, f64, f32 = LC.kept_rays(sc, inp, steps.cpu().numpy())
    m4 = mask[..., None]
    got, got_steps = C(out), steps.cpu().numpy()
    LG.bound(got * m4, f64["rgba"] * m4, f32["rgba"] * m4, "rgba")
    LG.bound((got * m4)[..., :3], (f64["rgba"] * m4)[..., :3], (f32["rgba"] * m4)[..., :3], "rgb")
    assert (got_steps == f64["steps"])[mask].all()
    assert (got <= 1.0).all() and np.isfinite(got).all()
    assert ((f64["skipped"] > 0) & (got[..., 3] > 0))[mask].any()      # kept rays skip samples and composite others
    if name == "nd_thin0_no_clip":
        assert (got_steps > S)[mask].any()                              # no max_samples clip in this mode
    if name == "nd_opaque0_sr4":
        assert (got_steps < inp["n"])[mask].any()                       # early termination
    if name == "nd_overexposed":
        over = mask & (f64["raw"][..., :3].min(-1) > 1.0 + 1e-3)        # all three channels past 1 before the final clamp
        assert over.sum() >= 10 and (got[over][:, :3] == 1.0).all()     # ... come out as exactly 1.0f
    if name == "nd_per_view":
        # the module, with a volume and a TF per item: the functional call's bits
        from differender_amd import _layout as L
        from differender_amd.lighting import RaycasterLit
        VX, VY, VZ = vol.shape[-3:]
        rc = RaycasterLit((VY, VZ, VX), sc["WH"], tf.shape[-2], jitter=True, max_samples=7, headlight=False)
        img = rc.raycast_nondiff(_module_volume(vol), tf.transpose(-1, -2).contiguous(), cam, sampling_rate=sr,
                                 light_pos=light[:, 0:3], light_color=light[:, 3:6], ambient=light[:, 6], diffuse=light[:, 7],
                                 specular=light[:, 8], shininess=light[:, 9])
        assert img.shape == (3, 4, sc["WH"][1], sc["WH"][0])
        assert torch.equal(img.view(torch.int32), L.image(out).view(torch.int32))
        assert all(not torch.equal(img[a], img[b]) for a in range(3) for b in range(a))


# --- 4. D5: a NaN upstream pixel ----------------------------------------------------------------------------------------------------

def test_nan_upstream_gradients_contribute_nothing_to_d_light(hiplib):
    """A quarter of the live rays of a 12x20 scene get a NaN in one channel of their upstream gradient, in all four, and in
    between (test_gpu_pose_edges.py's construction). Their per-ray d_light is 0 -- all ten columns, also d lc_k of a channel whose
    own upstream value is finite and every column of a ray whose NaN sits in alpha alone, which no lighting sum reads -- and
    every other ray's is, to the bit, that of a run where those rays' upstream gradient is 0."""
    F = LG.functional()
    fs = LG.forward_state("R2")
    sc, st, vol, tf, cam, light, out = (fs[k] for k in ("sc", "st", "vol", "tf", "cam", "light", "out"))
    e, x, r, n = fs["rays"]
    S, sr, (W, H) = sc["max_samples"], sc["sr"], sc["WH"]
    assert (W, H) == (12, 20)
    ref, ref32, mask = st["ref"], st["ref32"], st["mask"]
    live = n.cpu().numpy() > 1
    rng = np.random.RandomState(4)
    bad = live & (rng.rand(1, W, H) < 0.25)
    assert (bad & mask).sum() > 20
    chan = rng.rand(1, W, H, 4) < 0.5
    chan[..., 0] |= ~chan.any(-1)
    only = lambda c: (bad & chan[..., c] & ~np.delete(chan, c, -1).any(-1)).sum()
    assert only(0) > 0 and only(3) > 0 and (bad & chan.all(-1)).sum() > 0     # red alone, alpha alone, all four
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    bad_t, chan_t, gm = dev(bad, torch.bool)[..., None], dev(chan, torch.bool), dev(st["gm"], torch.float32)
    g_nan = torch.where(bad_t & chan_t, torch.full_like(gm, float("nan")), gm)
    g_zero = torch.where(bad_t, torch.zeros_like(gm), gm)
    assert bool(torch.isnan(g_nan).any(-1)[dev(bad, torch.bool)].all())

    def run(g):
        """d_light and the per-ray output alone (no d_vol, no d_tf), on the raw entry: the f64 sums as the kernel leaves them."""
        total = torch.zeros((1, 10), dtype=torch.float64, device=DEV)
        ray = torch.full((1, W, H, 10), float("nan"), device=DEV)
        LG.raw_bwd(vol, tf, cam, light, fs["rays"], S, sr, g.contiguous(), out, d_light=total, d_ray=ray)
        return C(total), ray

    total_n, ray_n = run(g_nan)
    want_l = F.march_lit_bwd(vol, tf, cam, light, e, x, r, n, S, sr, g_nan, out, want_vol=False, want_tf=False)
    assert want_l[0] is None and want_l[1] is None and np.abs(C(want_l[2]) - total_n).max() <= 1e-6 * np.abs(total_n).max()
    total_0, ray_0 = run(g_zero)
    assert (C(ray_n)[bad] == 0).all() and torch.isfinite(ray_n).all() and np.isfinite(total_n).all()
    keep = ~dev(bad, torch.bool)
    assert torch.equal(ray_n[keep].view(torch.int32), ray_0[keep].view(torch.int32))
    clean = mask & ~bad
    assert (C(ray_n)[clean] != 0).any(-1).all()
    assert (np.abs(total_n - C(ray_n).sum((1, 2))) <= 1e-9 * np.abs(total_n).max(0)).all()
    m4 = clean[..., None]
    want, want32 = (ref["dlight_ray"] * m4).sum((1, 2)), (ref32["dlight_ray"] * m4).sum((1, 2))
    l1 = (np.abs(ref32["dlight_ray"] - ref["dlight_ray"]) * m4).sum((1, 2)).max(0)
    LG.bound(total_n, want, want32, "dlight under NaN upstream")
    LG.bound(total_n, want, want32, "dlight under NaN upstream by column", per_column=True, err32=l1)


# --- 5. the module with a volume and a TF per item ------------------------------------------------------------------------------------

def test_module_routes_per_item_volume_and_tf_gradients(hiplib):
    """RaycasterLit with a batched volume (BS,1,D,H,W) and TF (BS,4,R) that require grad and per-view lighting tensors: the image
    is march_lit_fwd's on the per-view functional inputs to the bit, and every gradient is march_lit_bwd's -- item b's volume and
    TF get view b's -- within test_module_is_the_functional_calls_and_routes_gradients' bar."""
    from differender_amd import _layout as L
    from differender_amd.lighting import RaycasterLit
    F = LG.functional()
    sc = LC.scene("per_view_inputs")
    vol, tf, cam, light = LG.upload(sc)
    BS, (VX, VY, VZ), WH = vol.shape[0], vol.shape[-3:], sc["WH"]
    rc = RaycasterLit((VY, VZ, VX), WH, tf.shape[-2], jitter=False, max_samples=4096, headlight=False)
    vg = _module_volume(vol).requires_grad_(True)
    tg = tf.transpose(-1, -2).contiguous().requires_grad_(True)
    parts = [light[:, 0:3], light[:, 3:6], light[:, 6], light[:, 7], light[:, 8], light[:, 9]]
    pos, col, ka, kd, ks, sh = (p.clone().requires_grad_(True) for p in parts)
    img = rc(vg, tg, cam, light_pos=pos, light_color=col, ambient=ka, diffuse=kd, specular=ks, shininess=sh)
    go = torch.randn(img.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (img * go).sum().backward()

    fvol = L.field_view(vg.detach())
    rays = F.ray_setup(cam, WH, fvol.shape[-3:], 1.0)
    out, _ = F.march_lit_fwd(fvol, tf, cam, light, *rays, 4096, 1.0)
    assert img.shape == (BS, 4, WH[1], WH[0]) and torch.equal(L.image(out).view(torch.int32), img.detach().view(torch.int32))
    g_k = torch.flip(go.transpose(-1, -3), (-2,)).contiguous()        # the user image's gradient in the kernels' (W,H,4) layout
    dv, dt, dl = F.march_lit_bwd(fvol, tf, cam, light, *rays, 4096, 1.0, g_k, out)
    close = lambda a, b: (a - b).abs().max() <= 1e-5 * b.abs().max()
    assert dv.shape == (BS, VX, VY, VZ) and dt.shape == tf.shape
    assert close(L.field_view(vg.grad), dv) and close(tg.grad, dt.transpose(-1, -2))
    for b in range(BS):
        assert close(L.field_view(vg.grad)[b], dv[b]) and close(tg.grad[b], dt[b].t())
        for a in range(b):
            assert not close(vg.grad[a], vg.grad[b]) and not close(tg.grad[a], tg.grad[b])
    assert close(pos.grad, dl[:, 0:3]) and close(col.grad, dl[:, 3:6])
    for t, k in ((ka, 6), (kd, 7), (ks, 8), (sh, 9)):
        assert t.grad.shape == (BS,) and close(t.grad, dl[:, k]) and (t.grad != 0).all()
