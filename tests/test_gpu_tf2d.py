"""2-D (value, gradient-magnitude) transfer functions on the GPU (csrc/march_tf2d.hip): bit-exact against the
1-D baseline kernels with a one-column table, against the float64 transliteration (tests/tf2d_reference.py) with tables that
vary along the gradient axis, every LDS tier, the meaning of the gradient axis, Raycaster2D, a full-size run and the example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tf2d_reference as R2  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _F():
    from differender_amd import functional as F
    return F


def _N():
    from differender_amd import _native as N
    return N


def _volume(shape, seed=0, views=None):
    """Field-order (VX, VY, VZ) volume with structure at every scale: smooth blobs plus noise, in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    lead = () if views is None else (views,)
    axes = [torch.linspace(-1.0, 1.0, s) for s in shape]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    v = 0.5 + 0.3 * torch.sin(3.1 * x + 1.3) * torch.cos(2.3 * y - 0.4) * torch.sin(1.7 * z + 0.9)
    v = v + 0.4 * torch.exp(-8.0 * ((x - 0.2) ** 2 + (y + 0.1) ** 2 + z ** 2))
    v = v.expand(*lead, *shape) + 0.05 * torch.randn(*lead, *shape, generator=g)
    return v.clamp(0.0, 1.0).contiguous().to(DEV)


# alphas of the rows of a "skip" table: exact zeros, and values just below, at and just above the non-differentiable march's
# threshold 1e-3 (the early skip of march_tf2d.hip must leave exactly the samples the plain test leaves), next to zero rows
# and live rows so that samples lerp between them
SKIP_ROWS = (0.0, 0.0, 9.9999e-4, 0.0, 1e-3, 0.0, 1.0001e-3, 0.0, 0.3, 0.0, 9.9999e-4, 9.9999e-4, 0.5, 0.0, 1.0001e-3, 0.2)


def _tf1d(R, kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    tf = torch.rand((R, 4), generator=g) * 0.9 + 0.05
    if kind == "skip":
        tf[:, 3] = torch.tensor([SKIP_ROWS[k % len(SKIP_ROWS)] for k in range(R)])
    else:
        tf[:, 3] = torch.linspace(0.01, 0.06, R) if kind == "thin" else torch.linspace(0.0, 0.95, R) ** 2 + 0.05
    return tf.to(DEV)


def _tf2d(RV, RG, kind, seed=0, views=None):
    g = torch.Generator().manual_seed(seed)
    lead = () if views is None else (views,)
    tf = torch.rand((*lead, RV, RG, 4), generator=g) * 0.9 + 0.05
    ramp = torch.linspace(0.0, 1.0, RG)
    if kind == "thin":
        tf[..., 3] = 0.01 + 0.07 * torch.rand((*lead, RV, RG), generator=g) * ramp
    else:
        tf[..., 3] = 0.05 + 0.9 * torch.rand((*lead, RV, RG), generator=g) * ramp
    return tf.contiguous().to(DEV)


def _cams(views, first=0.9):
    from differender.utils import in_circles
    return torch.stack([in_circles(first + 1.7 * i).float() for i in range(views)]).to(DEV)


def _g_scale(vol):
    from differender_amd.tf2d import gradient_scale
    return gradient_scale(vol if vol.ndim == 3 else vol[0], q=0.9)


# --- 1. bit-exact anchor -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [0.7, 1.0, 2.0, 8.0])
@pytest.mark.parametrize("jitter", [0, 977], ids=["nojit", "jit"])
@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_one_gradient_column_is_the_1d_baseline_bit_for_bit(hiplib, sr, jitter, vdt):
    F, N = _F(), _N()
    vol = _volume((28, 24, 32), seed=1).to(vdt)
    cam = _cams(2)
    e, x, r, n = F.ray_setup(cam, (24, 20), vol.shape, sr, jitter_seed=jitter)
    S = 4096
    for kind in ("thin", "opaque", "skip"):   # (opaque: rays terminate early; skip: alphas around the NONDIFF threshold)
        tf = _tf1d(16, kind, seed=2)
        for mode in (N.DR_MODE_DIFF, N.DR_MODE_NONDIFF):
            ref, ref_steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, mode=mode, variant=N.DR_VARIANT_BASELINE,
                                         workspace=None, hints=0)
            out, steps = F.march_tf2d_fwd(vol, tf[:, None, :].contiguous(), cam, e, x, r, n, S, sr, 2.5, mode=mode)
            torch.cuda.synchronize()
            assert torch.equal(steps, ref_steps), (kind, mode)
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (kind, mode)
            if kind == "opaque" and sr >= 1.0:
                assert (ref_steps < n).any()
            if kind == "skip" and mode == N.DR_MODE_NONDIFF:
                assert (ref[..., 3] > 0).any() and (ref[..., 3] < 0.9).any()
        # the backward: the same f32 addends in another order (float atomics). An element is a sum of k of them, so the two
        # differ by at most ~k ulp of the sum of their magnitudes; 1e-5 of the largest element bounds that here (k < 1e3)
        g = torch.randn((2, 24, 20, 4), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        out, _ = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0)
        dv0, dt0 = F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out, variant=N.DR_VARIANT_BASELINE, workspace=None)
        dv1, dt1 = F.march_tf2d_bwd(vol, tf[:, None, :].contiguous(), cam, e, x, r, n, S, sr, 2.5, g, out)
        assert (dv1 - dv0).abs().max() <= 1e-5 * dv0.abs().max()
        assert (dt1[:, 0] - dt0).abs().max() <= 1e-5 * dt0.abs().max()


# --- 2. against the float64 transliteration -----------------------------------------------------------------------------------

def _reference(vol, tf2d, cam, WH, S, sr, g_scale, jitter=0, seed=0, count_flat=False):
    """The GPU forward and the f64 / f32 transliterations on the GPU's own ray buffers, for _compare and _assert_close. Rays whose
    f32 live-sample count differs from the f64 one are masked (zero upstream gradient `gm`, not compared)."""
    F = _F()
    V = cam.shape[0]
    e, x, r, n = F.ray_setup(cam, WH, vol.shape[-3:], sr, jitter_seed=jitter)
    out, steps = F.march_tf2d_fwd(vol, tf2d, cam, e, x, r, n, S, sr, g_scale)
    C = lambda t: t.detach().double().cpu().numpy()
    host = dict(vol=C(vol.float()), tf2d=C(tf2d), cam=C(cam), entry=C(e), exit_=C(x), rays=C(r), n=n.cpu().numpy())
    go = torch.randn((V, *WH, 4), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()
    args = lambda g: (host["vol"], host["tf2d"], g_scale, host["cam"], host["entry"], host["exit_"], host["rays"], host["n"], g,
                      S, sr)
    ref = R2.run(*args(go), want_grad=False)
    ref32 = R2.run(*args(go), dtype=torch.float32, want_grad=False)
    mask = (steps.cpu().numpy() == ref["steps"]) & (ref32["steps"] == ref["steps"]) & (host["n"] > 1)
    assert mask.sum() >= 0.8 * (host["n"] > 1).sum()
    gm = go * mask[..., None]
    ref = R2.run(*args(gm), pixels=mask, count_flat=count_flat)
    ref32 = R2.run(*args(gm), dtype=torch.float32, pixels=mask)
    return dict(ref=ref, ref32=ref32, mask=mask, host=host, rays=(e, x, r, n), out=out,
                gm=torch.from_numpy(gm).float().to(DEV))


def _assert_close(got, st, k, floor=1e-5):
    """got (a float64 numpy array) against st["ref"][k] ("rgba", "dvol" or "dtf"): the bar is 3x the f32 transliteration's own
    error, with a floor of `floor` x the largest reference element."""
    mask = st["mask"]
    m = mask[..., None] if k == "rgba" else 1
    want = st["ref"][k] * m
    err = np.abs(got * m - want).max()
    err32 = np.abs(st["ref32"][k] * m - want).max()
    scale = np.abs(want).max()
    assert scale > 0, k
    assert err <= 3.0 * err32 + floor * scale, (k, err / scale, err32 / scale)


def _compare(vol, tf2d, cam, WH, S, sr, g_scale, jitter=0, seed=0, floor=1e-5, count_flat=False):
    """GPU forward + backward against the f64 transliteration on the GPU's own ray buffers (_reference, _assert_close)."""
    F = _F()
    st = _reference(vol, tf2d, cam, WH, S, sr, g_scale, jitter, seed, count_flat)
    d_vol, d_tf = F.march_tf2d_bwd(vol, tf2d, cam, *st["rays"], S, sr, g_scale, st["gm"], st["out"])
    C = lambda t: t.detach().double().cpu().numpy()
    for k, got in (("rgba", C(st["out"])), ("dvol", C(d_vol)), ("dtf", C(d_tf))):
        _assert_close(got, st, k, floor)
    return st["ref"], st["mask"], st["host"]


CASES = {
    # name: (volume shape, views of volume/TF (None: shared), image, RV, RG, tf kind, sr, max_samples, jitter, vol dtype)
    "ert": ((20, 18, 22), (None, None), (16, 16), 12, 7, "opaque", 2.0, 4096, 0, torch.float32),
    "clip": ((24, 24, 24), (None, None), (12, 16), 8, 6, "thin", 1.0, 23, 0, torch.float32),
    "jitter": ((18, 22, 16), (None, None), (16, 16), 10, 5, "opaque", 1.0, 4096, 4242, torch.float32),
    "nonsquare": ((16, 20, 16), (None, None), (20, 12), 8, 9, "thin", 1.0, 4096, 0, torch.float32),
    "f16": ((20, 20, 20), (None, None), (16, 16), 8, 6, "opaque", 1.0, 4096, 0, torch.float16),
    "views3": ((16, 18, 20), (3, 3), (12, 12), 8, 6, "opaque", 1.0, 4096, 0, torch.float32),
    "shared_tf": ((16, 18, 20), (3, None), (12, 12), 8, 6, "thin", 1.0, 4096, 0, torch.float32),
    # one volume, a table per view: d_vol sums over the views, d_tf2d stays per view
    "shared_vol": ((16, 18, 20), (None, 3), (12, 12), 8, 6, "opaque", 1.0, 4096, 0, torch.float32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_f64_transliteration(hiplib, name):
    vshape, (vv, tv), WH, RV, RG, kind, sr, S, jit, vdt = CASES[name]
    vol = _volume(vshape, seed=3, views=vv).to(vdt)
    tf = _tf2d(RV, RG, kind, seed=4, views=tv)
    V = 3 if (vv or tv) else 1
    ref, mask, host = _compare(vol, tf, _cams(V), WH, S, sr, _g_scale(vol.float()), jitter=jit)
    if name == "ert":
        assert (ref["steps"] < np.minimum(host["n"], S))[mask].any()
    if name == "clip":
        assert (host["n"] > S).any()


# --- 3. the LDS tiers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("RV,RG", [(64, 53), (64, 54), (128, 80)], ids=["P3392", "P3456", "P10240"])
def test_every_lds_tier(hiplib, RV, RG):
    vol = _volume((20, 20, 20), seed=6)
    _compare(vol, _tf2d(RV, RG, "opaque", seed=7), _cams(1), (16, 16), 4096, 1.0, _g_scale(vol))


# --- 3b. the non-differentiable march with RG > 1 ------------------------------------------------------------------------------

@pytest.mark.parametrize("RV,RG", [(16, 6), (128, 80)], ids=["lds_skip", "global"])
def test_nondiff_against_the_f64_transliteration(hiplib, RV, RG):
    """NONDIFF with tables that vary along u, against the transliteration's non-differentiable march. (16, 6) stages the table
    in LDS and skips the taps of samples whose two value rows are both dead (every alpha of rows 4m and 4m + 1 is 0 or below
    1e-3: 0, 5e-4 or 9.9e-4 along u), beside live rows whose alphas grow with u; (128, 80) reads the table where it lies and
    skips nothing. The threshold's own bits are the anchor's (above); here rays with a sample within 1e-5 of alpha 1e-3 in f64
    are left out (f32 and f64 may take the threshold apart), as are rays whose live-sample counts differ."""
    vol = _volume((20, 18, 22), seed=15)
    tf = _tf2d(RV, RG, "opaque", seed=16)
    dead = torch.tensor([k % 4 in (0, 1) for k in range(RV)], device=DEV)
    level = torch.tensor([(0.0, 9.9e-4, 5e-4)[k % 3] for k in range(RV)], device=DEV)
    tf[..., 3] = torch.where(dead[:, None], level[:, None].expand(RV, RG), tf[..., 3])
    tf[dead, 0, 3] = 0.0
    tf = tf.contiguous()
    ref, mask = _compare_nondiff(vol, tf, _cams(2), (16, 14), 2.0, _g_scale(vol))
    assert (ref["steps"] > 64).any()                  # the non-differentiable march has no max_samples clip


def _compare_nondiff(vol, tf, cam, WH, sr, g_scale, S=64):
    """The NONDIFF march against the transliteration's, on the GPU's own ray buffers. Rays with a sample within 1e-5 of alpha
    1e-3 in f64 or f32 are left out, as are rays whose live-sample counts differ. Returns the f64 result and the compared rays."""
    F, N = _F(), _N()
    e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
    out, steps = F.march_tf2d_fwd(vol, tf, cam, e, x, r, n, S, sr, g_scale, mode=N.DR_MODE_NONDIFF)   # (no clip)
    C = lambda t: t.detach().double().cpu().numpy()
    host = (C(vol), C(tf), g_scale, C(cam), C(e), C(x), C(r), n.cpu().numpy())
    go = np.zeros((cam.shape[0], *WH, 4))
    ref = R2.run(*host, go, S, sr, want_grad=False, nondiff=True)
    ref32 = R2.run(*host, go, S, sr, dtype=torch.float32, want_grad=False, nondiff=True)
    mask = (C(steps) == ref["steps"]) & (ref32["steps"] == ref["steps"]) & ~ref["near"] & ~ref32["near"] & (host[-1] > 1)
    assert mask.sum() >= 0.8 * (host[-1] > 1).sum()
    want = ref["rgba"][mask]
    assert (want[:, 3] > 0).any() and (want[:, 3] < 0.99).any()
    err = np.abs(C(out)[mask] - want).max()
    err32 = np.abs(ref32["rgba"][mask] - want).max()
    assert err <= 3.0 * err32 + 1e-5 * np.abs(want).max(), (err, err32)
    return ref, mask


# --- 4. the meaning of the gradient axis ------------------------------------------------------------------------------------

def test_gradient_axis_is_the_scaled_gradient_magnitude(hiplib):
    """A ramp along x (one value per voxel: |dv| per voxel = 1) seen along z; a table constant along the value axis with
    r = the gradient coordinate and g = 1: C_r / C_g is the u of every sample, 1e-3 (VX - 1 - 1e-4) g_scale.
    (The f32 tap positions put ~5e-5 of relative noise on u; at u = 0.1 that is within the 1e-5 asked.)"""
    F = _F()
    VX = 16
    vol = torch.arange(VX, dtype=torch.float32)[:, None, None].expand(VX, 16, 16).contiguous().to(DEV)
    u = 0.1
    g_scale = u / (1e-3 * (VX - 1 - 1e-4))
    RV, RG = 4, 33
    tf = torch.zeros((RV, RG, 4))
    tf[..., 0] = torch.linspace(0.0, 1.0, RG)
    tf[..., 1] = 1.0
    tf[..., 2] = 0.5
    tf[..., 3] = 0.05
    cam = torch.tensor([[0.0, 0.0, 3.0]], device=DEV)
    e, x, r, n = F.ray_setup(cam, (16, 16), vol.shape, 1.0)
    out, _ = F.march_tf2d_fwd(vol, tf.to(DEV), cam, e, x, r, n, 4096, 1.0, g_scale)
    c = out[0, 6:10, 6:10].double().cpu()
    assert (c[..., 1] > 0.05).all()
    ratio = c[..., 0] / c[..., 1]
    assert (ratio - u).abs().max() <= 1e-5, ratio


# --- 5. Raycaster2D ----------------------------------------------------------------------------------------------------------

def test_raycaster2d_matches_the_functional_calls(hiplib):
    from differender_amd.tf2d import Raycaster2D
    F = _F()
    D, H, W = 18, 20, 22
    vol_user = _volume((D, H, W), seed=8)[None].requires_grad_(True)       # (1, D, H, W)
    tf_user = _tf2d(8, 6, "opaque", seed=9).permute(2, 0, 1).contiguous().requires_grad_(True)   # (4, RV, RG)
    lf = _cams(1)[0]
    g_scale = _g_scale(vol_user.detach()[0])
    rc = Raycaster2D((D, H, W), (24, 16), (8, 6), g_scale, jitter=False)
    img = rc(vol_user, tf_user, lf)
    assert img.shape == (4, 16, 24)
    img2 = rc(vol_user, tf_user, lf)
    assert torch.equal(img, img2)   # two forward runs are bitwise equal
    G = torch.randn(img.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    (img * G).sum().backward()
    vol_f = vol_user.detach().squeeze(0).permute(2, 0, 1)                  # (W, D, H): the field view
    tf_f = tf_user.detach().permute(1, 2, 0).contiguous()
    e, x, r, n = F.ray_setup(lf[None], (24, 16), vol_f.shape, 1.0)
    out, _ = F.march_tf2d_fwd(vol_f, tf_f, lf[None], e, x, r, n, 512, 1.0, g_scale)
    assert torch.equal(rc._image(out[0], False), img.detach())
    o = out[0].clone().requires_grad_(True)
    rc._image(o, False).backward(G)
    dv, dt = F.march_tf2d_bwd(vol_f, tf_f, lf[None], e, x, r, n, 512, 1.0, g_scale, o.grad[None], out)
    dv_user = dv.permute(1, 2, 0)[None]
    dt_user = dt.permute(2, 0, 1)
    assert (vol_user.grad - dv_user).abs().max() <= 1e-5 * dv_user.abs().max()
    assert (tf_user.grad - dt_user).abs().max() <= 1e-5 * dt_user.abs().max()
    with pytest.raises(ValueError, match="Raycaster"):
        rc(vol_user, tf_user, lf.clone().requires_grad_(True))


def test_raycaster2d_shares_an_unbatched_volume_and_table_among_batched_cameras(hiplib):
    """A shared (1, D, H, W) volume and (4, RV, RG) table with look_from (2, 3), on a 9 x 10 x 11 volume and an 11 x 13 image (no
    multiple of the 8 x 8 tile): image and live-sample counts are bit for bit the functional calls' on the explicitly permuted
    views, the shared inputs receive one gradient summed over both views. (The gradients are sums of atomics whose order varies
    from run to run: compared at the bar of test_raycaster2d_matches_the_functional_calls, not bit for bit.)"""
    from differender_amd.tf2d import Raycaster2D
    F = _F()
    D, H, W, WH = 9, 10, 11, (11, 13)
    vol_user = _volume((D, H, W), seed=12)[None].requires_grad_(True)       # (1, D, H, W)
    tf_user = _tf2d(8, 6, "opaque", seed=13).permute(2, 0, 1).contiguous().requires_grad_(True)   # (4, RV, RG)
    lf = _cams(2)
    g_scale = _g_scale(vol_user.detach()[0])
    rc = Raycaster2D((D, H, W), WH, (8, 6), g_scale, jitter=False)
    img = rc(vol_user, tf_user, lf)
    assert img.shape == (2, 4, 13, 11)
    vol_f = vol_user.detach().squeeze(0).permute(2, 0, 1)                  # (W, D, H): the field view
    tf_f = tf_user.detach().permute(1, 2, 0).contiguous()
    e, x, r, n = F.ray_setup(lf, WH, vol_f.shape, 1.0)
    out, steps = F.march_tf2d_fwd(vol_f, tf_f, lf, e, x, r, n, 512, 1.0, g_scale)
    assert torch.equal(img.detach(), torch.flip(out, (2,)).permute(0, 3, 2, 1)) and torch.equal(rc._steps, steps)
    G = torch.randn(img.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    (img * G).sum().backward()
    gk = torch.flip(G.permute(0, 3, 2, 1), (2,))
    dv, dt = F.march_tf2d_bwd(vol_f, tf_f, lf, e, x, r, n, 512, 1.0, g_scale, gk, out)
    dv_user = dv.permute(1, 2, 0)[None]
    dt_user = dt.permute(2, 0, 1)
    assert vol_user.grad.shape == vol_user.shape and tf_user.grad.shape == tf_user.shape
    assert (vol_user.grad - dv_user).abs().max() <= 1e-5 * dv_user.abs().max()
    assert (tf_user.grad - dt_user).abs().max() <= 1e-5 * dt_user.abs().max()


@pytest.mark.parametrize("batched", [False, True])
def test_raycaster2d_with_one_gradient_column_renders_what_raycaster_renders(hiplib, batched):
    from differender_amd.tf2d import Raycaster2D
    from differender_amd.volume_raycaster import Raycaster
    D, H, W, R = 20, 18, 24, 16
    vol = _volume((D, H, W), seed=10)[None]
    tf = _tf1d(R, "opaque", seed=11).t().contiguous()                       # (4, R)
    lf = _cams(2) if batched else _cams(1)[0]
    if batched:
        vol = vol[None].expand(2, 1, D, H, W)
        tf = tf[None].expand(2, 4, R).contiguous()
    rc1 = Raycaster((D, H, W), (20, 28), R, jitter=False)
    rc2 = Raycaster2D((D, H, W), (20, 28), (R, 1), 1.0, jitter=False)
    a = rc1(vol, tf, lf)
    b = rc2(vol, tf[..., None], lf)
    assert a.shape == b.shape == ((2, 4, 28, 20) if batched else (4, 28, 20))
    assert (a - b).abs().max() <= 1e-5
    an = rc1.raycast_nondiff(vol, tf, lf)
    bn = rc2.raycast_nondiff(vol, tf[..., None], lf)
    assert an.shape == bn.shape and (an - bn).abs().max() <= 1e-5


# --- 6. full size -------------------------------------------------------------------------------------------------------------

def test_full_size(hiplib):
    F, N = _F(), _N()
    n3 = 512
    vol = _volume((n3, n3, n3), seed=12)
    cam = _cams(1, first=0.4)
    tf = _tf1d(64, "opaque", seed=13)
    e, x, r, n = F.ray_setup(cam, (256, 256), vol.shape, 1.0)
    for mode in (N.DR_MODE_DIFF, N.DR_MODE_NONDIFF):
        ref, ref_steps = F.march_fwd(vol, tf, cam, e, x, r, n, 4096, 1.0, mode=mode, variant=N.DR_VARIANT_BASELINE,
                                     workspace=None, hints=0)
        out, steps = F.march_tf2d_fwd(vol, tf[:, None, :].contiguous(), cam, e, x, r, n, 4096, 1.0, 1.0, mode=mode)
        assert torch.equal(steps, ref_steps) and torch.equal(out.view(torch.int32), ref.view(torch.int32))
    # TF-only backward at 512^2 with a table that varies along u
    tf2d = _tf2d(32, 16, "opaque", seed=14)
    g_scale = _g_scale(vol)
    WH = (512, 512)
    e, x, r, n = F.ray_setup(cam, WH, vol.shape, 1.0)
    out, steps = F.march_tf2d_fwd(vol, tf2d, cam, e, x, r, n, 4096, 1.0, g_scale)
    g = torch.randn((1, *WH, 4), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    d_vol, d_tf = F.march_tf2d_bwd(vol, tf2d, cam, e, x, r, n, 4096, 1.0, g_scale, g, out, want_vol=False)
    assert d_vol is None and torch.isfinite(d_tf).all() and d_tf.abs().max() > 0
    # the upstream gradient on one 64 x 64 crop only: d_tf2d against the transliteration of those rays
    crop = np.zeros((1, *WH), bool)
    crop[0, 224:288, 224:288] = True
    C = lambda t: t.detach().double().cpu().numpy()
    host = (C(vol), C(tf2d), g_scale, C(cam), C(e), C(x), C(r), n.cpu().numpy())
    go = np.zeros((1, *WH, 4))
    go[crop] = np.random.RandomState(3).standard_normal((int(crop.sum()), 4))
    ref = R2.run(*host, go, 4096, 1.0, pixels=crop, want_vol=False)
    ref32 = R2.run(*host, go, 4096, 1.0, dtype=torch.float32, pixels=crop, want_vol=False)
    mask = crop & (steps.cpu().numpy() == ref["steps"]) & (ref32["steps"] == ref["steps"]) & (host[-1] > 1)
    assert mask.sum() >= 0.8 * crop.sum()
    gm = go * mask[..., None]
    ref = R2.run(*host, gm, 4096, 1.0, pixels=mask, want_vol=False)
    ref32 = R2.run(*host, gm, 4096, 1.0, dtype=torch.float32, pixels=mask, want_vol=False)
    _, d_tf = F.march_tf2d_bwd(vol, tf2d, cam, e, x, r, n, 4096, 1.0, g_scale, torch.from_numpy(gm).float().to(DEV), out,
                               want_vol=False)
    err = np.abs(C(d_tf) - ref["dtf"]).max()
    err32 = np.abs(ref32["dtf"] - ref["dtf"]).max()
    assert err <= 3.0 * err32 + 1e-5 * np.abs(ref["dtf"]).max(), (err, err32)


# --- 7. the example -----------------------------------------------------------------------------------------------------------

def test_example_fits_a_2d_tf(hiplib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tf2d_opt_synthetic.py"), "--vol", "48", "--img", "48",
                        "--iters", "60", "--views", "2"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    first = float(r.stdout.split("first loss")[1].split()[0])
    last = float(r.stdout.split("last loss")[1].split()[0])
    assert math.isfinite(last) and last <= 0.5 * first, r.stdout
