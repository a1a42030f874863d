"""Pre-classified RGBA volumes on the GPU (csrc/march_rgba.hip): both layouts (planar and interleaved) against
the float64 transliteration (tests/rgba_reference.py) and bit for bit against each other, the non-differentiable mode around its
alpha threshold, RaycasterRGBA and the example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rgba_gpu as RG  # noqa: E402
import rgba_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = RG.DEV
C = RG.C


def _F():
    from differender_amd import functional as F
    return F


def _interleaved(v):
    from differender_amd.rgba import interleaved
    return interleaved(v)


# --- 6. both layouts against the float64 transliteration -------------------------------------------------------------------

CASES = {
    # name: (volume shape, views (None: one view), per-view volumes, image, alpha kind, sr, max_samples, jitter, vol dtype)
    "ert": ((20, 18, 22), None, False, (16, 16), "opaque", 2.0, 4096, 0, torch.float32),
    "clip": ((24, 24, 24), None, False, (12, 16), "thin", 1.0, 23, 0, torch.float32),
    "jitter": ((18, 22, 16), None, False, (16, 16), "opaque", 1.0, 4096, 4242, torch.float32),
    "nonsquare": ((16, 20, 16), None, False, (20, 12), "thin", 1.0, 4096, 0, torch.float32),
    "sr07": ((16, 16, 16), None, False, (12, 12), "opaque", 0.7, 4096, 0, torch.float32),
    "sr8": ((12, 12, 12), None, False, (8, 8), "thin", 8.0, 4096, 0, torch.float32),
    "f16": ((20, 20, 20), None, False, (16, 16), "opaque", 1.0, 4096, 0, torch.float16),
    "views3": ((16, 18, 20), 3, True, (12, 12), "opaque", 1.0, 4096, 0, torch.float32),
    # one volume seen from three cameras: d_vol sums over the views
    "shared_vol": ((16, 18, 20), 3, False, (12, 12), "opaque", 1.0, 4096, 0, torch.float32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_layouts_against_the_f64_transliteration(hiplib, name):
    vshape, views, per_view, WH, kind, sr, S, jit, vdt = CASES[name]
    planar = RG.volume(vshape, kind, seed=3, views=views if per_view else None).to(DEV).to(vdt)
    inter = _interleaved(planar)
    assert planar.is_contiguous() and inter.stride(-4) == 1 and torch.equal(planar, inter)
    cam = RG.cams(views or 1)
    st = RG.compare(planar, cam, WH, S, sr, jitter=jit)
    ref, mask, host = st["ref"], st["mask"], st["host"]
    if kind == "opaque":
        assert (ref["steps"] < np.minimum(host["n"], S))[mask].any()   # some compared ray stops early
    if name == "clip":
        assert (host["n"] > S).any()
    if name == "shared_vol":
        assert ref["dvol"].shape == (4, *vshape)
    # the interleaved layout on the same rays: the same bits, and its own d_vol (another order of the atomics) to the reference
    F = _F()
    out_i, steps_i = F.march_rgba_fwd(inter, cam, *st["rays"], S, sr)
    assert torch.equal(steps_i, st["steps"])
    assert torch.equal(out_i.view(torch.int32), st["out"].view(torch.int32))
    d_i = RG.backward(inter, st)
    assert d_i.stride() == inter.stride() and d_i.dtype == torch.float32
    RG.assert_close(C(d_i), st, "dvol")


# --- 8. the non-differentiable mode --------------------------------------------------------------------------------------

def _threshold_volume(shape, seed):
    """Thin-to-medium live alpha with exact zeros (an octant and scattered voxels) and small constant blocks just below, at and
    just above the non-differentiable march's threshold 1e-3, beside live voxels."""
    vol = RG.volume(shape, "thin", seed=seed)
    rng = np.random.RandomState(seed + 1)
    b = (vol[3] - 0.01) / 0.05
    vol[3] = 0.02 + 0.4 * b ** 2
    VX, VY, VZ = shape
    vol[3, : VX // 2, : VY // 2, : VZ // 2] = 0.0
    vol[3][torch.from_numpy(rng.uniform(size=shape) < 0.05)] = 0.0
    for k, level in enumerate((9.9999e-4, 1e-3, 1.0001e-3)):
        x0 = VX // 2 + 1 + 3 * k
        vol[3, x0:x0 + 3, VY // 2 + 2:VY // 2 + 6, 2 + 4 * k:6 + 4 * k] = level
    return vol


@pytest.mark.parametrize("sr", [4.0, 8.0])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_nondiff_against_the_f64_transliteration(hiplib, sr, layout):
    """Rays with a sample within 1e-5 of alpha 1e-3 in f64 or f32 are left out (the two may take the threshold apart), as are
    rays whose live-sample counts differ."""
    F = _F()
    from differender_amd import _native as N
    vol = _threshold_volume((20, 18, 22), seed=15).to(DEV)
    if layout == "interleaved":
        vol = _interleaved(vol)
    cam, WH, S = RG.cams(2), (16, 14), 8
    e, x, r, n = F.ray_setup(cam, WH, vol.shape[-3:], sr)
    out, steps = F.march_rgba_fwd(vol, cam, e, x, r, n, S, sr, mode=N.DR_MODE_NONDIFF)   # (no clip)
    host = (C(vol), C(cam), C(e), C(x), C(r), n.cpu().numpy())
    go = np.zeros((2, *WH, 4))
    ref = RR.run(*host, go, S, sr, want_grad=False, nondiff=True)
    ref32 = RR.run(*host, go, S, sr, dtype=torch.float32, want_grad=False, nondiff=True)
    live = host[-1] > 1
    assert (ref["near"] & live).any()   # the blocks around the threshold are seen
    mask = (C(steps) == ref["steps"]) & (ref32["steps"] == ref["steps"]) & ~ref["near"] & ~ref32["near"] & live
    assert mask.sum() >= 0.8 * live.sum(), (mask.sum(), live.sum())
    assert (ref["steps"] > S)[mask].any()   # the non-differentiable march has no max_samples clip
    want = ref["rgba"][mask]
    assert (want[:, 3] > 0).any() and (want[:, 3] < 0.99).any()
    err = np.abs(C(out)[mask] - want).max()
    err32 = np.abs(ref32["rgba"][mask] - want).max()
    print(f"nondiff rgba: err {err:.3e} f32 transliteration {err32:.3e} (max |ref| {np.abs(want).max():.3e})")
    assert err <= 3.0 * err32 + 1e-5 * np.abs(want).max(), (err, err32)
    assert (C(out) <= 1.0).all()
    assert (C(out)[~live] == 0).all() and (C(steps)[~live] == 0).all()


# --- 10. RaycasterRGBA -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("batched", [False, True])
def test_raycaster_rgba_matches_the_functional_calls(hiplib, batched, vdt):
    from differender_amd.rgba import RaycasterRGBA, interleaved
    F = _F()
    D, H, W = 18, 20, 22
    BS = 2
    field = RG.volume((W, D, H), "opaque", seed=8, views=BS if batched else None).to(DEV).to(vdt)   # ([BS,] 4, W, D, H)
    user = field.permute(0, 1, 3, 4, 2) if batched else field.permute(0, 2, 3, 1)               # ([BS,] 4, D, H, W)
    vol_user = interleaved(user.contiguous()).detach().requires_grad_(True)
    lf = RG.cams(BS) if batched else RG.cams(1)[0]
    rc = RaycasterRGBA((D, H, W), (24, 16), sampling_rate=2.0, jitter=True)
    k = 2468
    torch.manual_seed(k)
    seed = F.new_jitter_seed()
    assert seed != 0
    torch.manual_seed(k)
    img = rc(vol_user, lf)
    assert img.shape == ((BS, 4, 16, 24) if batched else (4, 16, 24)) and img.dtype == torch.float32
    G = torch.randn(img.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    (img * G).sum().backward()
    assert vol_user.grad.dtype == vdt and vol_user.grad.stride() == vol_user.stride() and vol_user.grad.shape == vol_user.shape
    # the functional calls on the field view, with the replayed seed
    vol_f = vol_user.detach().permute(0, 1, 4, 2, 3) if batched else vol_user.detach().permute(0, 3, 1, 2)
    cam = lf.reshape(-1, 3)
    e, x, r, n = F.ray_setup(cam, (24, 16), vol_f.shape[-3:], 2.0, jitter_seed=seed)
    out, steps = F.march_rgba_fwd(vol_f, cam, e, x, r, n, 512, 2.0)
    res = out if batched else out[0]
    assert torch.equal(rc._image(res, batched), img.detach())
    assert torch.equal(rc._steps, steps if batched else steps[0])
    o = res.clone().requires_grad_(True)
    rc._image(o, batched).backward(G)
    dv = F.march_rgba_bwd(vol_f, cam, e, x, r, n, 512, 2.0, o.grad if batched else o.grad[None], out)
    dv_user = dv.permute(0, 1, 3, 4, 2) if batched else dv.permute(0, 2, 3, 1)
    # (another order of the float atomics, 1e-5 as in tests/test_gpu_tf2d.py; then one rounding to the volume's dtype: 2^-11)
    # (the functional d_vol itself, float32 for either storage, is held to the reference's 1e-5 rule in
    # test_both_layouts_against_the_f64_transliteration, case "f16" included; 2^-11 is only autograd's cast of .grad to float16)
    tol = 1e-5 if vdt == torch.float32 else 1e-5 + 2.0 ** -11
    assert (vol_user.grad.float() - dv_user).abs().max() <= tol * dv_user.abs().max()
    nd = rc.raycast_nondiff(vol_user.detach(), lf)
    assert nd.shape == img.shape and torch.isfinite(nd).all() and float(nd.max()) <= 1.0
    with pytest.raises(ValueError, match="look_from"):
        rc(vol_user, lf.clone().requires_grad_(True))


# --- 11. the example ---------------------------------------------------------------------------------------------------------

def test_example_recovers_an_rgba_volume(hiplib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rgba_recon_synthetic.py"), "--vol", "24", "--img", "32",
                        "--views", "4", "--steps", "30"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    first = float(r.stdout.split("first loss")[1].split()[0])
    last = float(r.stdout.split("last loss")[1].split()[0])
    assert math.isfinite(last) and last < first, r.stdout
