"""Edges of the RGBA march (csrc/march_rgba.hip) on the GPU: sub-tile and ragged images, a two-voxel axis,
non-dense and misaligned views (the scalar-load path must serve them), rays without samples, max_samples = 1, and non-finite
or out-of-range values."""
import os
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


# --- 7. shapes and views ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("WH", [(5, 3), (9, 17)], ids=["5x3", "9x17"])
def test_sub_tile_and_ragged_images(hiplib, WH):
    from differender_amd.rgba import interleaved
    vol = RG.volume((14, 12, 16), "opaque", seed=21).to(DEV)
    RG.compare(vol, RG.cams(2), WH, 4096, 1.0)
    RG.compare(interleaved(vol), RG.cams(2), WH, 4096, 2.0)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_volume_axis_of_two_voxels(hiplib, axis):
    from differender_amd.rgba import interleaved
    shape = [12, 10, 14]
    shape[axis] = 2
    vol = RG.volume(tuple(shape), "opaque", seed=22).to(DEV)
    RG.compare(vol, RG.cams(1), (12, 12), 4096, 2.0)
    RG.compare(interleaved(vol), RG.cams(1), (12, 12), 4096, 2.0)


def test_a_non_dense_planar_view(hiplib):
    big = torch.full((4, 16, 15, 19), float("nan"), device=DEV)   # (whatever lies around the view is never read)
    vol = big[:, 2:14, 1:13, 3:17]
    vol.copy_(RG.volume((12, 12, 14), "opaque", seed=23))
    assert not vol.is_contiguous()
    st = RG.compare(vol, RG.cams(1), (12, 12), 4096, 1.0)
    assert np.isfinite(C(st["out"])).all()


@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_channel_stride_one_with_a_voxel_stride_of_five(hiplib, vdt):
    """t[..., 1:5] of a 5-channel tensor: the channels are neighbours, the voxels are not 16-byte aligned: four loads per corner."""
    t = torch.full((12, 10, 14, 5), float("nan"), device=DEV, dtype=vdt)
    vol = t[..., 1:5].permute(3, 0, 1, 2)
    vol.copy_(RG.volume((12, 10, 14), "opaque", seed=24))
    assert vol.stride() == (1, 700, 70, 5)
    st = RG.compare(vol, RG.cams(1), (12, 12), 4096, 1.0)
    assert np.isfinite(C(st["out"])).all()


@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_an_interleaved_view_off_its_alignment(hiplib, vdt):
    """Interleaved strides, but the storage offset of one element breaks the 16-byte (8-byte) alignment of every voxel."""
    F = _F()
    from differender_amd.rgba import interleaved
    shape = (12, 10, 14)
    host = RG.volume(shape, "opaque", seed=25).to(vdt)
    buf = torch.full((4 * 12 * 10 * 14 + 4,), float("nan"), device=DEV, dtype=vdt)
    assert buf.data_ptr() % 16 == 0
    vol = buf[1:1 + 4 * 12 * 10 * 14].view(*shape, 4).permute(3, 0, 1, 2)
    vol.copy_(host)
    assert vol.stride(0) == 1 and vol.data_ptr() % (4 * vol.element_size()) != 0
    st = RG.compare(vol, RG.cams(1), (12, 12), 4096, 1.0)
    aligned = interleaved(host.to(DEV))
    out, steps = F.march_rgba_fwd(aligned, st["cam"], *st["rays"], 4096, 1.0)
    assert torch.equal(steps, st["steps"]) and torch.equal(out.view(torch.int32), st["out"].view(torch.int32))


def test_rays_without_samples_give_zero_and_no_gradient(hiplib):
    """A sampling rate so low that many rays plan one sample or none (n <= 1, H6): their pixels are exactly 0, their steps 0, and
    an upstream gradient on them alone reaches no voxel."""
    F = _F()
    from differender_amd import _native as N
    vol = RG.volume((12, 12, 12), "opaque", seed=26).to(DEV)
    cam, WH, sr = RG.cams(2), (12, 10), 0.06
    e, x, r, n = F.ray_setup(cam, WH, vol.shape[-3:], sr)
    dead = n <= 1
    assert dead.any() and (n > 1).any() and (n == 1).any()
    for mode in (N.DR_MODE_DIFF, N.DR_MODE_NONDIFF):
        out, steps = F.march_rgba_fwd(vol, cam, e, x, r, n, 4096, sr, mode=mode)
        assert (out[dead] == 0).all() and (steps[dead] == 0).all()
        assert (steps[~dead] > 0).all() and (out[~dead][:, 3] > 0).all()
    out, steps = F.march_rgba_fwd(vol, cam, e, x, r, n, 4096, sr)
    g = torch.randn((2, *WH, 4), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * dead[..., None]
    d_vol = F.march_rgba_bwd(vol, cam, e, x, r, n, 4096, sr, g, out)
    assert (d_vol == 0).all()
    RG.compare(vol, cam, WH, 4096, sr)   # and the rays that do have samples are the transliteration's


def test_max_samples_one(hiplib):
    from differender_amd.rgba import interleaved
    vol = RG.volume((12, 14, 12), "opaque", seed=27).to(DEV)
    for v in (vol, interleaved(vol)):
        st = RG.compare(v, RG.cams(1), (12, 12), 1, 2.0)
        live = st["host"]["n"] > 1
        assert (C(st["steps"])[live] == 1).all() and (st["host"]["n"][live] > 1).all()


# --- 9. non-finite and out-of-range values ---------------------------------------------------------------------------------

def _finite_close(got, ref, ref32, what):
    """Equal finiteness patterns, and the finite elements by the rule of rgba_gpu.assert_close."""
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), (what, int((np.isfinite(got) != fin).sum()))
    assert (np.isfinite(ref32) == fin).all(), what
    assert fin.any() and (~fin).any(), what
    err = np.abs(got[fin] - ref[fin]).max()
    err32 = np.abs(ref32[fin] - ref[fin]).max()
    scale = np.abs(ref[fin]).max()
    print(f"{what}: err {err / scale:.3e} f32 transliteration {err32 / scale:.3e} (of max |ref| {scale:.3e})")
    assert err <= 3.0 * err32 + 1e-5 * scale, (what, err / scale, err32 / scale)


def test_non_finite_upstream_gradients_propagate_as_in_the_transliteration(hiplib):
    """A NaN pixel, a pixel with +inf in one channel and a pixel of -inf in grad_out: the voxels their rays touch become
    non-finite exactly where the transliteration's do, every other voxel keeps its value; RaycasterRGBA's d_vol is finite."""
    F = _F()
    vol = RG.volume((14, 12, 16), "thin", seed=31).to(DEV)
    cam, WH, S, sr = RG.cams(1), (12, 12), 4096, 1.0
    st = RG.reference(vol, cam, WH, S, sr)
    mask, host = st["mask"], st["host"]
    assert mask[0, 3, 4] and mask[0, 6, 6] and mask[0, 9, 2]
    gm = C(st["gm"])
    gm[0, 3, 4] = np.nan
    gm[0, 6, 6, 0] = np.inf
    gm[0, 9, 2] = -np.inf
    args = (host["vol"], host["cam"], host["entry"], host["exit_"], host["rays"], host["n"], gm, S, sr)
    ref = RR.run(*args, pixels=mask)
    ref32 = RR.run(*args, dtype=torch.float32, pixels=mask)
    d_vol = F.march_rgba_bwd(vol, cam, *st["rays"], S, sr, torch.from_numpy(gm).float().to(DEV), st["out"])
    _finite_close(C(d_vol), ref["dvol"], ref32["dvol"], "dvol")
    # with +inf in the red channel alone, green and blue of that ray's voxels stay finite
    assert np.isfinite(ref["dvol"][1]).sum() > np.isfinite(ref["dvol"][0]).sum()

    from differender_amd.rgba import RaycasterRGBA
    D, H, W = 12, 16, 14
    user = vol.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    rc = RaycasterRGBA((D, H, W), WH, jitter=False, max_samples=S)
    img = rc(user, cam[0])
    w = torch.ones_like(img)
    w[:, 5, 7] = float("nan")
    w[0, 2, 3] = float("inf")
    (img * w).sum().backward()
    assert torch.isfinite(user.grad).all() and user.grad.abs().max() > 0


def _voxel_on_a_sample(cam, e, x, r, n, shape):
    """The voxel (lattice point of the field index space) nearest to a sample of a ray, over the planned samples from the fourth
    on of all rays of view 0: a sample within ~0.1 voxel of it takes more than 0.7 of its value. Not a voxel of the centre cell or of a face."""
    cam, e, x, r, n = cam[0], e[0].reshape(-1), x[0].reshape(-1), r[0].reshape(-1, 3), n[0].reshape(-1)
    best = (np.inf, None)
    scale = np.array(shape, np.float64) - 1.0 - 1e-4
    for s in range(3, int(n.max())):   # (not among a ray's first samples: the backward has samples in front of it)
        ok = (n > s) & (4 * n >= 3 * n.max())   # (a long ray: those samples lie in other cells)
        t0 = e + 0.5 * (x - e) / np.maximum(n, 1)
        f = s / np.maximum(n - 1, 1)
        pos = cam[None] + (t0 * (1 - f) + x * f)[:, None] * r
        q = np.clip(0.5 * pos + 0.5, 0.0, 1.0) * scale
        v = np.rint(q)
        d = np.abs(q - v).max(1)
        inner = ((v >= 1) & (v <= np.array(shape) - 2)).all(1) & (np.abs(v - scale / 2).max(1) > 1.5)
        d = np.where(ok & inner, d, np.inf)
        k = int(np.argmin(d))
        if d[k] < best[0]:
            best = (d[k], tuple(int(c) for c in v[k]))
    assert best[0] < 0.1, best
    return best[1]


@pytest.mark.parametrize("sr", [1.0, 2.0])
def test_an_alpha_voxel_above_one(hiplib, sr):
    """Opacities are not clamped: at rate 1 op = 1 - (1 - a) is above 1 and everything stays finite; at rate 2 a sample with
    a > 1 has a NaN opacity, its pixel is NaN and its ray ends there. The voxel of alpha 1.5 is the one nearest to a sample of
    some ray, so that ray's sample has a > 1. Rays on which the f32 and the f64 transliteration disagree about finiteness are
    left out, with those whose live-sample counts differ."""
    F = _F()
    vol = RG.volume((14, 12, 16), "thin", seed=32)
    cam, WH, S = RG.cams(1), (14, 14), 4096
    e, x, r, n = F.ray_setup(cam, WH, vol.shape[-3:], sr)
    vx, vy, vz = _voxel_on_a_sample(C(cam), C(e), C(x), C(r), n.cpu().numpy(), vol.shape[-3:])
    vol[3, vx, vy, vz] = 1.5
    vol = vol.to(DEV)
    out, steps = F.march_rgba_fwd(vol, cam, e, x, r, n, S, sr)
    host = (C(vol), C(cam), C(e), C(x), C(r), n.cpu().numpy())
    go = torch.randn((1, *WH, 4), generator=torch.Generator().manual_seed(5), dtype=torch.float64).numpy()
    ref = RR.run(*host, go, S, sr, want_grad=False)
    ref32 = RR.run(*host, go, S, sr, dtype=torch.float32, want_grad=False)
    live = host[-1] > 1
    fin = np.isfinite(ref["rgba"]).all(-1)
    mask = (C(steps) == ref["steps"]) & (ref32["steps"] == ref["steps"]) & (np.isfinite(ref32["rgba"]).all(-1) == fin) & live
    assert mask.sum() >= 0.8 * live.sum()
    hit = mask & ((ref["rgba"][..., 3] > 1.0) | ~fin)   # rays that met the voxel
    assert hit.any()
    if sr == 1.0:
        assert fin.all() and (ref["rgba"][..., 3] > 1.0)[mask].any()
    else:
        assert (~fin & mask).any()
    got = C(out)
    assert (np.isfinite(got).all(-1) == fin)[mask].all()
    # NaN pixels are NaN in all four channels or in none
    assert (np.isnan(got).any(-1) == np.isnan(got).all(-1)).all()
    gm = go * mask[..., None]
    ref = RR.run(*host, gm, S, sr, pixels=mask)
    ref32 = RR.run(*host, gm, S, sr, dtype=torch.float32, pixels=mask)
    ok = mask & fin
    scale = np.abs(ref["rgba"][ok]).max()
    err, err32 = np.abs(got[ok] - ref["rgba"][ok]).max(), np.abs(ref32["rgba"][ok] - ref["rgba"][ok]).max()
    print(f"rgba: err {err / scale:.3e} f32 transliteration {err32 / scale:.3e}")
    assert err <= 3.0 * err32 + 1e-5 * scale
    d_vol = F.march_rgba_bwd(vol, cam, e, x, r, n, S, sr, torch.from_numpy(gm).float().to(DEV), out)
    if sr == 1.0:
        assert np.isfinite(ref["dvol"]).all()
        st = dict(ref=ref, ref32=ref32, mask=mask)
        RG.assert_close(C(d_vol), st, "dvol")
    else:
        _finite_close(C(d_vol), ref["dvol"], ref32["dvol"], "dvol")
