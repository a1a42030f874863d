"""X-ray line-integral and maximum intensity projections on the GPU: both forwards against the float64
transliteration (tests/proj_reference.py) on the kernels' own ray buffers, the chord length, MIP ties, negative and missed rays;
the adjoint identity of both SUM backwards, windowed against plain, d_vol and d look_from against autograd of the
transliteration (D8's rule), Projector against the functional calls, a 512^3 run and the CT example."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import proj_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _dev():
    return torch.device("cuda")


def _cam(theta, phi, r):
    return [r * math.cos(phi) * math.sin(theta), r * math.sin(phi), r * math.cos(phi) * math.cos(theta)]


def _rays(cams, WH, vshape, sr, seed=0, fov=30.0, view_base=0):
    from differender_amd import functional as F
    cam = torch.tensor(cams, dtype=torch.float32, device=_dev()).reshape(-1, 3)
    return (cam,) + F.ray_setup(cam, WH, vshape, sr, fov, 0.1, seed, view_base)


def _volume(vshape, seed, views=None, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    shape = tuple(vshape) if views is None else (views,) + tuple(vshape)
    return (lo + torch.rand(shape, generator=g)).to(_dev())


def _ref_fwd(vol, cam, e, x, r, n, S, mode, view):
    v = vol[view] if vol.ndim == 4 else vol
    c = lambda t: t[view].reshape(-1, *t.shape[3:]).double().cpu()
    out, arg = PR.project(v.double().cpu(), cam[view].double().cpu(), c(e), c(x), c(r), c(n).long(), S, mode)
    return out, arg


FWD_CASES = {
    # name: volume, image, sampling rate, jitter seed, cameras, max_samples, per-view volumes, dtype
    "orbit_sr1": ((24, 20, 28), (16, 12), 1.0, 0, [_cam(0.6, 0.3, 2.7)], None, False, torch.float32),
    "jitter_sr0.7": ((20, 24, 18), (12, 16), 0.7, 4242, [_cam(2.0, -0.2, 3.0)], None, False, torch.float32),
    "f16_sr4": ((16, 18, 20), (10, 9), 4.0, 0, [_cam(-1.1, 0.6, 2.4)], None, False, torch.float16),
    "f16_jitter_sr2.5": ((18, 16, 16), (9, 11), 2.5, 99, [_cam(0.2, 0.1, 3.3)], None, False, torch.float16),
    "views_shared": ((16, 16, 16), (8, 8), 1.5, 7, [_cam(k, 0.2 * k - 0.4, 2.8) for k in range(4)], None, False, torch.float32),
    "views_own": ((16, 14, 12), (8, 10), 1.0, 0, [_cam(k + 0.3, 0.1, 3.0) for k in range(3)], None, True, torch.float32),
    "inside": ((20, 20, 20), (16, 16), 1.0, 0, [[0.3, -0.2, 0.4]], None, False, torch.float32),
    "clipped": ((24, 24, 24), (12, 12), 2.0, 0, [_cam(0.4, 0.4, 2.6)], 17, False, torch.float32),
    "aniso": ((40, 12, 24), (14, 10), 1.0, 5, [_cam(0.9, -0.3, 2.9)], None, False, torch.float32),
}


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("case", sorted(FWD_CASES))
def test_forward_matches_the_transliteration(case, mode):
    from differender_amd import functional as F
    vshape, WH, sr, seed, cams, S, own, dt = FWD_CASES[case]
    V = len(cams)
    vol = _volume(vshape, 11, V if own else None, lo=-0.3 if mode == "max" else 0.0).to(dt)
    cam, e, x, r, n = _rays(cams, WH, vshape, sr, seed)
    out, arg = F.project_fwd(vol, cam, e, x, r, n, S, mode)
    torch.cuda.synchronize()
    for v in range(V):
        ref, _ = _ref_fwd(vol, cam, e, x, r, n, S, mode, v)
        got = out[v].reshape(-1).double().cpu()
        scale = float(ref.abs().max()) + 1e-30
        # SUM: the f32 sum's roundings; MAX: one sample, whose f32 position (t, pos: ~2e-7 world units) moves its value on a
        # random volume (slopes ~ (V - 1) / 2 per world unit) by a few 1e-6
        assert float((got - ref).abs().max()) <= (2e-6 if mode == "sum" else 1e-5) * scale, (case, v)
        if mode == "max":   # the stored sample holds the maximum (its index may differ from f64's only on near-ties)
            a = arg[v].reshape(-1).cpu()
            nn = n[v].reshape(-1).cpu()
            assert ((a >= 0) == (nn > 1)).all()
    if S is not None:
        assert (n > S).any()


def test_constant_volume_gives_the_chord_length():
    from differender_amd import functional as F
    c = 0.625
    for seed, cams in ((0, [_cam(0.5, 0.2, 2.8), [0.2, 0.1, -0.3]]), (31, [_cam(2.5, -0.5, 4.0)])):
        for dt in (torch.float32, torch.float16):
            vol = torch.full((20, 18, 22), c, device=_dev(), dtype=dt)
            cam, e, x, r, n = _rays(cams, (17, 13), (20, 18, 22), 1.0, seed)
            out, _ = F.project_fwd(vol, cam, e, x, r, n, None, "sum")
            ok = n >= 2
            assert ok.any()
            chord = c * (x - e)
            torch.testing.assert_close(out[ok], chord[ok], rtol=2e-6, atol=1e-6)
            assert (out[~ok] == 0).all()


def test_mip_ties_negative_and_missed_rays():
    from differender_amd import functional as F
    vs = (16, 16, 16)
    cam, e, x, r, n = _rays([_cam(0.3, 0.2, 5.0)], (32, 32), vs, 1.0)   # the image corners miss the box
    assert (n == 0).any() and (n > 1).any()
    out, arg = F.project_fwd(torch.full(vs, -0.5, device=_dev()), cam, e, x, r, n, None, "max")
    live = n > 1
    assert (arg[live] == 0).all() and (out[live] == -0.5).all()   # all equal: the first sample wins
    assert (arg[n == 0] == -1).all() and (out[n == 0] == 0).all()
    vol = -1.0 - _volume(vs, 4)
    out, arg = F.project_fwd(vol, cam, e, x, r, n, None, "max")
    ref, _ = _ref_fwd(vol, cam, e, x, r, n, None, "max", 0)
    assert (out[live] < -1.0).all()
    assert float((out[0].reshape(-1).double().cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def _dvol(vol, cam, e, x, r, n, g, S, mode, arg, variant):
    from differender_amd import functional as F
    return F.project_bwd(vol, cam, e, x, r, n, g, S, mode, arg, variant=variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_sum_adjoint_identity(variant):
    from differender_amd import functional as F
    for vshape, WH, sr, seed, cams, own in (((32, 28, 36), (24, 20), 1.3, 0, [_cam(0.4, 0.3, 2.7)], False),
                                            ((24, 24, 24), (16, 16), 2.0, 17, [_cam(k, 0.5 - 0.3 * k, 3.0) for k in range(3)], True)):
        vol = _volume(vshape, 2, len(cams) if own else None)
        cam, e, x, r, n = _rays(cams, WH, vshape, sr, seed)
        out, _ = F.project_fwd(vol, cam, e, x, r, n, None, "sum")
        g = torch.randn(out.shape, device=_dev())
        d = _dvol(vol, cam, e, x, r, n, g, None, "sum", None, variant)
        lhs = float((out.double() * g.double()).sum())
        rhs = float((vol.double() * d.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((out.double().abs() * g.double().abs()).sum()), (lhs, rhs)


WINDOW_CASES = {
    # name: volume (field order, contiguous or the user's (1, D, H, W) permuted), image, rate, cameras, fov
    "axis_aligned": ((48, 48, 48), (40, 36), 1.0, [[0.0, 0.0, 2.8]], 30.0, False),
    "oblique_45": ((40, 44, 36), (37, 29), 1.5, [_cam(math.pi / 4, math.atan(1 / math.sqrt(2)), 2.6)], 30.0, True),
    "shared_8_views": ((32, 32, 32), (24, 24), 1.0, [_cam(0.8 * k, 0.3 * math.sin(k), 2.7) for k in range(8)], 30.0, True),
    "near_wide_fallback": ((64, 64, 64), (9, 7), 1.0, [[0.1, 0.2, 0.6]], 60.0, False),
}


@pytest.mark.parametrize("case", sorted(WINDOW_CASES))
def test_windowed_backward_matches_the_plain_one(case):
    from differender_amd import functional as F
    vshape, WH, sr, cams, fov, user_layout = WINDOW_CASES[case]
    if user_layout:   # the layout Projector hands over: x contiguous
        vol = _volume((vshape[1], vshape[2], vshape[0]), 6).permute(2, 0, 1)
    else:
        vol = _volume(vshape, 6)
    cam = torch.tensor(cams, dtype=torch.float32, device=_dev())
    e, x, r, n = F.ray_setup(cam, WH, vshape, sr, fov, 0.1, 123)
    g = torch.randn((len(cams),) + WH, device=_dev())
    dw = _dvol(vol, cam, e, x, r, n, g, None, "sum", None, 0)
    dp = _dvol(vol, cam, e, x, r, n, g, None, "sum", None, 1)
    assert dw.stride() == vol.stride()
    scale = float(dp.abs().max())
    assert scale > 0
    assert float((dw - dp).abs().max()) <= 1e-5 * scale, case
    assert int(((dw != 0) != (dp != 0)).sum()) <= int((dp.abs() < 1e-6 * scale).sum())


def _d8_check(got, ref64, ref32, what):
    err32 = float((ref32 - ref64).abs().max())
    scale = float(ref64.abs().max())
    tol = max(3.0 * err32, 1e-5 * max(scale, 1.0))
    assert float((got - ref64).abs().max()) <= tol, (what, float((got - ref64).abs().max()), tol, err32)


GRAD_CASES = {
    "orbit": ((14, 12, 16), (10, 8), 1.0, 0, _cam(0.5, 0.3, 2.7)),
    "jitter_sr2": ((12, 14, 12), (8, 9), 2.0, 555, _cam(2.4, -0.3, 3.1)),
    "inside": ((12, 12, 12), (8, 8), 1.0, 0, [0.2, -0.1, 0.5]),
}


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("case", sorted(GRAD_CASES))
def test_gradients_match_autograd_of_the_transliteration(case, mode):
    from differender_amd import functional as F
    vshape, (W, H), sr, seed, cp = GRAD_CASES[case]
    VIEW = 3
    vol = _volume(vshape, 8)
    cam = torch.tensor([cp], dtype=torch.float32, device=_dev())
    e, x, r, n = F.ray_setup(cam, (W, H), vshape, sr, 30.0, 0.1, seed, VIEW)
    out, arg = F.project_fwd(vol, cam, e, x, r, n, None, mode)
    g = torch.randn((1, W, H), device=_dev())
    dvol = F.project_bwd(vol, cam, e, x, r, n, g, None, mode, arg, variant=0)
    dcam, dray = F.project_bwd_cam(vol, cam, e, x, r, n, g, None, mode, arg, jitter_seed=seed, view_base=VIEW, per_ray=True)
    gc = g[0].reshape(-1).double().cpu()

    refs = {}
    for dt in (F64, torch.float32):
        v = vol.cpu().to(dt).requires_grad_(True)
        cpp = torch.tensor(cp, dtype=dt).expand(W * H, 3).clone().requires_grad_(True)
        o, a, (e2, x2, r2, n2) = PR.project_camera(v, cpp, W, H, sr, None, mode, jitter_seed=seed, view=VIEW)
        (o * gc.to(dt)).sum().backward()
        refs[dt] = (v.grad.double(), cpp.grad.double(), n2, a)
    # d_vol on the kernels' own buffers (the f64 ray setup can pick another n for a ray). MIP: at the kernel's own argmax -- an f32
    # near-tie can move it off the transliteration's, which would move that ray's taps -- so that every case is compared
    dv_refs = {}
    a_own = arg[0].reshape(-1).cpu().long() if mode == "max" else None
    for dt in (F64, torch.float32):
        v = vol.cpu().to(dt).requires_grad_(True)
        c = lambda t: t[0].reshape(-1, *t.shape[3:]).cpu().to(dt)
        bufs = (cam[0].cpu().to(dt), c(e), c(x), c(r), n[0].reshape(-1).cpu().long())
        if mode == "sum":
            o, _ = PR.project(v, *bufs, None, mode)
        else:
            assert (PR.project(v.detach(), *bufs, None, mode)[1] == a_own).float().mean() > 0.99
            o = PR.sample_at(v, *bufs, a_own)
        (o * gc.to(dt)).sum().backward()
        dv_refs[dt] = v.grad.double()
    assert bool((dv_refs[F64] != 0).any())
    _d8_check(dvol.double().cpu(), dv_refs[F64], dv_refs[torch.float32], "d_vol")
    # d look_from per ray, on the rays whose n (and, for MIP, argmax) the f64 ray setup reproduces
    _, c64, n64, a64 = refs[F64]
    _, c32, n32, a32 = refs[torch.float32]
    same = (n64 == n[0].reshape(-1).cpu().long()) & (n32 == n64)
    if mode == "max":
        same &= (a64 == arg[0].reshape(-1).cpu().long()) & (a32 == a64)
    assert same.float().mean() > 0.9
    got = dray[0].reshape(-1, 3).double().cpu()
    _d8_check(got[same], c64[same], c32[same], "d look_from")
    assert torch.isfinite(dcam).all()


def test_projector_matches_the_functional_calls():
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    D, Hh, Ww = 20, 18, 22
    for mode in ("sum", "max"):
        pj = Projector((D, Hh, Ww), (16, 12), mode=mode, sampling_rate=1.5, jitter=False, max_samples=40)
        vol = _volume((3, 1, D, Hh, Ww), 9).reshape(3, 1, D, Hh, Ww).requires_grad_(True)
        lf = torch.tensor([_cam(0.3 * k, 0.2, 2.8) for k in range(3)], device=_dev(), requires_grad=True)
        img = pj(vol, lf)
        assert img.shape == (3, 1, 12, 16)
        g = torch.randn_like(img)
        (img * g).sum().backward()
        vf = vol.detach().squeeze(1).permute(0, 3, 1, 2)
        e, x, r, n = F.ray_setup(lf.detach(), (16, 12), vf.shape[-3:], 1.5, 30.0, 0.1, 0)
        out, arg = F.project_fwd(vf, lf.detach(), e, x, r, n, 40, mode)
        torch.testing.assert_close(img.detach(), torch.flip(out, (2,)).permute(0, 2, 1)[:, None], rtol=0, atol=0)
        gk = torch.flip(g[:, 0].permute(0, 2, 1), (2,))
        dv = F.project_bwd(vf, lf.detach(), e, x, r, n, gk, 40, mode, arg)
        torch.testing.assert_close(vol.grad.squeeze(1).permute(0, 3, 1, 2), dv, rtol=1e-5, atol=1e-6)
        dc = F.project_bwd_cam(vf, lf.detach(), e, x, r, n, gk, 40, mode, arg)
        torch.testing.assert_close(lf.grad, dc, rtol=1e-5, atol=1e-6)
        # a shared volume and camera, f16 under autocast: the image is float32, gradients in the inputs' dtypes
        v1 = vol.detach()[0].half().requires_grad_(True)
        l1 = lf.detach()[0].clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            im1 = pj(v1, l1)
        assert im1.shape == (1, 12, 16) and im1.dtype == torch.float32
        im1.sum().backward()
        assert v1.grad.dtype == torch.float16 and l1.grad.shape == (3,)
        with torch.no_grad():
            assert torch.isfinite(pj(vol, lf)).all()


def test_projector_shares_an_unbatched_volume_among_batched_cameras():
    """A shared (1, D, H, W) volume with look_from (2, 3), mode "max", on a 9 x 10 x 11 volume and an 11 x 13 image (no multiple
    of the 8 x 8 tile): the image is bit for bit the functional calls' on the explicitly permuted view, the shared volume
    receives one gradient summed over both views. (The gradients are sums of atomics whose order varies from run to run:
    compared at the bar of test_projector_matches_the_functional_calls, not bit for bit.)"""
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    D, Hh, Ww, WH = 9, 10, 11, (11, 13)
    pj = Projector((D, Hh, Ww), WH, mode="max", jitter=False)
    vol = _volume((1, D, Hh, Ww), 21).requires_grad_(True)
    lf = torch.tensor([_cam(0.3, 0.2, 2.8), _cam(1.9, -0.3, 2.6)], device=_dev(), requires_grad=True)
    img = pj(vol, lf)
    assert img.shape == (2, 1, 13, 11)
    vf = vol.detach().squeeze(0).permute(2, 0, 1)
    e, x, r, n = F.ray_setup(lf.detach(), WH, vf.shape, 1.0, 30.0, 0.1, 0)
    out, arg = F.project_fwd(vf, lf.detach(), e, x, r, n, None, "max")
    assert torch.equal(img.detach(), torch.flip(out, (2,)).permute(0, 2, 1)[:, None])
    g = torch.randn_like(img)
    (img * g).sum().backward()
    gk = torch.flip(g[:, 0].permute(0, 2, 1), (2,))
    dv = F.project_bwd(vf, lf.detach(), e, x, r, n, gk, None, "max", arg)
    assert vol.grad.shape == vol.shape and dv.shape == vf.shape
    torch.testing.assert_close(vol.grad.squeeze(0).permute(2, 0, 1), dv, rtol=1e-5, atol=1e-6)
    dc = F.project_bwd_cam(vf, lf.detach(), e, x, r, n, gk, None, "max", arg)
    assert lf.grad.shape == (2, 3)
    torch.testing.assert_close(lf.grad, dc, rtol=1e-5, atol=1e-6)


def test_full_size_512():
    from differender_amd import functional as F
    N, WH = 512, (512, 512)
    vol = torch.rand((N, N, N), device=_dev())
    cam, e, x, r, n = _rays([_cam(0.7, 0.35, 2.7)], WH, (N, N, N), 1.0, 77)
    out, _ = F.project_fwd(vol, cam, e, x, r, n, None, "sum")
    g = torch.randn_like(out)
    lhs = float((out.double() * g.double()).sum())
    for variant in (0, 1):
        d = F.project_bwd(vol, cam, e, x, r, n, g, None, "sum", None, variant=variant)
        assert bool(torch.isfinite(d).all())
        rhs = float((vol.double() * d.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((out.double().abs() * g.double().abs()).sum()), (variant, lhs, rhs)
        del d
    out, arg = F.project_fwd(vol, cam, e, x, r, n, None, "max")
    assert bool(torch.isfinite(out).all()) and bool((arg[n > 1] >= 0).all())


def test_ct_example_lowers_the_volume_error():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ct_recon_synthetic.py"), "--vol", "32", "--img", "48",
                          "--views", "12", "--batch", "4", "--iterations", "40"], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    m = re.search(r"start ([0-9.e+-]+)\s+end ([0-9.e+-]+)", res.stdout)
    assert m, res.stdout
    assert float(m.group(2)) < 0.5 * float(m.group(1)), res.stdout
