"""The projection backward kernels held to the float64 transliteration where tests/test_gpu_projection.py
leaves them to each other: both SUM backwards against float64 autograd at window sizes, on every path of the windowed kernel
(LDS at the first depth, LDS after halving, the global fallback: tests/proj_reference.window_plan says which a case takes, and
tests/test_projection.py holds the case table to it), under max_samples clipping, on f16 and per-view volumes, in four memory
layouts; the camera kernel under clipping, f16, another field of view, several jittered views and its per-view total; the MIP's
arg_max and its d_vol at the kernel's own arg_max; stale arg_max entries; NaN and infinite upstream gradients; Projector with
jitter and with an f16 volume outside autocast.

Every expected value is the float64 transliteration on the kernels' own ray buffers (camera gradients: from the camera, which
recomputes the rays), every tolerance the project's own (_d8_check, 2e-6 / 1e-5 of the scale for the SUM / MAX forward, 1e-5
for windowed against plain) but the one derived at _check_total.

Not targeted: the windowed kernel's out-of-box tap, the global atomic taken when a last-place rounding of mix() moves a cell
outside the box of the first and last sample's cells. No input is known to reach it on purpose."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proj_reference as PR  # noqa: E402
import test_gpu_projection as B  # noqa: E402  (_d8_check, the device)

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def _setup(case, vol_seed, lo=0.0):
    """The case on the device: vol (its dtype and layout), its values (CPU float32), cam (V, 3) and the ray buffers."""
    from differender_amd import functional as F
    V = len(case["cams"])
    vals = PR.case_values(case, vol_seed, V if case.get("own") else None, lo)
    vol = PR.layout_volume(vals.to(B._dev()).to(case["dtype"]), case.get("layout", "z"))
    cam = torch.tensor(case["cams"], dtype=F32, device=B._dev()).reshape(-1, 3)
    e, x, r, n = F.ray_setup(cam, case["WH"], case["vshape"], case["sr"], case["fov"], 0.1, case["seed"], case.get("view_base", 0))
    return vol, vals, cam, e, x, r, n


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(B._dev())


def _bufs(cam, e, x, r, n, v, dt):
    """View v's camera and ray buffers on the CPU in dt (a missed ray's entry and exit, never used, as zeros)."""
    nn = n[v].reshape(-1).cpu().long()
    c = lambda t: t[v].reshape(-1, *t.shape[3:]).cpu().to(dt)
    zero = torch.zeros((), dtype=dt)
    return cam[v].cpu().to(dt), torch.where(nn > 0, c(e), zero), torch.where(nn > 0, c(x), zero), c(r), nn


def _ref_dvol(vals, own, cam, e, x, r, n, g, dt, fn):
    """d sum_v <fn(volume of view v, view v's buffers, v), g[v]> / d vals by autograd in dt. fn returns (W * H,)."""
    vv = vals.detach().to(dt).clone().requires_grad_(True)
    total = torch.zeros((), dtype=dt)
    for v in range(n.shape[0]):
        out = fn(vv[v] if own else vv, *_bufs(cam, e, x, r, n, v, dt), v)
        total = total + (out * g[v].reshape(-1).cpu().to(dt)).sum()
    total.backward()
    return vv.grad.double()


def _sum_fn(S):
    return lambda vol, c, e, x, r, n, v: PR.project(vol, c, e, x, r, n, S, "sum")[0]


def _at_fn(arg):
    a = arg.reshape(arg.shape[0], -1).cpu().long()
    return lambda vol, c, e, x, r, n, v: PR.sample_at(vol, c, e, x, r, n, a[v])


def _check_dvol(got, vals, own, bufs, g, fn, what):
    refs = {dt: _ref_dvol(vals, own, *bufs, g, dt, fn) for dt in (F64, F32)}
    assert got.dtype == F32 and got.shape == vals.shape
    assert float(refs[F64].abs().max()) > 0, what
    B._d8_check(got.double().cpu(), refs[F64], refs[F32], what)


def _check_total(dcam, dray, what):
    """d_cam[v] is the sum of d_cam_ray[v]: the kernel adds the same float32 per-ray values in float64 and the wrapper rounds the
    total to float32 once, 2^-24 relative to at most sum |d_cam_ray|; 1e-6 of that leaves 16x and takes the float64 order in."""
    rows = dray.double().cpu().reshape(dray.shape[0], -1, 3)
    assert bool(torch.isfinite(dcam).all()), what
    err = (dcam.double().cpu() - rows.sum(1)).abs()
    assert bool((err <= 1e-6 * rows.abs().sum(1)).all()), (what, err.tolist(), rows.abs().sum(1).tolist())


def _plan(case, cam, e, x, r, n):
    W, H = case["WH"]
    total = np.zeros(5, dtype=np.int64)
    for v in range(n.shape[0]):
        total += np.array(PR.window_plan(cam[v].cpu().numpy(), e[v].cpu().numpy(), x[v].cpu().numpy(), r[v].cpu().numpy(),
                                         n[v].cpu().numpy(), case["vshape"], case["S"], W, H))
    return PR.WindowPlan(*(int(t) for t in total))


# ---- B: both SUM backwards against float64 autograd at window sizes -----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PR.EDGE_CASES))
def test_sum_backwards_match_float64_autograd(name):
    from differender_amd import functional as F
    case = PR.EDGE_CASES[name]
    S, own = case["S"], case["own"]
    vol, vals, cam, e, x, r, n = _setup(case, 6)
    g = _randn(tuple(n.shape), 40)
    dw = F.project_bwd(vol, cam, e, x, r, n, g, S, "sum", None, variant=0)
    dp = F.project_bwd(vol, cam, e, x, r, n, g, S, "sum", None, variant=1)
    torch.cuda.synchronize()
    # the case is what the table says: its window paths on these very buffers, its clipping, its strides
    plan = _plan(case, cam, e, x, r, n)
    print(f"PROJ_WINDOW_PATHS {name}: lds_full {plan.lds_full} lds_halved {plan.lds_halved} fallback {plan.fallback} "
          f"dead_tiles {plan.dead_tiles} live_tiles {plan.live_tiles}")
    windows = plan.lds_full + plan.lds_halved + plan.fallback
    for path in case["paths"]:
        assert getattr(plan, path) >= max(3, 0.05 * windows), (name, path, plan)
    if case.get("dead_tiles"):
        assert plan.dead_tiles >= 1 and plan.live_tiles >= 1
    if S is not None:
        assert float((n[n > 1] > S).float().mean()) > 1 / 3
    if own:
        assert vol.stride(0) != 0 and dw.stride(0) != 0
    if case["layout"] == "strided":
        assert 1 not in vol.stride() and dw.stride() != vol.stride() and dw.stride(-3) == 1
    else:
        assert dw.stride() == vol.stride() and dp.stride() == vol.stride()
    refs = {dt: _ref_dvol(vals, own, cam, e, x, r, n, g, dt, _sum_fn(S)) for dt in (F64, F32)}
    for variant, d in (("windowed", dw), ("plain", dp)):
        assert d.dtype == F32 and d.shape == vol.shape
        B._d8_check(d.double().cpu(), refs[F64], refs[F32], (name, variant))
    scale = float(dp.abs().max())
    assert scale > 0
    assert float((dw - dp).abs().max()) <= 1e-5 * scale, name
    assert int(((dw != 0) != (dp != 0)).sum()) <= int((dp.abs() < 1e-6 * scale).sum())


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("name", sorted(k for k, c in PR.EDGE_CASES.items() if c["layout"] in ("y", "strided")))
def test_forward_on_y_contiguous_and_strided_volumes(name, mode):
    from differender_amd import functional as F
    case = PR.EDGE_CASES[name]
    vol, vals, cam, e, x, r, n = _setup(case, 6, lo=-0.3 if mode == "max" else 0.0)
    assert vol.stride(-1) != 1 and vol.stride(-3) != 1   # neither of tri_sample's pair-load paths
    out, arg = F.project_fwd(vol, cam, e, x, r, n, case["S"], mode)
    torch.cuda.synchronize()
    for v in range(n.shape[0]):
        ref, _ = PR.project((vals[v] if case["own"] else vals).double(), *_bufs(cam, e, x, r, n, v, F64), case["S"], mode)
        got = out[v].reshape(-1).double().cpu()
        scale = float(ref.abs().max())
        assert scale > 0
        assert float((got - ref).abs().max()) <= (2e-6 if mode == "sum" else 1e-5) * scale, (name, v)


# ---- C: the camera backward per ray and in total ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("name", sorted(PR.CAM_CASES))
def test_camera_gradient_per_ray_and_total(name, mode):
    from differender_amd import functional as F
    case = PR.CAM_CASES[name]
    (W, H), S, vb = case["WH"], case["S"], case["view_base"]
    vol, vals, cam, e, x, r, n = _setup(case, 8, lo=-0.3 if mode == "max" else 0.0)
    V = n.shape[0]
    out, arg = F.project_fwd(vol, cam, e, x, r, n, S, mode)
    g = _randn((V, W, H), 41)
    dcam, dray = F.project_bwd_cam(vol, cam, e, x, r, n, g, S, mode, arg, fov_deg=case["fov"], jitter_seed=case["seed"],
                                   view_base=vb, per_ray=True)
    torch.cuda.synchronize()
    assert dcam.shape == (V, 3) and dray.shape == (V, W, H, 3)
    if S is not None:
        assert float((n[n > 1] > S).float().mean()) > 1 / 3
    if name == "odd_missed":
        assert W % 8 and H % 8 and bool((n == 0).any()) and bool((n > 1).any())
    _check_total(dcam, dray, (name, mode))
    for v in range(V):
        gc = g[v].reshape(-1).double().cpu()
        refs = {}
        for dt in (F64, F32):
            cpp = cam[v].cpu().to(dt).expand(W * H, 3).clone().requires_grad_(True)
            o, a, (_, _, _, n2) = PR.project_camera(vals.to(dt), cpp, W, H, case["sr"], S, mode, fov_deg=case["fov"],
                                                    jitter_seed=case["seed"], view=vb + v)
            (o * gc.to(dt)).sum().backward()
            refs[dt] = (cpp.grad.double(), n2, a)
        c64, n64, a64 = refs[F64]
        c32, n32, a32 = refs[F32]
        # the rays whose n (and, for MIP, argmax) the f64 ray setup reproduces
        same = (n64 == n[v].reshape(-1).cpu().long()) & (n32 == n64)
        if mode == "max":
            same &= (a64 == arg[v].reshape(-1).cpu().long()) & (a32 == a64)
        share = float(same.float().mean())
        print(f"{name} {mode} view {v}: compared share {share:.3f}")
        assert share >= 0.9, (name, mode, v, share)
        got = dray[v].reshape(-1, 3).double().cpu()
        assert float(c64[same].abs().max()) > 0
        B._d8_check(got[same], c64[same], c32[same], ("d look_from per ray", name, mode, v))
        # the total: the reference on the compared rays, the kernel's own rows on the others
        rest = got[~same].sum(0)
        B._d8_check(dcam[v].double().cpu(), c64[same].sum(0) + rest, c32[same].sum(0) + rest, ("d look_from", name, mode, v))


# ---- D: the MIP's arg_max, its d_vol at the kernel's own arg_max, stale indices -------------------------------------------

@pytest.mark.parametrize("name", sorted(PR.MIP_CASES))
def test_mip_arg_max_and_its_volume_gradient(name):
    from differender_amd import functional as F
    case = PR.MIP_CASES[name]
    S, own = case["S"], case["own"]
    vol, vals, cam, e, x, r, n = _setup(case, 11, lo=-0.3)
    out, arg = F.project_fwd(vol, cam, e, x, r, n, S, "max")
    g = _randn(tuple(n.shape), 42)
    dvol = F.project_bwd(vol, cam, e, x, r, n, g, S, "max", arg)
    torch.cuda.synchronize()
    for v in range(n.shape[0]):
        bufs = _bufs(cam, e, x, r, n, v, F64)
        nn = bufs[-1]
        vv = (vals[v] if own else vals).double()
        best, a64, gap = PR.project_top2(vv, *bufs, S)
        a = arg[v].reshape(-1).cpu().long()
        got = out[v].reshape(-1).double().cpu()
        live = nn > 1
        m = nn if S is None else torch.clamp(nn, max=S)
        assert live.sum() >= 50 and bool(((a >= 0) == live).all()) and bool((a[live] < m[live]).all()) and bool((a[~live] == -1).all())
        if S is not None:
            assert float((nn[live] > S).float().mean()) > 1 / 3
        scale = float(best.abs().max())
        at = PR.sample_at(vv, *bufs, a)
        assert float((at - got).abs().max()) <= 1e-5 * scale, (name, v)      # out is the value at arg_max ...
        assert float((at - best).abs().max()) <= 1e-5 * scale, (name, v)     # ... which is the maximum
        clear = live & (gap > 1e-4 * scale)
        share = float(clear[live].float().mean())
        print(f"{name} view {v}: clear maxima {share:.4f}, arg_max differs on {int((a != a64).sum())} rays")
        assert share >= 0.95, (name, v, share)
        assert bool((a[clear] == a64[clear]).all()), (name, v)               # ... and, where it is a clear one, the first
    _check_dvol(dvol, vals, own, (cam, e, x, r, n), g, _at_fn(arg), ("MAX d_vol", name))


def test_stale_arg_max_entries_contribute_nothing():
    from differender_amd import functional as F
    case = PR.MIP_CASES["clipped"]
    S = case["S"]
    vol, vals, cam, e, x, r, n = _setup(case, 11, lo=-0.3)
    out, arg = F.project_fwd(vol, cam, e, x, r, n, S, "max")
    g = _randn(tuple(n.shape), 43)
    m = torch.clamp(n, max=S)
    live = torch.nonzero((n > 1).reshape(-1))[:, 0].cpu()
    pick = live[torch.randperm(live.numel(), generator=torch.Generator().manual_seed(1))[:36]].to(B._dev())
    stale = arg.clone().reshape(-1)
    stale[pick[:12]] = -1
    stale[pick[12:24]] = m.reshape(-1)[pick[12:24]]          # one past the last sample taken (a sample of the unclipped ray)
    stale[pick[24:]] = m.reshape(-1)[pick[24:]] + 7
    stale = stale.reshape(arg.shape)
    assert bool((n.reshape(-1)[pick[12:]] > S + 7).any())
    bad = torch.zeros(n.numel(), dtype=torch.bool, device=B._dev())
    bad[pick] = True
    bad = bad.reshape(n.shape)
    dvol = F.project_bwd(vol, cam, e, x, r, n, g, S, "max", stale)
    dcam, dray = F.project_bwd_cam(vol, cam, e, x, r, n, g, S, "max", stale, fov_deg=case["fov"], jitter_seed=case["seed"],
                                   per_ray=True)
    _, dray_fresh = F.project_bwd_cam(vol, cam, e, x, r, n, g, S, "max", arg, fov_deg=case["fov"], jitter_seed=case["seed"],
                                      per_ray=True)
    torch.cuda.synchronize()
    g0 = torch.where(bad, torch.zeros_like(g), g)
    _check_dvol(dvol, vals, False, (cam, e, x, r, n), g0, _at_fn(arg), "MAX d_vol, stale arg_max")
    assert bool((dray[bad] == 0).all()) and bool((dray_fresh[bad] != 0).any())
    assert torch.equal(dray[~bad], dray_fresh[~bad])
    _check_total(dcam, dray, "stale arg_max")


# ---- F: non-finite upstream gradients ------------------------------------------------------------------------------------

def _nonfinite_case(mode):
    from differender_amd import functional as F
    case = PR.EDGE_CASES["full_strided"]
    vol, vals, cam, e, x, r, n = _setup(case, 6, lo=-0.3 if mode == "max" else 0.0)
    _, arg = F.project_fwd(vol, cam, e, x, r, n, None, mode)
    live = torch.nonzero((n > 1).reshape(-1))[:, 0].cpu()
    order = live[torch.randperm(live.numel(), generator=torch.Generator().manual_seed(2))].to(B._dev())
    fn = _sum_fn(None) if mode == "sum" else _at_fn(arg)
    return case, vol, vals, cam, e, x, r, n, arg, order, fn


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_nan_upstream_gradients_contribute_nothing(mode):
    from differender_amd import functional as F
    case, vol, vals, cam, e, x, r, n, arg, order, fn = _nonfinite_case(mode)
    g0 = _randn(tuple(n.shape), 44)
    bad = torch.zeros(n.numel(), dtype=torch.bool, device=B._dev())
    bad[order[:max(8, order.numel() // 20)]] = True
    bad = bad.reshape(n.shape)
    gn = torch.where(bad, torch.full_like(g0, float("nan")), g0)
    g0 = torch.where(bad, torch.zeros_like(g0), g0)
    for variant in ((0, 1) if mode == "sum" else (0,)):
        d = F.project_bwd(vol, cam, e, x, r, n, gn, None, mode, arg, variant=variant)
        assert bool(torch.isfinite(d).all()), (mode, variant)
        _check_dvol(d, vals, False, (cam, e, x, r, n), g0, fn, ("d_vol, NaN upstream", mode, variant))
    kw = dict(fov_deg=case["fov"], jitter_seed=case["seed"], per_ray=True)
    dcam, dray = F.project_bwd_cam(vol, cam, e, x, r, n, gn, None, mode, arg, **kw)
    _, dray0 = F.project_bwd_cam(vol, cam, e, x, r, n, g0, None, mode, arg, **kw)
    assert bool((dray[bad] == 0).all()) and bool(torch.isfinite(dray).all())
    assert torch.equal(dray[~bad], dray0[~bad]) and bool((dray0[~bad] != 0).any())
    _check_total(dcam, dray, ("NaN upstream", mode))


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_infinite_upstream_gradients_are_clamped(mode):
    from differender_amd import functional as F
    case, vol, vals, cam, e, x, r, n, arg, order, fn = _nonfinite_case(mode)
    inf = float("inf")
    g = torch.zeros(n.numel(), device=B._dev())
    g[order[:6]] = torch.tensor([inf, -inf, inf, -inf, -inf, inf], device=B._dev())
    g = g.reshape(n.shape)
    # finite_or_zero(g D) = +-1e30 for SUM, finite_or_zero(g) = +-1e30 for MAX: the upstream gradient that gives the same
    delta = torch.where(n > 1, (x.double() - e.double()) / n.clamp(min=1).double(), torch.ones_like(x, dtype=F64))
    gref = torch.where(torch.isinf(g), torch.sign(g).double() * 1e30 / (delta if mode == "sum" else 1.0), torch.zeros_like(delta))
    for variant in ((0, 1) if mode == "sum" else (0,)):
        d = F.project_bwd(vol, cam, e, x, r, n, g, None, mode, arg, variant=variant)
        assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 1e28, (mode, variant)
        _check_dvol(d, vals, False, (cam, e, x, r, n), gref, fn, ("d_vol, infinite upstream", mode, variant))
    dcam, dray = F.project_bwd_cam(vol, cam, e, x, r, n, g, None, mode, arg, fov_deg=case["fov"], jitter_seed=case["seed"],
                                   per_ray=True)
    assert bool(torch.isfinite(dray).all()) and bool(torch.isfinite(dcam).all())
    assert bool((dray[~torch.isinf(g)] == 0).all())


# ---- G: Projector with jitter, and with an f16 volume outside autocast ------------------------------------------------------

def _to_image(out, batched):
    return torch.flip(out, (2,)).permute(0, 2, 1)[:, None] if batched else torch.flip(out[0], (1,)).t()[None]


def _from_image(g, batched):
    return torch.flip(g[:, 0].permute(0, 2, 1), (2,)) if batched else torch.flip(g[0].t(), (1,))[None]


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("mode", ["sum", "max"])
def test_projector_with_jitter_hands_its_seed_to_the_backwards(mode, batched):
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    D, Hh, Ww = 20, 18, 22
    WH = (16, 12)
    pj = Projector((D, Hh, Ww), WH, mode=mode, sampling_rate=1.5, jitter=True, max_samples=40)
    vol = B._volume((3, 1, D, Hh, Ww) if batched else (1, D, Hh, Ww), 9).requires_grad_(True)
    lf = torch.tensor([B._cam(0.3 * k, 0.2, 2.8) for k in range(3)] if batched else B._cam(0.4, 0.2, 2.8), device=B._dev(),
                      requires_grad=True)
    g = _randn((3, 1, 12, 16) if batched else (1, 12, 16), 45)
    torch.manual_seed(1234)
    seed = F.new_jitter_seed()
    assert seed != 0
    torch.manual_seed(1234)
    img = pj(vol, lf)
    assert img.shape == g.shape
    (img * g).sum().backward()
    vf = vol.detach().squeeze(1).permute(0, 3, 1, 2) if batched else vol.detach().squeeze(0).permute(2, 0, 1)
    cam = lf.detach().reshape(-1, 3)
    e, x, r, n = F.ray_setup(cam, WH, vf.shape[-3:], 1.5, 30.0, 0.1, seed)
    out, arg = F.project_fwd(vf, cam, e, x, r, n, 40, mode)
    torch.testing.assert_close(img.detach(), _to_image(out, batched), rtol=1e-5, atol=1e-6)
    gk = _from_image(g, batched)
    dv = F.project_bwd(vf, cam, e, x, r, n, gk, 40, mode, arg)
    got_dv = vol.grad.squeeze(1).permute(0, 3, 1, 2) if batched else vol.grad.squeeze(0).permute(2, 0, 1)
    torch.testing.assert_close(got_dv, dv, rtol=1e-5, atol=1e-6)
    dc = F.project_bwd_cam(vf, cam, e, x, r, n, gk, 40, mode, arg, jitter_seed=seed)
    torch.testing.assert_close(lf.grad.reshape(-1, 3), dc, rtol=1e-5, atol=1e-6)
    # the draw matters to all three: neither the unjittered rays nor a backward without the seed would pass the above
    e0, x0, r0, n0 = F.ray_setup(cam, WH, vf.shape[-3:], 1.5, 30.0, 0.1, 0)
    out0, _ = F.project_fwd(vf, cam, e0, x0, r0, n0, 40, mode)
    assert not torch.allclose(out0, out, rtol=1e-5, atol=1e-6)
    dc0 = F.project_bwd_cam(vf, cam, e, x, r, n, gk, 40, mode, arg, jitter_seed=0)
    assert not torch.allclose(dc0, dc, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_projector_runs_an_f16_volume_outside_autocast(mode):
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    D, Hh, Ww = 20, 18, 22
    WH = (16, 12)
    pj = Projector((D, Hh, Ww), WH, mode=mode, sampling_rate=1.5, jitter=False)
    vol = B._volume((1, D, Hh, Ww), 9).half().requires_grad_(True)
    lf = torch.tensor(B._cam(0.4, 0.2, 2.8), device=B._dev(), requires_grad=True)
    img = pj(vol, lf)
    assert img.dtype == F32
    g = _randn((1, 12, 16), 46)
    (img * g).sum().backward()
    vf = vol.detach().squeeze(0).permute(2, 0, 1)
    assert vf.dtype == torch.float16
    cam = lf.detach().reshape(1, 3)
    e, x, r, n = F.ray_setup(cam, WH, vf.shape, 1.5, 30.0, 0.1, 0)
    out, arg = F.project_fwd(vf, cam, e, x, r, n, None, mode)
    assert torch.equal(img.detach(), _to_image(out, False))
    ref, _ = PR.project(vf.double().cpu(), *_bufs(cam, e, x, r, n, 0, F64), None, mode)
    assert float((out.reshape(-1).double().cpu() - ref).abs().max()) <= (2e-6 if mode == "sum" else 1e-5) * float(ref.abs().max())
    gk = _from_image(g, False)
    dv = F.project_bwd(vf, cam, e, x, r, n, gk, None, mode, arg)
    assert vol.grad.dtype == torch.float16
    # autograd rounds the float32 d_vol to the volume's f16 once: 2^-11 relative (2^-10 leaves the atomics' order room), and the
    # Projector test's atol covers f16's subnormal spacing (6e-8)
    torch.testing.assert_close(vol.grad.squeeze(0).permute(2, 0, 1).float(), torch.nan_to_num(dv), rtol=2.0 ** -10, atol=1e-6)
    dc = F.project_bwd_cam(vf, cam, e, x, r, n, gk, None, mode, arg)
    torch.testing.assert_close(lf.grad.reshape(1, 3), dc, rtol=1e-5, atol=1e-6)
