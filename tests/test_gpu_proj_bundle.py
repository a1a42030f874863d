"""Projections of ray bundles on the GPU: a pinhole camera's rays give dr_project_fwd's out and arg_max bit for
bit; the launch tail; the chord of a constant volume; both forwards, d_vol and the per-ray d_origin / d_dir against the float64
autograd reference of tests/proj_bundle_reference.py (the forward's bounds of tests/test_gpu_projection.py, D8's rule for the
gradients -- no other tolerance); the SUM adjoint identity; the windowed backward against the plain one on every path of the
kernel; NaN and inf upstream gradients (D5); RayBundleProjector against Projector; the parallel-beam example."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bundle_reference as BR  # noqa: E402
import proj_bundle_reference as PB  # noqa: E402
import proj_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("sum", "max")
AUTO, BASELINE = 0, 1
C = lambda t: t.detach().double().cpu().numpy()
bits = lambda t: t.contiguous().view(torch.int32)


def dev(a, dt=torch.float32):
    return torch.tensor(np.asarray(a, np.float64), dtype=dt, device="cuda")


def _F():
    from differender_amd import functional as F
    return F


def _opts(inp):
    return dict(t_near=inp.get("t_near"), jitter_seed=int(inp["jitter_seed"]), ray_base=int(inp["ray_base"]))


def _forward(inp, mode, vol=None):
    """bundle_setup + project_bundle_fwd of inp on the device (vol: the device volume in the place of inp's, as float32) ->
    (vol, o, d, e, x, n, out, arg)."""
    F = _F()
    vol = dev(inp["vol"]) if vol is None else vol
    o, d = dev(inp["origins"]), dev(inp["dirs"])
    e, x, n = F.bundle_setup(o, d, vol.shape, float(inp["sr"]), **_opts(inp))
    out, arg = F.project_bundle_fwd(vol, o, d, e, x, n, inp.get("max_samples"), mode)
    return vol, o, d, e, x, n, out, arg


def _ref_fwd(vol, o, d, e, x, n, S, mode):
    """proj_reference.project in float64 on the kernel's own ray buffers -> out, arg (numpy)."""
    T = lambda t: t.detach().double().cpu()
    out, arg = PR.project(T(vol), T(o), T(e), T(x), T(d), n.cpu().long(), S, mode)
    return out.numpy(), None if arg is None else arg.numpy()


def _check_forward(inp, mode, what, vol=None):
    vol, o, d, e, x, n, out, arg = _forward(inp, mode, vol)
    ref, ref_arg = _ref_fwd(vol, o, d, e, x, n, inp.get("max_samples"), mode)
    scale = float(np.abs(ref).max())
    err = float(np.abs(C(out) - ref).max())
    print("proj_bundle fwd", what, mode, "err/scale %.3g" % (err / scale))
    # tests/test_gpu_projection.py's bounds: SUM the f32 sum's roundings, MAX one sample whose f32 position moves its value
    assert scale > 0 and err <= (2e-6 if mode == "sum" else 1e-5) * scale, (what, mode, err / scale)
    live = n.cpu().numpy() > 1
    assert live.sum() > 0.5 * live.size and (C(out)[~live] == 0).all()
    if mode == "max":
        a = arg.cpu().numpy()
        assert ((a >= 0) == live).all() and (a[~live] == -1).all()
        assert (a == ref_arg).mean() > 0.95   # (an f32 near-tie may move an index)
    return n


# ---- 1. a pinhole camera's rays: dr_project_fwd's out and arg_max, bit for bit ------------------------------------------------------

VIEW = 3
PINHOLE = {
    # name: volume, image, sampling rate, jitter seed, camera
    "orbit_sr1": ((24, 20, 28), (16, 12), 1.0, 0, PR.orbit(0.6, 0.3, 2.7)),
    "jitter_sr0.7": ((24, 20, 28), (16, 12), 0.7, 4242, PR.orbit(2.0, -0.2, 3.0)),
    "inside": ((24, 20, 28), (16, 12), 1.0, 0, [0.3, -0.2, 0.4]),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(PINHOLE))
def test_a_pinhole_cameras_rays_give_its_projection_bit_for_bit(hiplib, case, mode):
    F = _F()
    vshape, (W, H), sr, seed, cp = PINHOLE[case]
    vol = torch.rand(vshape, generator=torch.Generator().manual_seed(11)).cuda() - (0.3 if mode == "max" else 0.0)
    cam = dev([cp])
    e0, x0, r0, n0 = F.ray_setup(cam, (W, H), vshape, sr, 30.0, 0.1, seed, VIEW)
    o, d = cam.expand(W * H, 3).contiguous(), r0.reshape(W * H, 3)
    # (view 0 of a launch whose view_base is VIEW hashes (seed, VIEW, pixel i H + j): ray_base = VIEW, p = i H + j; t_near off)
    e, x, n = F.bundle_setup(o, d, vshape, sr, None, seed, ray_base=VIEW)
    assert torch.equal(bits(e), bits(e0.reshape(-1))) and torch.equal(bits(x), bits(x0.reshape(-1))) and torch.equal(n, n0.reshape(-1))
    assert int((n > 1).sum()) > 50
    out0, arg0 = F.project_fwd(vol, cam, e0, x0, r0, n0, None, mode)
    out, arg = F.project_bundle_fwd(vol, o, d, e, x, n, None, mode)
    assert out.shape == (W * H,) and torch.equal(bits(out), bits(out0.reshape(-1)))
    assert float(out.abs().max()) > 0
    if mode == "max":
        assert arg.dtype == torch.int32 and torch.equal(arg, arg0.reshape(-1))
    else:
        assert arg is None and arg0 is None
    if case == "inside":   # the line through the camera, not the ray: samples lie behind the origin
        assert bool((e[n > 1] < 0).all())


# ---- 2. the launch tail --------------------------------------------------------------------------------------------------------------

TAIL = (1, 63, 257, 300)
CANARY = 12345.0


def _tail_run(inp, count, vol, mode):
    """The first `count` rays through the three entries on buffers 8 rays longer, pre-filled with CANARY (77 for integers)."""
    from differender_amd import _native as N
    F = _F()
    o, d = dev(inp["origins"][:count]), dev(inp["dirs"][:count])
    e, x, n = F.bundle_setup(o, d, vol.shape, float(inp["sr"]), **_opts(inp))
    pad = count + 8
    fbuf = lambda *k: torch.full((pad, *k), CANARY, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = F._proj_bundle_head(vol, o, d, e, x, n, None, mode)[3]
    out, arg = fbuf(), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    assert N.lib().dr_project_bundle_fwd(*head, out.data_ptr(), arg.data_ptr(), stream) == 0
    g = dev(inp["grad_out"][:count])
    d_o, d_d = fbuf(3), fbuf(3)
    opts = _opts(inp)
    assert N.lib().dr_project_bundle_bwd_rays(*head, -math.inf if opts["t_near"] is None else opts["t_near"], opts["jitter_seed"],
                                              opts["ray_base"], g.data_ptr(), arg.data_ptr(), d_o.data_ptr(), d_d.data_ptr(),
                                              stream) == 0
    d_vols = [F.project_bundle_bwd(vol, o, d, e, x, n, g, None, mode, arg[:count].clone(), variant=v) for v in (AUTO, BASELINE)]
    torch.cuda.synchronize()
    return dict(out=out, arg=arg, d_o=d_o, d_d=d_d), d_vols


@pytest.mark.parametrize("mode", MODES)
def test_the_launch_tail_writes_its_own_rays_and_nothing_else(hiplib, mode):
    inp = PB.inputs("random_jitter", (14, 12, 16), 1.0, rays=BR.random_bundle(max(TAIL)))
    vol = dev(inp["vol"])
    full, _ = _tail_run(inp, max(TAIL), vol, mode)
    assert float(full["d_o"][:max(TAIL)].abs().max()) > 0 and float(full["d_d"][:max(TAIL)].abs().max()) > 0
    for count in TAIL:
        got, (dw, dp) = _tail_run(inp, count, vol, mode)
        scale = float(dp.abs().max())
        assert scale > 0 and bool(torch.isfinite(dw).all()) and float((dw - dp).abs().max()) <= 1e-5 * scale, count
        for k, t in got.items():
            if mode == "sum" and k == "arg":   # not written
                assert bool((t == 77).all())
                continue
            assert torch.equal(bits(t[:count]), bits(full[k][:count])), (count, k)
            assert bool((t[count:] == (77 if t.dtype == torch.int32 else CANARY)).all()), (count, k)


# ---- 3. a constant volume: the chord -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_constant_volume_under_an_axis_parallel_bundle_gives_the_chord(hiplib, axis):
    """0.625 (exact in f16) times exit - entry, to the bound of test_gpu_projection.py's chord test. The origins lie strictly
    inside (-1, 1) on the two other axes (no 0 * inf in the slab test); five more rays outside it miss the box: n = 0, out 0."""
    F = _F()
    c, vshape, P = 0.625, (20, 18, 22), 200
    rng = np.random.RandomState(axis)
    o = rng.uniform(-0.95, 0.95, (P + 5, 3))
    o[:, axis] = rng.uniform(1.5, 3.0, P + 5)
    o[P:, (axis + 1) % 3] = rng.uniform(1.2, 2.0, 5)
    dirs = np.zeros((P + 5, 3))
    dirs[:, axis] = -1.0
    o, d = dev(o), dev(dirs)
    for seed in (0, 31):
        e, x, n = F.bundle_setup(o, d, vshape, 1.0, None, seed)
        assert bool((n[:P] >= 2).all()) and bool((n[P:] == 0).all())
        assert bool(((x - e)[:P] > 1.8).all()) and bool(((x - e)[:P] <= 2.0).all())   # the chord, less the jitter offset
        for dt in (torch.float32, torch.float16):
            vol = torch.full(vshape, c, device="cuda", dtype=dt)
            out, _ = F.project_bundle_fwd(vol, o, d, e, x, n, None, "sum")
            torch.testing.assert_close(out[:P], (c * (x - e))[:P], rtol=2e-6, atol=1e-6)
            assert bool((out[P:] == 0).all())
            top, arg = F.project_bundle_fwd(vol, o, d, e, x, n, None, "max")
            torch.testing.assert_close(top[:P], torch.full((P,), c, device="cuda"), rtol=2e-6, atol=0)
            assert bool((arg[:P] >= 0).all()) and bool((arg[P:] == -1).all()) and bool((top[P:] == 0).all())


# ---- 4. the forwards against float64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(PB.SHAPES))
@pytest.mark.parametrize("bundle", sorted(BR.BUNDLES))
def test_forward_matches_the_f64_reference(hiplib, bundle, shape, mode):
    inp = PB.inputs(bundle, *PB.SHAPES[shape])
    n = _check_forward(inp, mode, (bundle, shape))
    if bundle == "ortho":
        assert int((n == 0).sum()) == 4   # four rays of the grid miss the box


@pytest.mark.parametrize("mode", MODES)
def test_forward_clipped_anisotropic_permuted_and_f16(hiplib, mode):
    inp = PB.inputs("random", (24, 24, 24), 2.0, max_samples=17)
    n = _check_forward(inp, mode, "clipped")
    assert bool((n > 17).any())
    _check_forward(PB.inputs("random_jitter", (40, 12, 24), 1.0), mode, "aniso")
    # the user's (1, D, H, W) tensor seen as the field (W, D, H): x contiguous
    inp = PB.inputs("interior_near0", (14, 12, 16), 1.0)
    vol = dev(np.ascontiguousarray(inp["vol"].transpose(1, 2, 0))).permute(2, 0, 1)
    assert vol.stride(0) == 1 and not vol.is_contiguous() and np.array_equal(C(vol), inp["vol"])
    _check_forward(inp, mode, "permuted", vol=vol)
    inp = PB.inputs("random", (14, 12, 16), 1.0, dtype=torch.float16)
    vol = dev(inp["vol"]).half()
    assert np.array_equal(C(vol), inp["vol"])
    _check_forward(inp, mode, "f16", vol=vol)


# ---- 5. d_vol, d_origin and d_dir against autograd of the reference (D8's rule) -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _state(bundle, shape, mode):
    """The inputs and the two references of a gradient case (computed once and shared; nobody writes to them)."""
    inp = PB.inputs(bundle, *PB.SHAPES[shape])
    return inp, PB.run(inp, mode), PB.run(inp, mode, torch.float32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(PB.SHAPES))
@pytest.mark.parametrize("bundle", sorted(BR.BUNDLES))
def test_gradients_match_autograd_of_the_reference(hiplib, bundle, shape, mode):
    F = _F()
    inp, ref, ref32 = _state(bundle, shape, mode)
    vol, o, d, e, x, n, out, arg = _forward(inp, mode)
    g = dev(inp["grad_out"])
    # d_vol on the kernel's own buffers and its own argmax (an f32 near-tie can move it off the reference's), both variants
    own = [C(e), C(x), n.cpu().numpy()]
    a_own = None if arg is None else arg.cpu().numpy()
    dv64 = PB.on_buffers(inp["vol"], inp["origins"], inp["dirs"], *own, inp["grad_out"], None, mode, torch.float64, a_own)[1]
    dv32 = PB.on_buffers(inp["vol"], inp["origins"], inp["dirs"], *own, inp["grad_out"], None, mode, torch.float32, a_own)[1]
    assert (dv64 != 0).any()
    for variant in (AUTO, BASELINE):
        d_vol = F.project_bundle_bwd(vol, o, d, e, x, n, g, None, mode, arg, variant=variant)
        PB.d8_check(C(d_vol), dv64, dv32, (bundle, shape, mode, "d_vol", variant))
    # the ray gradients on the rays whose n (and argmax) float32, float64 and the kernel agree on
    d_o, d_d = F.project_bundle_bwd_rays(vol, o, d, e, x, n, g, None, mode, arg, **_opts(inp))
    same, live = PB.agree(ref, ref32, mode, n.cpu().numpy(), a_own)
    keep = same & live
    assert keep.sum() >= 0.9 * live.sum(), (keep.sum(), live.sum())
    dead = n.cpu().numpy() <= 1
    assert (C(d_o)[dead] == 0).all() and (C(d_d)[dead] == 0).all()
    PB.d8_check(C(d_o)[keep], ref["d_origin"][keep], ref32["d_origin"][keep], (bundle, shape, mode, "d_origin"))
    PB.d8_check(C(d_d)[keep], ref["d_dir"][keep], ref32["d_dir"][keep], (bundle, shape, mode, "d_dir"))
    if bundle == "random_jitter":   # the draw matters: the jitter-free gradient is another one
        other = _state("random", shape, mode)[1]
        assert np.abs(other["d_origin"] - ref["d_origin"]).max() > 1e-2 * np.abs(ref["d_origin"]).max()


# ---- 6. the SUM adjoint identity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [AUTO, BASELINE])
def test_sum_adjoint_identity(hiplib, variant):
    F = _F()
    for name in ("ortho_tiled_full", "random_300_fall_through"):
        o, d, case = PB.window_case(name)
        o, d = dev(o), dev(d)
        vol = torch.rand(case["vshape"], generator=torch.Generator().manual_seed(2)).cuda()
        e, x, n = F.bundle_setup(o, d, vol.shape, 1.3, None, 17)
        out, _ = F.project_bundle_fwd(vol, o, d, e, x, n, None, "sum")
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
        dv = F.project_bundle_bwd(vol, o, d, e, x, n, g, None, "sum", None, variant=variant)
        lhs = float((out.double() * g.double()).sum())
        rhs = float((vol.double() * dv.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((out.double().abs() * g.double().abs()).sum()), (name, lhs, rhs)


# ---- 7. the windowed backward against the plain one, on every path ------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PB.WINDOW_CASES))
def test_windowed_backward_matches_the_plain_one(hiplib, name):
    F = _F()
    o, d, case = PB.window_case(name)
    vshape = case["vshape"]
    vals = torch.rand(vshape, generator=torch.Generator().manual_seed(6)).cuda()
    vol = PR.layout_volume(vals, "x") if case["user_layout"] else vals
    o, d = dev(o), dev(d)
    e, x, n = F.bundle_setup(o, d, vshape, case["sr"], None, case["seed"], PB.RAY_BASE)
    plan = PB.group_plan(C(o), C(e), C(x), C(d), n.cpu().numpy(), vshape)   # the kernel's own buffers
    for path in case["paths"]:
        assert getattr(plan, path) > 0, (name, plan)
    g = torch.randn((o.shape[0],), generator=torch.Generator().manual_seed(7)).cuda()
    dw = F.project_bundle_bwd(vol, o, d, e, x, n, g, None, "sum", None, variant=AUTO)
    dp = F.project_bundle_bwd(vol, o, d, e, x, n, g, None, "sum", None, variant=BASELINE)
    assert dw.stride() == vol.stride()
    scale = float(dp.abs().max())
    assert scale > 0
    assert float((dw - dp).abs().max()) <= 1e-5 * scale, name
    assert int(((dw != 0) != (dp != 0)).sum()) <= int((dp.abs() < 1e-6 * scale).sum())


# ---- 8. NaN and inf upstream gradients (D5) -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_nan_and_inf_upstream_rays_are_contained(hiplib, mode):
    F = _F()
    inp, ref, _ = _state("random", "sr1", mode)
    vol, o, d, e, x, n, out, arg = _forward(inp, mode)
    P, nan_ray, inf_ray = o.shape[0], 7, 100
    assert ref["n"][nan_ray] > 1 and ref["n"][inf_ray] > 1
    g = dev(inp["grad_out"])
    run = lambda gg: F.project_bundle_bwd_rays(vol, o, d, e, x, n, gg, None, mode, arg, **_opts(inp))
    back = lambda gg, v: F.project_bundle_bwd(vol, o, d, e, x, n, gg, None, mode, arg, variant=v)
    clean = run(g)
    g_bad, g_zero = g.clone(), g.clone()
    g_bad[nan_ray], g_bad[inf_ray] = float("nan"), float("inf")
    g_zero[nan_ray] = g_zero[inf_ray] = 0.0
    got = run(g_bad)
    others = torch.ones(P, dtype=torch.bool, device="cuda")
    others[[nan_ray, inf_ray]] = False
    for a, b in zip(got, clean):
        assert bool(torch.isfinite(a).all())
        assert bool((a[nan_ray] == 0).all()) and float(b[nan_ray].abs().max()) > 0
        assert bool(((a[inf_ray].abs() == 1.0e30) | (a[inf_ray] == 0)).all())   # clamped (inf) or dropped (inf * 0, inf - inf)
        assert torch.equal(bits(a[others]), bits(b[others]))
    # d_vol: the NaN ray adds nothing, the inf ray a clamped back-projection of its own; off that ray's taps d_vol is the
    # others' (float atomics reorder: the windowed-against-plain bound)
    only_inf = torch.zeros_like(g)
    only_inf[inf_ray] = 1.0
    taps = back(only_inf, BASELINE) != 0
    assert 0 < int(taps.sum()) < taps.numel() // 4
    for variant in ((AUTO, BASELINE) if mode == "sum" else (BASELINE,)):
        want, bad = back(g_zero, BASELINE), back(g_bad, variant)
        assert bool(torch.isfinite(bad).all()) and float(bad[taps].abs().max()) > 1e28
        assert float((bad - want)[~taps].abs().max()) <= 1e-5 * float(want.abs().max())


# ---- 9. the module -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_module_on_pinhole_rays_gives_projectors_image_and_look_from_gradient(hiplib, mode):
    """RayBundleProjector on bundle.pinhole_rays against Projector with the same camera, (24, 20, 28) under a 12 x 10 image.
    Image: pinhole_rays forms its directions in float32 torch -- near_pos - look_from cancels |look_from| / near = 27 times the
    rounding of near_pos, a few 1e-6 -- and Projector's ray setup in doubles: with delta the largest difference of a direction
    component (measured here, held below 1e-5), a sample at t <= 4.5 moves by <= 4.5 delta world units in each axis, a trilinear
    value on a volume in [0, 1) with 27 voxels per 2 world units by <= 3 x 13.5 x 4.5 delta = 183 delta, and a line integral
    over a chord <= 2 sqrt(3) by <= 3.5 x 183 delta plus the chord's own change (a few delta times a value < 1): 700 delta bounds
    both modes. Compared on the rays with the same sample count (a rounding of the chord can move n).
    look_from.grad: both modules against autograd of proj_reference.project_camera by D8's rule, the upstream gradient zero
    off the rays whose n (and argmax) float64, float32, Projector's and the bundle's buffers agree on."""
    F = _F()
    from differender_amd.bundle import pinhole_rays
    from differender_amd.projection import Projector, RayBundleProjector
    (D, Hh, Ww), (W, H), cp = (24, 20, 28), (12, 10), PR.orbit(0.6, 0.3, 2.7)
    user = torch.rand((1, D, Hh, Ww), generator=torch.Generator().manual_seed(9)).cuda()
    field = user[0].permute(2, 0, 1)   # (W, D, H): what both modules hand their kernels
    up, at = torch.tensor([0.0, 1.0, 0.0], device="cuda"), torch.zeros(3, device="cuda")
    pj = Projector((D, Hh, Ww), (W, H), mode=mode, jitter=False)
    pb = RayBundleProjector((D, Hh, Ww), mode=mode, jitter=False, ray_grad=True)
    lf_p, lf_b = (dev(cp).requires_grad_(True) for _ in range(2))
    img_p = pj(user, lf_p)[0]
    ob, db = pinhole_rays(lf_b, at, up, 30.0, (W, H))
    img_b = pb(user, ob, db)
    assert img_p.shape == img_b.shape == (H, W)
    to_kernel = lambda img: torch.flip(img, (0,)).transpose(0, 1).reshape(W * H, *img.shape[2:])   # (H, W, ..) -> [W][H] rays
    # the two ray sets' buffers, as the modules made them (no jitter: seed 0)
    cam = lf_p.detach()[None]
    e0, x0, r0, n0 = F.ray_setup(cam, (W, H), field.shape, 1.0, 30.0, 0.1, 0)
    n_p = n0.reshape(-1).cpu().numpy()
    ok, dk = to_kernel(ob.detach()).contiguous(), to_kernel(db.detach()).contiguous()
    delta = float((dk - r0.reshape(-1, 3)).abs().max())
    assert delta <= 1e-5
    eb, xb, nb = F.bundle_setup(ok, dk, field.shape, 1.0, None, 0)
    n_b = nb.cpu().numpy()
    same_n = n_b == n_p
    assert same_n.mean() > 0.9
    got_p, got_b = C(to_kernel(img_p)), C(to_kernel(img_b))
    scale = float(np.abs(got_p).max())
    assert scale > 0.5 and np.abs(got_b - got_p)[same_n].max() <= 700.0 * delta
    # the references: one camera leaf, float64 and float32
    gk = np.random.RandomState(5).standard_normal(W * H)
    refs = {}
    for dt in (torch.float64, torch.float32):
        v = field.detach().cpu().to(dt)
        c = torch.tensor(cp, dtype=torch.float32).to(dt)
        _, a, (_, _, _, n_r) = PR.project_camera(v, c, W, H, 1.0, None, mode)
        refs[dt] = (n_r.numpy(), None if a is None else a.numpy())
    mask = same_n & (n_p > 1) & (refs[torch.float64][0] == n_p) & (refs[torch.float32][0] == n_p)
    if mode == "max":
        a_p = F.project_fwd(field, cam, e0, x0, r0, n0, None, mode)[1].reshape(-1).cpu().numpy()
        a_b = F.project_bundle_fwd(field, ok, dk, eb, xb, nb, None, mode)[1].cpu().numpy()
        mask &= (a_p == a_b) & (refs[torch.float64][1] == a_p) & (refs[torch.float32][1] == a_p)
    assert mask.sum() >= 0.9 * (n_p > 1).sum()
    gk = gk * mask
    want = {}
    for dt in (torch.float64, torch.float32):
        v = field.detach().cpu().to(dt)
        c = torch.tensor(cp, dtype=torch.float32).to(dt).requires_grad_(True)
        out, _, _ = PR.project_camera(v, c, W, H, 1.0, None, mode)
        (out * torch.from_numpy(gk).to(dt)).sum().backward()
        want[dt] = c.grad.double().numpy()
    g_dev = dev(gk)
    (to_kernel(img_p) * g_dev).sum().backward()
    (to_kernel(img_b) * g_dev).sum().backward()
    PB.d8_check(C(lf_p.grad), want[torch.float64], want[torch.float32], (mode, "Projector look_from"))
    PB.d8_check(C(lf_b.grad), want[torch.float64], want[torch.float32], (mode, "RayBundleProjector look_from"))


def test_module_volume_gradient_layout_autocast_and_no_grad(hiplib):
    from differender_amd.bundle import orthographic_rays, tile_order
    from differender_amd.projection import RayBundleProjector
    F = _F()
    D, Hh, Ww = 20, 18, 22
    lf = dev([1.2, 0.9, 2.0])
    o, d = orthographic_rays(lf, torch.zeros(3, device="cuda"), torch.tensor([0.0, 1.0, 0.0], device="cuda"), 1.8, (32, 16))
    perm = tile_order((16, 32)).cuda()
    o, d = o.reshape(-1, 3)[perm], d.reshape(-1, 3)[perm]
    for mode in MODES:
        pb = RayBundleProjector((D, Hh, Ww), mode=mode, sampling_rate=1.5, jitter=False, max_samples=40)
        vol = torch.rand((1, D, Hh, Ww), generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
        out = pb(vol, o, d)
        assert out.shape == (512,)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
        (out * g).sum().backward()
        field = vol.detach()[0].permute(2, 0, 1)
        e, x, n = F.bundle_setup(o, d, field.shape, 1.5, None, 0)
        want, arg = F.project_bundle_fwd(field, o, d, e, x, n, 40, mode)
        assert torch.equal(out.detach(), want) and bool((n > 40).any())
        dv = F.project_bundle_bwd(field, o, d, e, x, n, g, 40, mode, arg)
        torch.testing.assert_close(vol.grad[0].permute(2, 0, 1), dv, rtol=1e-5, atol=1e-6)
        # f16 under autocast: the result is float32, the gradient in the input's dtype
        v16 = vol.detach().half().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            o16 = pb(v16, o, d)
        assert o16.dtype == torch.float32
        o16.sum().backward()
        assert v16.grad.dtype == torch.float16 and bool(torch.isfinite(v16.grad).all())
        with torch.no_grad():
            assert bool(torch.isfinite(pb(vol, o.reshape(16, 32, 3), d.reshape(16, 32, 3))).all())


# ---- 10. the example -----------------------------------------------------------------------------------------------------------------

def test_parallel_beam_example_lowers_its_loss(hiplib):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ct_parallel_beam_synthetic.py"), "--vol", "24", "--det", "32",
                          "--views", "6", "--iterations", "12"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    m = re.search(r"loss: first ([0-9.e+-]+)\s+last ([0-9.e+-]+)", res.stdout)
    assert m, res.stdout
    assert float(m.group(2)) < float(m.group(1)), res.stdout
