"""The differentiable light and Phong material on the GPU (csrc/march_lit.hip): the reference's lighting
bit for bit against the plain 1-D kernels, other lights and materials against the float64 transliteration
(tests/light_reference.py) by D8's rule, a flat volume's closed form, nullable outputs and accumulation, every LDS tier,
RaycasterLit, and the example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import light_cases as LC  # noqa: E402
import light_reference as LR  # noqa: E402
from light_gpu import C, DEV, bound as _bound, compare as _compare, raw_bwd as _raw_bwd, upload as _upload  # noqa: E402

pytestmark = pytest.mark.gpu


def _F():
    from differender_amd import functional as F
    return F


def _N():
    from differender_amd import _native as N
    return N


def _cams(views, first=0.9):
    from differender.utils import in_circles
    return torch.stack([in_circles(first + 1.7 * i).float() for i in range(views)]).to(DEV)


# --- 1. the reference's lighting: the bits of DR_VARIANT_BASELINE ----------------------------------------------------------------

@pytest.mark.parametrize("sr", [1.0, 2.0])
@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", ["diff", "nondiff"])
def test_reference_lighting_is_the_baseline_bit_for_bit(hiplib, mode, vdt, sr):
    F, N = _F(), _N()
    mode = N.DR_MODE_DIFF if mode == "diff" else N.DR_MODE_NONDIFF
    vol = torch.from_numpy(LC.synth_volume((20, 16, 24), 21)).float().to(DEV).to(vdt)
    cam = _cams(3)
    light = F.default_light(cam)
    assert torch.equal(light[:, :3], cam + torch.tensor([0.0, 1.0, 0.0], device=DEV))
    e, x, r, n = F.ray_setup(cam, (12, 20), vol.shape, sr, jitter_seed=4242)
    for R, kind in ((8, "thin"), (32, "opaque")):   # (opaque: rays terminate early)
        g = torch.Generator().manual_seed(R)
        tf = torch.rand((R, 4), generator=g) * 0.9 + 0.05
        tf[:, 3] = torch.linspace(0.0, 0.02, R) if kind == "thin" else torch.linspace(0.0, 0.95, R) ** 2
        tf = tf.to(DEV)                              # (alphas from 0: the non-differentiable march's 1e-3 skip is taken)
        ref, ref_steps = F.march_fwd(vol, tf, cam, e, x, r, n, 4096, sr, mode=mode, variant=N.DR_VARIANT_BASELINE, workspace=None,
                                     hints=0)
        out, steps = F.march_lit_fwd(vol, tf, cam, light, e, x, r, n, 4096, sr, mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(steps, ref_steps), kind
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), kind
        assert (ref[..., 3] > 0).any()
        if kind == "opaque":
            assert (ref_steps < n).any()


# --- 2. other lights and materials against the float64 transliteration (and 5: every LDS tier) -----------------------------------

@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_against_the_f64_transliteration(hiplib, name):
    sc, st, got = _compare(name)
    ref, mask, n, S = st["ref"], st["mask"], got["n"], sc["max_samples"]
    if name == "side_colour_sh7":
        assert (ref["clamped"][mask] == 0).all()                      # nothing clamps
    if name == "bright_clamps":
        assert ((ref["clamped"] > 0) & (ref["clamped"] < ref["steps"]))[mask].any()   # a kept ray has Lraw > 1 samples, and others
    if name == "lc_zero":
        assert sc["light"][0, 4] == 0.0 and abs(ref["dlight"][0, 4]) > 1e-3 * np.abs(ref["dlight"][0, 3:6]).max()
        assert abs(got["d_light"][0, 4]) > 0
    if name == "three_views":
        rows = got["d_light"]
        assert all(np.abs(rows[a] - rows[b]).max() > 1e-3 * np.abs(rows).max() for a, b in ((0, 1), (0, 2), (1, 2)))
    if name == "ert_opaque":
        assert (got["steps"] < np.minimum(n, S))[mask].any()          # a kept ray stops early
    if name == "clip_S23":
        assert (n > S)[mask].any() and (got["steps"][mask] <= S).all()


# --- 3. a flat volume ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ka", [0.55, 1.3], ids=["ka0.55", "ka1.3_clamped"])
def test_flat_volume_has_the_closed_form(hiplib, ka):
    """A volume that is 1 everywhere: every tap is exactly 1 in f32 (a + RN(1 - a) rounds to 1 for every fraction a), every
    normal is flat (D1) and every sample is lit by L = min(1, ka) alone: C_k = L c_k lc_k A, A = 1 - (1 - op)^steps, with
    (c, op) the TF's last entry. Each pixel is `steps` fused multiply-adds of exact products' roundings: (steps + 4) 2^-23
    relative. d ka is the reference's (0 where it clamps); kd, ks, sh and p receive exactly 0; nothing is NaN."""
    F = _F()
    R, WH, S = 8, (16, 16), 4096
    vol = torch.ones((14, 12, 16), device=DEV)
    g = torch.Generator().manual_seed(5)
    tf = (torch.rand((R, 4), generator=g) * 0.9 + 0.05)
    tf[:, 3] = torch.linspace(0.01, 0.06, R)
    tf = tf.to(DEV)
    cam = _cams(1, 2.3)
    light = torch.tensor([[2.4, 0.7, -1.1, 0.9, 0.6, 0.35, ka, 0.5, 0.3, 7.5]], device=DEV)
    e, x, r, n = F.ray_setup(cam, WH, vol.shape, 1.0)
    out, steps = F.march_lit_fwd(vol, tf, cam, light, e, x, r, n, S, 1.0)
    live = (n > 1).cpu().numpy()[0]
    k = steps.cpu().numpy()[0][live].astype(np.float64)
    assert live.sum() > 50 and (k == n.cpu().numpy()[0][live]).all() and len(set(k.tolist())) > 3
    c, op = C(tf)[-1, :3], C(tf)[-1, 3]
    A = 1.0 - (1.0 - op) ** k
    L = min(1.0, C(light)[0, 6])
    got = C(out)[0][live]
    tol = (k.max() + 4) * 2.0 ** -23
    assert np.abs(got[:, 3] - A).max() <= tol * A.max()
    for ch in range(3):
        want = L * c[ch] * C(light)[0, 3 + ch] * A
        assert np.abs(got[:, ch] - want).max() <= tol * want.max(), ch
    go = torch.randn((1, *WH, 4), generator=torch.Generator().manual_seed(6)).to(DEV) * (n > 1)[..., None]
    d_vol, d_tf, d_light, d_ray = F.march_lit_bwd(vol, tf, cam, light, e, x, r, n, S, 1.0, go, out, per_ray=True)
    for t in (d_vol, d_tf, d_light, d_ray):
        assert torch.isfinite(t).all()
    assert (d_light[0, [0, 1, 2, 7, 8, 9]] == 0).all() and (d_ray[..., [0, 1, 2, 7, 8, 9]] == 0).all()
    inp = dict(vol=C(vol), tf=C(tf), cam=C(cam), entry=C(e), exit=C(x), rays=C(r), n=n.cpu().numpy(), grad_out=C(go), sr=1.0,
               max_samples=S)
    ref, ref32 = LR.run(inp, C(light)), LR.run(inp, C(light), dtype=torch.float32)
    assert (ref["steps"] == steps.cpu().numpy())[n.cpu().numpy() != 1].all()
    if ka > 1.0:
        assert (ref["dlight"][0, 6] == 0) and d_light[0, 6] == 0 and (ref["clamped"] == ref["steps"]).all()
    else:
        _bound(C(d_light)[:, 6], ref["dlight"][:, 6], ref32["dlight"][:, 6], "d ka")
        _bound(C(d_ray)[..., 6], ref["dlight_ray"][..., 6], ref32["dlight_ray"][..., 6], "d ka per ray")
    _bound(C(d_light)[:, 3:6], ref["dlight"][:, 3:6], ref32["dlight"][:, 3:6], "d lc")
    _bound(C(d_tf), ref["dtf"], ref32["dtf"], "dtf")


# --- 4. nullable outputs and accumulation ---------------------------------------------------------------------------------------

def test_nullable_outputs_and_accumulation(hiplib):
    """Each output alone is what the call with all four gives: d_vol and d_tf up to the order of their float atomics (k < 1e3
    f32 addends per element: 1e-5 of the largest element, the bar of the 1-D kernels' own such test), d_light up to the order of
    a few hundred f64 atomics (1e-12), the per-ray d_light bit for bit. d_light is accumulated: a pre-filled buffer comes back as
    pre-fill + gradient."""
    F = _F()
    sc = LC.scene("three_views")
    vol, tf, cam, light = _upload(sc)
    S, sr = sc["max_samples"], sc["sr"]
    rays = F.ray_setup(cam, sc["WH"], vol.shape, sr)
    out, _ = F.march_lit_fwd(vol, tf, cam, light, *rays, S, sr)
    V, (W, H) = 3, sc["WH"]
    go = torch.randn((V, W, H, 4), generator=torch.Generator().manual_seed(9)).to(DEV)
    new = lambda: (torch.zeros_like(vol), torch.zeros_like(tf), torch.zeros((V, 10), dtype=torch.float64, device=DEV),
                   torch.full((V, W, H, 10), float("nan"), device=DEV))
    dv, dt, dl, dr = new()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, dv, dt, dl, dr)
    assert dv.abs().max() > 0 and dt.abs().max() > 0 and (dl != 0).all() and torch.isfinite(dr).all()
    dv1, dt1, dl1, dr1 = new()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_vol=dv1)
    assert (dv1 - dv).abs().max() <= 1e-5 * dv.abs().max()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_tf=dt1)
    assert (dt1 - dt).abs().max() <= 1e-5 * dt.abs().max()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_light=dl1)
    assert ((dl1 - dl).abs() <= 1e-12 * dl.abs().max(0).values).all()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_ray=dr1)
    assert torch.equal(dr1.view(torch.int32), dr.view(torch.int32))
    # ... and beside d_light alone
    dl2, dr2 = new()[2:]
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_light=dl2, d_ray=dr2)
    assert torch.equal(dr2.view(torch.int32), dr.view(torch.int32))
    assert ((dr.double().sum((1, 2)) - dl).abs() <= 1e-9 * dl.abs().max(0).values).all()   # d_light is the rays' sum
    # the functional wrapper returns the same
    fv, ft, fl, fr = F.march_lit_bwd(vol, tf, cam, light, *rays, S, sr, go, out, per_ray=True)
    assert torch.equal(fr.view(torch.int32), dr.view(torch.int32)) and (fl.double() - dl).abs().max() <= 1e-6 * dl.abs().max()
    assert F.march_lit_bwd(vol, tf, cam, light, *rays, S, sr, go, out, False, False, False) == (None, None, None)
    # accumulation
    fill = torch.arange(1.0, 31.0, dtype=torch.float64, device=DEV).reshape(V, 10)
    dl3 = fill.clone()
    _raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_light=dl3)
    assert ((dl3 - fill - dl).abs() <= 1e-12 * (fill + dl.abs().max(0).values)).all()


# --- 6. the module ------------------------------------------------------------------------------------------------------------

def _module_inputs(bs=None, seed=31):
    """User-layout inputs: volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3)."""
    D, H, W, R = 14, 12, 16, 8
    v = torch.from_numpy(LC.synth_volume((W, D, H), seed)).float().permute(1, 2, 0).contiguous()[None].to(DEV)   # (1,D,H,W)
    g = torch.Generator().manual_seed(seed)
    tf = torch.rand((4, R), generator=g) * 0.9 + 0.05
    tf[3] = torch.linspace(0.01, 0.06, R)
    lf = _cams(bs or 1, 1.3)
    return v, tf.to(DEV), (lf if bs else lf[0]), (D, H, W), R


def test_module_default_lighting_is_raycasters_image(hiplib):
    from differender_amd.lighting import RaycasterLit
    from differender_amd.volume_raycaster import Raycaster
    v, tf, lf, shape, R = _module_inputs(2)
    kw = dict(sampling_rate=1.0, jitter=False, max_samples=4096)
    img = RaycasterLit(shape, (20, 12), R, **kw)(v, tf, lf)
    ref = Raycaster(shape, (20, 12), R, **kw)(v, tf, lf)
    assert img.shape == ref.shape == (2, 4, 12, 20) and ref[:, 3].max() > 0.1
    assert (img - ref).abs().max() <= 1e-5      # the bar the fast path is held to against the oracle


LIGHTING = dict(light_pos=(2.4, 0.7, -1.1), light_color=(0.9, 0.6, 0.35), ambient=0.1, diffuse=0.5, specular=0.3, shininess=7.5)


def test_module_is_the_functional_calls_and_routes_gradients(hiplib):
    """The image and the gradients of RaycasterLit are those of ray_setup + march_lit_fwd / _bwd on the same inputs; every
    lighting tensor that requires grad gets its gradient -- a shared one the sum over the views, a per-view one its rows --
    and none that does not."""
    from differender_amd import _layout as L
    from differender_amd.lighting import RaycasterLit
    F = _F()
    v, tf, lf, shape, R = _module_inputs(2)
    WH = (20, 12)   # the module's output_shape is the kernels' (W, H); the user's image is (4, 12, 20)
    rc = RaycasterLit(shape, (20, 12), R, jitter=False, max_samples=4096, headlight=False)
    T = lambda x, grad: torch.tensor(x, device=DEV, requires_grad=grad)
    pos = torch.tensor([LIGHTING["light_pos"], (-2.2, 0.4, 1.9)], device=DEV, requires_grad=True)   # per view
    col, ka, kd = T(LIGHTING["light_color"], True), T(LIGHTING["ambient"], True), T(LIGHTING["diffuse"], False)
    ks, sh = T([LIGHTING["specular"]], True), T(LIGHTING["shininess"], True)
    vg, tg = v.clone().requires_grad_(True), tf.clone().requires_grad_(True)
    img = rc(vg, tg, lf, light_pos=pos, light_color=col, ambient=ka, diffuse=kd, specular=ks, shininess=sh)
    go = torch.randn(img.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (img * go).sum().backward()

    vol = L.field_view(v)
    light = torch.cat([pos.detach(), col.detach().expand(2, 3), torch.tensor([[0.1, 0.5, 0.3, 7.5]], device=DEV).expand(2, 4)], 1)
    rays = F.ray_setup(lf, WH, vol.shape, 1.0)
    out, _ = F.march_lit_fwd(vol, tf.t().contiguous(), lf, light, *rays, 4096, 1.0)
    assert torch.equal(L.image(out).view(torch.int32), img.detach().view(torch.int32))
    g_k = torch.flip(go.transpose(-1, -3), (-2,)).contiguous()        # the user image's gradient in the kernels' (W,H,4) layout
    dv, dt, dl = F.march_lit_bwd(vol, tf.t().contiguous(), lf, light, *rays, 4096, 1.0, g_k, out)
    close = lambda a, b: (a - b).abs().max() <= 1e-5 * b.abs().max()
    assert close(L.field_view(vg.grad), dv) and close(tg.grad, dt.t())
    assert kd.grad is None
    assert close(pos.grad, dl[:, 0:3]) and (pos.grad[0] != pos.grad[1]).any()
    assert close(col.grad, dl[:, 3:6].sum(0)) and close(ka.grad, dl[:, 6].sum()) and close(ks.grad, dl[:, 8].sum()[None])
    assert close(sh.grad, dl[:, 9].sum()) and sh.grad.shape == () and ks.grad.shape == (1,) and pos.grad.shape == (2, 3)
    for t in (pos, col, ka, ks, sh):
        assert t.grad.abs().max() > 0
    # nothing requires grad: no backward graph at all
    assert not rc(v, tf, lf, **LIGHTING).requires_grad


def test_module_headlight_offset_is_a_world_light_at_look_from_plus_offset(hiplib):
    from differender_amd.lighting import RaycasterLit
    v, tf, lf, shape, R = _module_inputs(2)
    kw = dict(jitter=False, max_samples=4096)
    o = torch.tensor([0.5, 1.5, -0.25], device=DEV)
    a = RaycasterLit(shape, (16, 16), R, headlight=True, **kw)(v, tf, lf, light_pos=o, specular=0.6, shininess=9.0)
    b = RaycasterLit(shape, (16, 16), R, headlight=False, **kw)(v, tf, lf, light_pos=lf + o, specular=0.6, shininess=9.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and a[:, 3].max() > 0.1
    c = RaycasterLit(shape, (16, 16), R, headlight=True, **kw)(v, tf, lf, specular=0.6, shininess=9.0)
    assert not torch.equal(a, c)   # the offset matters


def test_module_nondiff_and_free_camera_are_the_functional_calls(hiplib):
    from differender_amd import _layout as L
    from differender_amd.lighting import RaycasterLit
    F, N = _F(), _N()
    v, tf, lf, shape, R = _module_inputs(None)
    rc = RaycasterLit(shape, (20, 12), R, jitter=False, max_samples=64, headlight=False)
    vol, tfk = L.field_view(v), tf.t().contiguous()
    light = torch.tensor([[*LIGHTING["light_pos"], *LIGHTING["light_color"], 0.1, 0.5, 0.3, 7.5]], device=DEV)
    # raycast_nondiff: the default rate is 4x the module's, never jittered, no max_samples clip
    img = rc.raycast_nondiff(v, tf, lf, **LIGHTING)
    cam = lf[None]
    rays = F.ray_setup(cam, (20, 12), vol.shape, 4.0)
    out, steps = F.march_lit_fwd(vol, tfk, cam, light, *rays, 64, 4.0, mode=N.DR_MODE_NONDIFF)
    assert img.shape == (4, 12, 20) and torch.equal(L.image(out[0]).view(torch.int32), img.view(torch.int32))
    assert (steps > 64).any()
    # the free camera: look_at, up and a per-view fov
    look_at, up, fov = torch.tensor([0.1, -0.2, 0.05], device=DEV), torch.tensor([0.2, 1.0, 0.1], device=DEV), 24.0
    img = rc(v, tf, lf, look_at=look_at, up=up, fov=fov, **LIGHTING)
    pose9 = F.pack_pose(cam, look_at[None], up[None])
    fov_v = torch.deg2rad(torch.tensor([fov], device=DEV))
    rays = F.ray_setup_pose(pose9, (20, 12), vol.shape, 1.0, 30.0, 0.1, 0, fov_v=fov_v)
    out, _ = F.march_lit_fwd(vol, tfk, pose9[:, :3], light, *rays, 64, 1.0)
    assert torch.equal(L.image(out[0]).view(torch.int32), img.view(torch.int32)) and img[3].max() > 0.1
    assert not torch.equal(img, rc(v, tf, lf, **LIGHTING))


# --- 7. the example -----------------------------------------------------------------------------------------------------------

def test_example_recovers_light_and_material(hiplib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "light_opt_synthetic.py"), "--small"], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    first = float(r.stdout.split("first loss")[1].split()[0])
    last = float(r.stdout.split("last loss")[1].split()[0])
    assert math.isfinite(last) and last < first, r.stdout
    for group in ("position", "colour", "material"):
        a, b = (float(t) for t in r.stdout.split(group + " error")[1].split()[:3:2])
        assert math.isfinite(b) and b < a, (group, r.stdout)
