"""The depth march on the GPU: dr_march_depth_fwd / _bwd against the float64 transliteration
(tests/depth_reference.py) on the kernels' own ray buffers under light_gpu.bound, the alpha channel and `steps` against the plain
colour march's bits, the three table tiers of d_tf, accumulation and batching, a view that misses the box, the camera and pose
gradients on the references' buffers under camgrad_gpu.d8_rule / pose_gpu.pose_rule, the module end to end, and the example."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import camgrad_gpu as K  # noqa: E402
import depth_gpu as DG  # noqa: E402
import depth_reference as DR  # noqa: E402
import pose_gpu as PG  # noqa: E402
from depth_gpu import C, dev  # noqa: E402
from light_gpu import bound  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = lambda: torch.device("cuda")


def _F():
    from differender_amd import functional as F
    return F


# ---- 1. forward and volume / TF backward against float64 -------------------------------------------------------------------------

@pytest.mark.parametrize("name,f16", DG.MARCH_CASES, ids=lambda v: v if isinstance(v, str) else ("f16" if v else "f32"))
def test_forward_and_backward_match_the_f64_reference(hiplib, name, f16):
    fs = DG.forward_state(name, f16)
    st, out, steps, S, sr = (fs[k] for k in ("st", "out", "steps", "S", "sr"))
    e, x, r, n = fs["rays"]
    nn, ss = n.cpu().numpy()[0], steps.cpu().numpy()[0]
    W, H = nn.shape
    # the case's own premise
    if name == "b_sr2_ert":
        assert ((ss < nn) & (nn > 1)).sum() > 20          # rays that terminate early
    if name == "c_clip":
        assert (nn > S).sum() > 20 and ss.max() == S      # the max_samples clip
    if name == "d_jitter":
        assert int(fs["inp"]["jitter_seed"]) == 4242 and int(fs["inp"]["view"]) != 0
    if name == "e_nonsquare":
        assert (W, H) == (20, 12) and ((W + 7) // 8) * ((H + 7) // 8) == 6   # a second, partly empty workgroup; partial tiles
    if name == "j_inside":
        assert (C(e) < 0).all() and (nn > 1).all()
    ref, ref32, mask = st["ref"], st["ref32"], st["mask"]
    m4 = mask[..., None]
    got = C(out)
    assert (got[..., 2] == 0).all() and np.isfinite(got).all()
    assert (got[nn[None] <= 1] == 0).all() and (ss[nn <= 1] == 0).all()   # H6
    bound(got * m4, ref["moments"] * m4, ref32["moments"] * m4, "moments")
    for k in (0, 1, 3):
        bound((got * m4)[..., k], (ref["moments"] * m4)[..., k], (ref32["moments"] * m4)[..., k], f"moments[{k}]")
    gm = dev(st["gm"])
    d_vol, d_tf = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, S, sr, gm, out)
    assert d_vol.dtype == torch.float32 and d_vol.shape == fs["vol"].shape
    bound(C(d_vol), ref["dvol"], ref32["dvol"], "dvol")
    assert (C(d_tf)[:, :3] == 0).all() and (ref["dtf"][:, :3] == 0).all()
    bound(C(d_tf)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf alpha")
    # either gradient alone is the same program
    only_v, none_t = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, S, sr, gm, out, want_tf=False)
    none_v, only_t = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, S, sr, gm, out, want_vol=False)
    assert none_t is None and none_v is None
    bound(C(only_v), ref["dvol"], ref32["dvol"], "dvol alone")
    bound(C(only_t)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf alone")


# ---- 2. the same bits as the plain colour march ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a_orbit_sr1", "b_sr2_ert", "d_jitter"])
def test_alpha_and_steps_are_the_plain_colour_marchs_bits(hiplib, name):
    """Channel 3 and `steps` against DR_VARIANT_BASELINE's alpha and steps on the same buffers: the same statements in the same
    order. A single-sample ray (n == 1) is where the two programs differ by their definitions: the colour march samples it at
    s / (n - 1) = 0 / 0 (H6), the depth march renders 0 with 0 steps."""
    from differender_amd import _native as N
    fs = DG.forward_state(name)
    colour, csteps = _F().march_fwd(fs["vol"], fs["tf"], fs["cam"], *fs["rays"], fs["S"], fs["sr"], variant=N.DR_VARIANT_BASELINE,
                                   workspace=None)
    got, steps, n = fs["out"].cpu().numpy(), fs["steps"].cpu().numpy(), fs["rays"][3].cpu().numpy()
    many = n != 1
    assert (n > 1).sum() > 100
    assert np.array_equal(got[..., 3][many], colour.cpu().numpy()[..., 3][many]) and got[..., 3].max() > 0
    assert np.array_equal(steps[many], csteps.cpu().numpy()[many])
    assert (got[~many] == 0).all() and (steps[~many] == 0).all()
    assert (got[..., 2] == 0).all()


# ---- 3. d_tf through the three table tiers ---------------------------------------------------------------------------------------

_small_scene, _small_state, _raw_bwd = DG.small_scene, DG.small_state, DG.raw_bwd   # (shared with test_gpu_depth_edges.py)


@pytest.mark.parametrize("R", [8, 3393, 10177])
def test_d_tf_through_the_three_table_tiers(hiplib, R):
    """R = 8: the table and its double gradient table in LDS; 3393: the table only, d_tf by float atomics; 10177: nothing in LDS."""
    fs = _small_state(*_small_scene(R))
    e, x, r, n = fs["rays"]
    d_vol, d_tf = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, fs["S"], fs["sr"], dev(fs["st"]["gm"]), fs["out"])
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    got = C(d_tf)
    assert got.shape == (R, 4) and (got[:, :3] == 0).all()
    bound(got[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], f"dtf alpha R {R}")
    bound(C(d_vol), ref["dvol"], ref32["dvol"], f"dvol R {R}")
    m4 = fs["st"]["mask"][..., None]
    bound(C(fs["out"]) * m4, ref["moments"] * m4, ref32["moments"] * m4, f"moments R {R}")


# ---- 4. accumulation and batching ------------------------------------------------------------------------------------------------

def test_prefilled_gradients_come_back_as_prefill_plus_gradient(hiplib):
    fs = _small_state(*_small_scene())
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    d_vol, d_tf = torch.full_like(fs["vol"], 0.5), torch.full_like(fs["tf"], -0.25)
    _raw_bwd(fs, dev(fs["st"]["gm"]), d_vol, d_tf)
    bound(C(d_vol) - 0.5, ref["dvol"], ref32["dvol"], "dvol over a pre-fill")
    assert (C(d_tf)[:, :3] == -0.25).all()   # the colour columns are never written
    bound(C(d_tf)[:, 3] + 0.25, ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf alpha over a pre-fill")


def test_two_views_sharing_a_volume_sum_their_gradients(hiplib):
    vol, tf, cams, g = _small_scene(views=2)
    fs = _small_state(vol, tf, cams, g)
    e, x, r, n = fs["rays"]
    gm = dev(fs["st"]["gm"])
    F = _F()
    both_v, both_t = F.march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, fs["S"], fs["sr"], gm, fs["out"])
    singles = [F.march_depth_bwd(fs["vol"], fs["tf"], fs["cam"][v:v + 1], e[v:v + 1], x[v:v + 1], r[v:v + 1], n[v:v + 1], fs["S"],
                                 fs["sr"], gm[v:v + 1], fs["out"][v:v + 1]) for v in range(2)]
    for k, got in ((0, both_v), (1, both_t)):
        want = C(singles[0][k]) + C(singles[1][k])
        assert np.abs(C(singles[0][k]) - C(singles[1][k])).max() > 1e-3 * np.abs(want).max()
        bound(C(got), want, want, ("dvol", "dtf")[k] + " of two views = the sum of the single views")
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    bound(C(both_v), ref["dvol"], ref32["dvol"], "dvol two views")
    bound(C(both_t)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf two views")


def test_per_view_volumes_and_tables_get_their_own_gradients(hiplib):
    vol, tf, cams, g = _small_scene(views=3, per_view=True, seed=1)
    fs = _small_state(vol, tf, cams, g, seed=9)
    e, x, r, n = fs["rays"]
    d_vol, d_tf = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, fs["S"], fs["sr"], dev(fs["st"]["gm"]), fs["out"])
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    for k, got in (("dvol", C(d_vol)), ("dtf", C(d_tf))):
        assert got.shape == ref[k].shape and got.shape[0] == 3
        for v in range(3):
            if k == "dtf":
                assert (got[v][:, :3] == 0).all()
            bound(got[v], ref[k][v], ref32[k][v], f"{k} view {v}")
        big = np.abs(got).max()
        assert all(np.abs(got[a] - got[b]).max() > 1e-3 * big for a in range(3) for b in range(a)), k   # (a view stride of 0)
    m4 = fs["st"]["mask"][..., None]
    bound(C(fs["out"]) * m4, ref["moments"] * m4, ref32["moments"] * m4, "moments per view")


# ---- 5. a view that misses the box -----------------------------------------------------------------------------------------------

def test_a_camera_looking_away_from_the_box_gives_zeros(hiplib):
    F = _F()
    W, H, vshape = 12, 10, (10, 9, 11)
    vol_np, tf_np, _, _ = _small_scene()
    vol, tf = dev(vol_np), dev(tf_np)
    lf = torch.tensor([[2.2, 1.1, 1.7]], device=DEV())
    pose = F.pack_pose(lf, torch.tensor([4.0, 2.0, 3.5], device=DEV()))
    g = torch.ones((1, W, H, 4), device=DEV())
    for seed in (0, 9):
        e, x, r, n = F.ray_setup_pose(pose, (W, H), vshape, 1.0, jitter_seed=seed)
        assert int(n.max()) <= 1
        out, steps = F.march_depth_fwd(vol, tf, lf, e, x, r, n, 512, 1.0)
        assert int(steps.max()) == 0 and float(out.abs().max()) == 0
        d_vol, d_tf = F.march_depth_bwd(vol, tf, lf, e, x, r, n, 512, 1.0, g, out)
        d, d_ray = F.march_depth_bwd_pose(vol, tf, pose, e, x, r, n, steps, 512, 1.0, g, out, jitter_seed=seed, per_ray=True)
        c, c_ray = F.march_depth_bwd_cam(vol, tf, lf, e, x, r, n, steps, 512, 1.0, g, out, jitter_seed=seed, per_ray=True)
        for t in (d_vol, d_tf, d, d_ray, c, c_ray):
            assert bool((t == 0).all()) and bool(torch.isfinite(t).all())


# ---- 6. camera and pose ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,posed,f16", DG.CAMERA_CASES,
                         ids=["-".join((n, DG.case_id(p)) + (("f16",) if h else ())) for n, p, h in DG.CAMERA_CASES])
def test_camera_and_pose_gradients_match_the_f64_reference(hiplib, name, posed, f16):
    inp, ref, ref32 = DG.camera_refs(name, posed, f16)
    what = (name, DG.case_id(posed), "f16" if f16 else "f32")
    if name == "d_jitter":
        assert int(inp["jitter_seed"]) != 0 and int(inp["view"]) != 0   # view_base != 0 with jitter
    ray, total, mask, _ = DG.one(inp, ref, ref32, posed, f16)
    assert ray.shape[-1] == (10 if posed else 3)
    DG.rule(ray, total, ref, ref32, mask, posed, what)      # (asserts that rays outside the mask are exactly 0)
    for _, sl in (PG.COLUMNS if posed else K.LOOK_FROM):    # every tensor has a gradient in every case
        assert np.abs(ray[..., sl]).max() > 0
    ray, total, mask, _ = DG.one(inp, ref, ref32, posed, f16, keep=DG.good_rays(ref, ref32, posed, what))
    DG.rule(ray, total, ref, ref32, mask, posed, what + ("conditioned",))


@pytest.mark.parametrize("posed", [True, False], ids=DG.case_id)
def test_a_nan_upstream_gradient_zeroes_its_ray_only(hiplib, posed):
    """D5: the ray whose upstream gradient is NaN contributes exactly 0, an infinite one is clamped, every other ray's result is
    the same bits, and the totals stay finite. Channel 2 of the upstream gradient is never used: a NaN there changes nothing."""
    inp, ref, ref32 = DG.camera_refs("b_sr2_ert", posed)
    clean, clean_total, mask, _ = DG.one(inp, ref, ref32, posed)
    ii, jj = np.nonzero(mask & (np.abs(clean).max(-1) > 0))
    (na, nb), (fa, fb) = (ii[0], jj[0]), (ii[len(ii) // 2], jj[len(ii) // 2])

    def poison(g):
        g = g.clone()
        g[0, na, nb, 1] = float("nan")
        g[0, fa, fb, 3] = float("inf")
        return g

    ray, total, mask2, _ = DG.one(inp, ref, ref32, posed, upstream=poison)
    assert np.array_equal(mask, mask2)
    assert (ray[na, nb] == 0).all()
    assert np.isfinite(ray).all() and np.isfinite(total).all()
    others = np.ones(mask.shape, bool)
    others[na, nb] = others[fa, fb] = False
    assert np.array_equal(ray[others], clean[others])

    def unused_channel(g):
        g = g.clone()
        g[..., 2] = float("nan")
        return g

    ray, total, _, _ = DG.one(inp, ref, ref32, posed, upstream=unused_channel)
    assert np.array_equal(ray, clean) and np.array_equal(total, clean_total)


def test_the_conditioned_rule_rejects_a_one_percent_error():
    """camgrad_gpu.mutation_check's two mutations with arrays in the kernel's place, on d_jitter under the pose (the one case
    with an ill-conditioned ray): with the float32 reference as the answer the rule passes, with every per-ray gradient 1 % too
    large it raises -- over the well-conditioned rays and, here, over all kept rays as well. mutation_check itself also asserts
    that the rule over ALL rays accepts the 1 % error, the premise of a lit march (a ray next to a lighting kink puts err32 at
    percents of the scale); this march has no kinks, its worst ray is 2.4e-4 of the scale off, and that assertion does not
    hold: the conditioned rule is not what makes the check bite here, and the test says so."""
    _, ref, ref32 = DG.camera_refs("d_jitter", True)
    keep = PG.keep(ref, ref32)
    good = DG.good_rays(ref, ref32, True)
    assert good.sum() < (keep & (ref["n"] > 1)).sum()   # there is an ill-conditioned ray to leave out
    with pytest.raises(AssertionError, match="fails the rule over all rays"):
        K.mutation_check(PG.pose_rule, ref["dpose_ray"], ref32["dpose_ray"], ref, ref32, keep, good)
    for mask in (keep & (ref["n"] > 1), good):
        m = mask[..., None]
        PG.pose_rule(ref32["dpose_ray"] * m, (ref32["dpose_ray"] * m).sum((0, 1)), ref, ref32, mask)
        wrong = 1.01 * ref["dpose_ray"] * m
        with pytest.raises(AssertionError):
            PG.pose_rule(wrong, wrong.sum((0, 1)), ref, ref32, mask)


# ---- 7. the module, end to end ---------------------------------------------------------------------------------------------------

VSHAPE, OSHAPE, R_MOD = (10, 9, 11), (10, 12), 8   # (D, H, W); the image's two extents as the module takes them
POSES = [dict(look_from=(2.2, 1.1, 1.7), fov=26.0), dict(look_from=(-1.7, 1.4, 1.9), fov=31.0)]
LOOK_AT, UP = (0.1, -0.05, 0.08), (0.15, 1.0, -0.1)


@functools.lru_cache(maxsize=None)
def _module_inputs():
    rng = np.random.RandomState(21)
    vol = PG.F32(np.clip(0.5 + 0.25 * rng.standard_normal((1, *VSHAPE)), 0.0, 1.0))     # (1, D, H, W)
    tf = rng.uniform(0.05, 0.95, (4, R_MOD))
    tf[3] = np.linspace(0.02, 0.08, R_MOD)    # thin: no ray terminates early
    return vol, PG.F32(tf)


def _to_kernel(g_user):
    """A gradient of the module's ([3,H,W]) moments -> the kernels' (W,H,4) upstream gradient (channel 2 unused)."""
    k = np.flip(g_user, -2).transpose(2, 1, 0)
    out = np.zeros(k.shape[:2] + (4,))
    out[..., 0], out[..., 1], out[..., 3] = k[..., 0], k[..., 1], k[..., 2]
    return out


def _to_user(m_kernel):
    """The kernels' (W,H,4) moments -> the module's (3,H,W)."""
    return np.flip(m_kernel[..., [0, 1, 3]].transpose(2, 1, 0), -2).copy()


def _view_reference(v, w_d, w_v):
    """View v of the module scene through the float64 and the float32 transliteration, each chained through expected_depth and
    depth_variance under the upstream weights w_d, w_v (H,W) in its own precision and on its own ray buffers: the float32
    program is float32 from the ray setup to the helpers' gradient, as the module is.
    -> [(inputs with the chained grad_out, reference)] for float64, float32."""
    from differender_amd.depth import depth_variance, expected_depth
    vol, tf = _module_inputs()
    p = POSES[v]
    base = dict(vol=vol[0].transpose(2, 0, 1).copy(), tf=tf.T.copy(), look_from=PG.F32(p["look_from"]), look_at=PG.F32(LOOK_AT),
                up=PG.F32(UP), fov_rad=PG.F32(np.deg2rad(np.float32(p["fov"]))),   # (radians in float32, as the module forms them)
                sr=np.float64(1.0), max_samples=np.int32(512), jitter_seed=np.int64(0), view=np.int32(v),
                grad_out=np.zeros((OSHAPE[0], OSHAPE[1], 4)))
    out = []
    for dtype in (torch.float64, torch.float32):
        fwd = DR.run_case(base, dtype=dtype)
        m = torch.from_numpy(_to_user(fwd["rgba"])).to(dtype).requires_grad_(True)
        wd, wv = torch.from_numpy(w_d).to(dtype), torch.from_numpy(w_v).to(dtype)
        ((expected_depth(m) * wd).sum() + (depth_variance(m) * wv).sum()).backward()
        inp = dict(base, grad_out=_to_kernel(m.grad.double().numpy()))
        out.append((inp, DR.run_case(inp, dtype=dtype)))
    return out


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
def test_depth_module_end_to_end(hiplib, batched):
    from differender_amd.depth import DepthRaycaster, depth_variance, expected_depth
    from differender_amd.volume_raycaster import Raycaster
    vol_np, tf_np = _module_inputs()
    views = 2 if batched else 1
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV())
    vol, tf = t(vol_np).requires_grad_(True), t(tf_np).requires_grad_(True)
    lf = t([p["look_from"] for p in POSES[:views]] if batched else POSES[0]["look_from"]).requires_grad_(True)
    fov = t([p["fov"] for p in POSES[:views]] if batched else POSES[0]["fov"]).requires_grad_(True)
    la, up = t(LOOK_AT).requires_grad_(True), t(UP).requires_grad_(True)
    rc = DepthRaycaster(VSHAPE, OSHAPE, R_MOD, jitter=False, camera_grad=True)
    m = rc(vol, tf, lf, look_at=la, up=up, fov=fov)
    H, W = OSHAPE[1], OSHAPE[0]
    assert m.shape == ((views,) if batched else ()) + (3, H, W)

    # channel A is the alpha channel of Raycaster's image (D4's bar: Raycaster may take the brick path)
    with torch.no_grad():
        colour = Raycaster(VSHAPE, OSHAPE, R_MOD, jitter=False)(vol.detach(), tf.detach(), lf.detach(), look_at=la.detach(),
                                                                up=up.detach(), fov=fov.detach())
    assert colour.shape[-3] == 4 and float(colour[..., 3, :, :].max()) > 0
    assert float((m[..., 2, :, :].detach() - colour[..., 3, :, :]).abs().max()) <= 1e-5

    rng = np.random.RandomState(8)
    w_d, w_v = rng.standard_normal((views, H, W)), rng.standard_normal((views, H, W))
    sel = (lambda a: a) if batched else (lambda a: a[0])
    (expected_depth(m) * t(sel(w_d))).sum().add((depth_variance(m) * t(sel(w_v))).sum()).backward()

    cases = [_view_reference(v, PG.F32(w_d[v]), PG.F32(w_v[v])) for v in range(views)]
    refs64, refs32 = [c[0][1] for c in cases], [c[1][1] for c in cases]
    # the scene's premise: the kernels' rays are the references' (no ray at a sample-count boundary, none terminates early)
    for v, (ref, ref32) in enumerate(zip(refs64, refs32)):
        assert np.array_equal(ref["steps"], ref["n"] * (ref["n"] > 1)) and np.array_equal(ref32["n"], ref["n"])
        got_steps = (rc._steps if batched else rc._steps[None])[v].cpu().numpy()
        assert np.array_equal(got_steps, ref["steps"]), "move the camera: a ray sits at a sample-count boundary"
        bound(C(m if batched else m[None])[v], _to_user(ref["rgba"]), _to_user(ref32["rgba"]), f"module moments view {v}")

    # volume and TF gradients: each transliteration over the views on its own ray buffers, under its own chained upstream
    def over_views(k, dtype):
        inps, refs_ = [c[k][0] for c in cases], [c[k][1] for c in cases]
        stack = lambda key: np.stack([r[key] for r in refs_])
        return DR.run(inps[0]["vol"], inps[0]["tf"], np.stack([i["look_from"] for i in inps]), stack("entry"), stack("exit"),
                      stack("rays"), stack("n"), np.stack([i["grad_out"] for i in inps]), 512, 1.0, dtype=dtype)

    r64, r32 = over_views(0, torch.float64), over_views(1, torch.float32)
    user_vol = lambda d: d.transpose(1, 2, 0)[None]   # (W, D, H) -> (1, D, H, W)
    bound(C(vol.grad), user_vol(r64["dvol"]), user_vol(r32["dvol"]), "module volume.grad")
    assert (C(tf.grad)[:3] == 0).all()
    bound(C(tf.grad)[3], r64["dtf"][:, 3], r32["dtf"][:, 3], "module tf.grad alpha")

    # camera gradients: the totals by D8's total rule, per tensor; fov per degree
    live = [r["n"] > 1 for r in refs64]
    per_view = [PG.COLUMNS[0][1], PG.COLUMNS[3][1]]
    deg = math.pi / 180.0
    for name, sl, leaf in zip(("look_from", "look_at", "up", "fov"), (s for _, s in PG.COLUMNS), (lf, la, up, fov)):
        scale = deg if name == "fov" else 1.0
        got = C(leaf.grad).reshape(views if (batched and sl in per_view) else 1, -1)
        if batched and sl in per_view:   # look_from and fov are batched: one gradient per view
            for v in range(views):
                K.d8_total_rule(PG._three(got[v] / scale, slice(None)), PG._three(refs64[v]["dpose_ray"], sl),
                                PG._three(refs32[v]["dpose_ray"], sl), live[v], ("module", name, v))
        else:                            # shared by the views: their sum
            want = np.concatenate([PG._three(r["dpose_ray"], sl).reshape(-1, 3) for r in refs64])
            want32 = np.concatenate([PG._three(r["dpose_ray"], sl).reshape(-1, 3) for r in refs32])
            K.d8_total_rule(PG._three(got[0] / scale, slice(None)), want, want32, np.concatenate([m_.reshape(-1) for m_ in live]),
                            ("module", name))
        assert leaf.grad.shape == leaf.shape and float(leaf.grad.abs().max()) > 0


def test_depth_module_refuses_camera_grads_without_camera_grad(hiplib):
    from differender_amd.depth import DepthRaycaster
    vol_np, tf_np = _module_inputs()
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV())
    rc = DepthRaycaster(VSHAPE, OSHAPE, R_MOD, jitter=False)
    with pytest.raises(ValueError, match="look_from"):
        rc(t(vol_np), t(tf_np), t(POSES[0]["look_from"]).requires_grad_(True))
    vol = t(vol_np).requires_grad_(True)
    m = rc(vol, t(tf_np), t(POSES[0]["look_from"]))
    m.sum().backward()
    assert float(vol.grad.abs().max()) > 0


# ---- 8. the example --------------------------------------------------------------------------------------------------------------

def test_depth_pose_recovery_example(hiplib):
    """examples/depth_pose_synthetic.py at a small size, from a start that is off in position, pan, roll and zoom at once: what
    test_pose_recovery_example asserts. The reprojection error of the box's corners, the rotation between the camera frames,
    the fov error and the loss all end below where they started; the position error alone is printed, not asserted."""
    sys.path.insert(0, ROOT)
    from examples.depth_pose_synthetic import main
    res = main(["--vol", "24", "--img", "32", "--iters", "60", "--quiet"])
    first, last, losses = res["errors"][0], res["errors"][-1], res["losses"]
    print("depth pose recovery (reprojection, position, rotation, fov)", first, "->", last, "loss", losses[0], "->", losses[-1])
    for k in (0, 2, 3):
        assert last[k] < first[k], (k, first, last)
    assert losses[-1] < losses[0]
