"""Edges of the depth march (csrc/march_depth.hip) on the GPU: the camera kernel on both sides of its own table
boundary, the last R of each tier of the backward, the max_samples clip in the camera kernel (alone and with early termination),
sampling rates 0.6, 3 and 4, exact-zero and out-of-range voxels and axial rays, batched camera launches with per-view tables and
volumes, tiny and ragged shapes, non-dense volumes and gradient buffers, max_samples 1 and 2, and non-finite upstream
gradients. The scenes and their premises are depth_gpu's (held without a GPU by test_depth.py); the bars are the family's own:
light_gpu.bound, camgrad_gpu.d8_rule / pose_gpu.pose_rule over the kept rays and again over depth_gpu.good_rays."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_gpu as DG  # noqa: E402
import depth_reference as DR  # noqa: E402
import pose_gpu as PG  # noqa: E402
from depth_gpu import C, dev  # noqa: E402
from light_gpu import bound  # noqa: E402

pytestmark = pytest.mark.gpu

POSED = pytest.mark.parametrize("posed", [False, True], ids=DG.case_id)
ids = lambda keys: [DG.edge_id(k) for k in keys]


def _F():
    from differender_amd import functional as F
    return F


@functools.lru_cache(maxsize=None)
def _state(key):
    """An edge scene's forward_state_of (shared: nobody writes to it), its premise asserted on the kernels' own buffers."""
    fs = DG.forward_state_of(DG.edge_inputs(key))
    e, x, r, n = fs["rays"]
    fs["counts"] = DG.check_premise(key, fs["inp"], C(e)[0], C(x)[0], C(r)[0], n.cpu().numpy()[0], fs["steps"].cpu().numpy()[0])
    print("premise", DG.edge_id(key), fs["counts"])
    return fs


def _fwd_bwd(fs, what, zero_dvol=False):
    """The moments, d_vol and the alpha column of d_tf of a forward state against its float64 reference under `bound`.
    zero_dvol: the reference's d_vol is exactly 0, and so must the kernel's be. -> (d_vol, d_tf) as float64 arrays."""
    st, out = fs["st"], fs["out"]
    e, x, r, n = fs["rays"]
    ref, ref32, m4 = st["ref"], st["ref32"], st["mask"][..., None]
    got = C(out)
    assert (got[..., 2] == 0).all() and np.isfinite(got).all()
    nn = n.cpu().numpy()
    assert (got[nn <= 1] == 0).all() and (fs["steps"].cpu().numpy()[nn <= 1] == 0).all()   # H6
    bound(got * m4, ref["moments"] * m4, ref32["moments"] * m4, f"{what} moments")
    for k in (0, 1, 3):
        bound((got * m4)[..., k], (ref["moments"] * m4)[..., k], (ref32["moments"] * m4)[..., k], f"{what} moments[{k}]")
    d_vol, d_tf = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, fs["S"], fs["sr"], dev(st["gm"]), out)
    d_vol, d_tf = C(d_vol), C(d_tf)
    assert d_vol.shape == ref["dvol"].shape and d_tf.shape == ref["dtf"].shape
    if zero_dvol:
        assert (ref["dvol"] == 0).all() and (d_vol == 0).all()
    else:
        bound(d_vol, ref["dvol"], ref32["dvol"], f"{what} dvol")
    assert (d_tf[..., :3] == 0).all() and (ref["dtf"][..., :3] == 0).all()
    bound(d_tf[..., 3], ref["dtf"][..., 3], ref32["dtf"][..., 3], f"{what} dtf alpha")
    return d_vol, d_tf


# ---- 1. the camera kernel across its own table boundary --------------------------------------------------------------------------

@POSED
@pytest.mark.parametrize("R", DG.CAM_TABLE_R)
def test_camera_kernel_across_its_table_boundary(hiplib, R, posed):
    """R = 9792: the table staged in LDS beside the reductions' 6 KiB; 9793: march_depth_cam_kernel<VT, TF_LDS = false>, the
    table read where it lies. The 1-D tiers switch at 10176 / 10177: this boundary is the camera kernel's alone."""
    DG.table_tiers()
    key = DG.variant("d_jitter", posed, table=("ramp", R))
    inp, ref, ref32 = DG.edge_refs(key)
    c = DG.check_premise(key, inp, ref["entry"], ref["exit"], ref["rays"], ref["n"], ref["steps"])
    print("premise", DG.edge_id(key), c)
    DG.both_passes(key, columns_nonzero=True)


@pytest.mark.parametrize("R", DG.CAM_TABLE_R)
def test_forward_and_backward_at_the_camera_kernels_boundary(hiplib, R):
    """The same scenes through the forward and the volume / TF backward (both in tier 1 on either side): a d_tf of 9793
    texels, few samples to a texel, which a shift by one texel changes beyond any bar."""
    _fwd_bwd(_state(DG.variant("d_jitter", table=("ramp", R))), f"ramp R {R}")


# ---- 2. the last R inside each tier ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", DG.FULLEST_R)
def test_the_fullest_table_tiers(hiplib, R):
    """R = 3392: tier 2 with its LDS at its fullest (48 B a texel, the [R] double table within the [R][4] budget); 10176:
    tier 1 at its fullest. test_d_tf_through_the_three_table_tiers runs the first R of the next tier."""
    DG.table_tiers()
    fs = DG.small_state(*DG.small_scene(R))
    _fwd_bwd(fs, f"R {R}")
    if R == DG.FULLEST_R[0]:
        ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
        d_vol, d_tf = torch.full_like(fs["vol"], 0.5), torch.full_like(fs["tf"], -0.25)
        DG.raw_bwd(fs, dev(fs["st"]["gm"]), d_vol, d_tf)
        bound(C(d_vol) - 0.5, ref["dvol"], ref32["dvol"], "dvol over a pre-fill")
        assert (C(d_tf)[:, :3] == -0.25).all()   # the colour columns are never written
        bound(C(d_tf)[:, 3] + 0.25, ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf alpha over a pre-fill")


# ---- 3. the max_samples clip in the camera kernel --------------------------------------------------------------------------------

CLIP_ERT = dict(table="opaque", **DG.CLIP_ERT)


@POSED
@pytest.mark.parametrize("ert", [False, True], ids=["clip", "clip+ert"])
def test_camera_kernel_under_the_clip(hiplib, ert, posed):
    """m = min(depth_samples(n, S), fwd_steps) while f = s / (n - 1) keeps the unclipped n: the s0 / s1 weights and the direct
    term e_s under the clip -- c_clip (S = 23, no ray terminates) and c_clip at rate 2 under an opaque table with S = 80, where
    rays that stop at the clip and rays that terminate before it share the image."""
    key = DG.variant("c_clip", posed, **(CLIP_ERT if ert else {}))
    inp, ref, ref32 = DG.edge_refs(key)
    S = int(inp["max_samples"])
    c = DG.check_premise(key, inp, ref["entry"], ref["exit"], ref["rays"], ref["n"], ref["steps"])
    print("premise", DG.edge_id(key), c)
    _, _, mask = DG.both_passes(key)
    assert (mask & (ref["n"] > S) & (ref["steps"] == S)).sum() > 20               # compared, not only present
    assert not ert or (mask & (ref["steps"] < np.minimum(ref["n"], S))).sum() > 20


def test_clip_and_early_termination_on_one_image(hiplib):
    fs = _state(DG.variant("c_clip", **CLIP_ERT))
    assert fs["counts"]["clipped"] > 20 and fs["counts"]["early"] > 20
    _fwd_bwd(fs, "clip+ert")


# ---- 4. sampling rates 0.6, 3 and 4 ----------------------------------------------------------------------------------------------

RATE_CASES = [(name, sr) for name in ("b_sr2_ert", "d_jitter") for sr in DG.RATES]
rate_ids = [f"{name}-{sr:g}" for name, sr in RATE_CASES]


@pytest.mark.parametrize("name,sr", RATE_CASES, ids=rate_ids)
def test_other_sampling_rates_forward_and_backward(hiplib, name, sr):
    """0.6: pow_spec and inv_sr > 1, the derivative's exponent positive; 3: pow_spec; 4: two nested square roots. Channel 3
    and `steps` stay DR_VARIANT_BASELINE's bits (test_alpha_and_steps_are_the_plain_colour_marchs_bits)."""
    from differender_amd import _native as N
    fs = _state(DG.variant(name, sr=sr))
    assert fs["sr"] == sr and (1.0 / sr > 1.0) == (sr < 1.0)
    _fwd_bwd(fs, f"{name} rate {sr:g}")
    colour, csteps = _F().march_fwd(fs["vol"], fs["tf"], fs["cam"], *fs["rays"], fs["S"], fs["sr"], variant=N.DR_VARIANT_BASELINE,
                                   workspace=None)
    got, steps, n = fs["out"].cpu().numpy(), fs["steps"].cpu().numpy(), fs["rays"][3].cpu().numpy()
    many = n != 1
    assert np.array_equal(got[..., 3][many], colour.cpu().numpy()[..., 3][many]) and got[..., 3].max() > 0
    assert np.array_equal(steps[many], csteps.cpu().numpy()[many])
    assert (got[~many] == 0).all() and (steps[~many] == 0).all()


@POSED
@pytest.mark.parametrize("name,sr", RATE_CASES, ids=rate_ids)
def test_other_sampling_rates_camera_and_pose(hiplib, name, sr, posed):
    DG.both_passes(DG.variant(name, posed, sr=sr), columns_nonzero=True)


# ---- 5. frozen predicates of the intensity tap, axial rays -----------------------------------------------------------------------

@pytest.mark.parametrize("name", DG.FROZEN)
def test_frozen_predicates_forward_and_backward(hiplib, name):
    """m_object_in_air: samples of exactly 0 (0 < xtf is false: no gradient to the volume) -- d_vol is exactly 0 on the voxels
    that only such samples can reach, in the reference and in the kernel; n_out_of_range: samples outside [0, 1], clamped by
    the lookup; the plane and axis scenes: direction components of exactly 0."""
    fs = _state(DG.variant(name))   # (check_premise: the zero and the out-of-range samples exist on the kernels' buffers)
    d_vol, _ = _fwd_bwd(fs, name)
    if name == "m_object_in_air":
        e, x, r, n = fs["rays"]
        I, on, cell = DG.sample_values(fs["inp"]["vol"], fs["inp"]["look_from"], C(e)[0], C(x)[0], C(r)[0], n.cpu().numpy()[0],
                                       fs["steps"].cpu().numpy()[0])
        air = DG.deep_air(fs["inp"]["vol"], cell, on & (I == 0))
        assert air.sum() > 20 and (fs["st"]["ref"]["dvol"][air] == 0).all()
        assert (d_vol[air] == 0).all()
        assert np.abs(d_vol).max() > 0


@POSED
@pytest.mark.parametrize("name", DG.FROZEN)
def test_frozen_predicates_camera_and_pose(hiplib, name, posed):
    key = DG.variant(name, posed)
    _, ref, _ = DG.edge_refs(key)
    ray, _, mask = DG.both_passes(key, columns_nonzero=True)
    if name in ("i_on_x_axis", "g_plane_y0") and not posed:   # the direct term of t meets camera_ray_tail's slab-face rows
        axial = DG.axial_rays(ref) & mask
        assert axial.sum() > 0 and np.abs(ray[axial]).max(-1).min() > 0


# ---- 6. batched camera launches --------------------------------------------------------------------------------------------------

@POSED
@pytest.mark.parametrize("how", DG.BATCH_KINDS)
def test_a_batched_camera_launch(hiplib, how, posed):
    """Three views in one launch, jitter on, view_base = 5: one shared volume under a per-view (3, R, 4) table, then per-view
    f16 volumes under one table. View v's reference is the case with view = 5 + v; each view is held to its rule in both
    passes, and no two views' results agree (a view stride of 0 would give them all view 0's table or volume)."""
    trip = [DG.edge_refs(k) for k in DG.batch_keys(how, posed)]
    inps, refs, refs32 = ([t[k] for t in trip] for k in range(3))
    assert [int(i["view"]) for i in inps] == [DG.BATCH_BASE + v for v in range(DG.BATCH_VIEWS)] and int(inps[0]["jitter_seed"]) != 0
    if how == "tables":
        vol, tf = dev(inps[0]["vol"]), dev(np.stack([i["tf"] for i in inps]))
    else:
        vol, tf = dev(np.stack([i["vol"] for i in inps])).half(), dev(inps[0]["tf"])
    assert vol.ndim == (3 if how == "tables" else 4) and tf.ndim == (3 if how == "tables" else 2)
    what = (how, DG.case_id(posed))
    ray, total, mask = DG.many(vol, tf, inps, refs, refs32, posed)
    for v in range(DG.BATCH_VIEWS):
        DG.rule(ray[v], total[v], refs[v], refs32[v], mask[v], posed, what + (v,))
    for got in (ray, total):
        big = np.abs(got).max()
        assert all(np.abs(got[a] - got[b]).max() > 1e-3 * big for a in range(DG.BATCH_VIEWS) for b in range(a))
    good = [DG.good_rays(refs[v], refs32[v], posed, what + (v,)) for v in range(DG.BATCH_VIEWS)]
    ray, total, mask = DG.many(vol, tf, inps, refs, refs32, posed, good)
    for v in range(DG.BATCH_VIEWS):
        DG.rule(ray[v], total[v], refs[v], refs32[v], mask[v], posed, what + (v, "conditioned"))


# ---- 7. tiny and ragged shapes ---------------------------------------------------------------------------------------------------

tiny_ids = ["%s-%s-R%d" % ("x".join(map(str, v)), "x".join(map(str, wh)), R) for v, wh, R in DG.TINY]


@pytest.mark.parametrize("vshape,WH,R", DG.TINY, ids=tiny_ids)
def test_tiny_and_ragged_shapes_forward_and_backward(hiplib, vshape, WH, R):
    """A two-voxel volume, an image smaller than a tile, a single ray, a ragged image over several workgroups; R = 1, 2, 4, 8.
    With one texel the alpha does not depend on the volume: d_vol is exactly 0."""
    fs = _state(("tiny", vshape, WH, R, False))
    assert fs["out"].shape == (1, *WH, 4) and fs["vol"].shape == vshape
    _, d_tf = _fwd_bwd(fs, f"tiny {vshape} {WH} R {R}", zero_dvol=(R == 1))
    assert np.abs(d_tf[:, 3]).max() > 0


@POSED
@pytest.mark.parametrize("vshape,WH,R", DG.TINY, ids=tiny_ids)
def test_tiny_and_ragged_shapes_camera_and_pose(hiplib, vshape, WH, R, posed):
    ray, total, mask = DG.both_passes(("tiny", vshape, WH, R, posed))
    assert mask.sum() > 0 and np.abs(ray[..., :3]).max() > 0 and np.abs(total[:3]).max() > 0


# ---- 8. non-dense volumes and gradient buffers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_non_dense_volume_views(hiplib, vdt):
    """A slice of a larger NaN-filled tensor (nothing around it may be read) and a permuted view give the dense copy's bits in
    the forward and stay within `bound` in the backward."""
    F = _F()
    vol, tf, cams, g = DG.small_scene()
    if vdt == torch.float16:
        vol = PG.F16(vol)
    dense = dev(vol).to(vdt)
    fs = DG.small_state(vol, tf, cams, g, device_vol=dense)
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    _fwd_bwd(fs, "dense")
    sliced = torch.full((14, 12, 16), float("nan"), device=dense.device, dtype=vdt)[2:12, 1:10, 3:14]
    permuted = torch.full((11, 10, 9), float("nan"), device=dense.device, dtype=vdt).permute(1, 2, 0)
    gm = dev(fs["st"]["gm"])
    for what, view in (("sliced", sliced), ("permuted", permuted)):
        view.copy_(dense)
        assert view.shape == dense.shape and not view.is_contiguous()
        out, steps = F.march_depth_fwd(view, fs["tf"], fs["cam"], *fs["rays"], fs["S"], fs["sr"])
        assert torch.equal(steps, fs["steps"]) and torch.equal(out.view(torch.int32), fs["out"].view(torch.int32)), what
        d_vol, d_tf = F.march_depth_bwd(view, fs["tf"], fs["cam"], *fs["rays"], fs["S"], fs["sr"], gm, out)
        assert d_vol.shape == dense.shape and d_vol.dtype == torch.float32
        bound(C(d_vol), ref["dvol"], ref32["dvol"], f"dvol {what}")
        bound(C(d_tf)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], f"dtf alpha {what}")


def test_a_non_dense_gradient_buffer(hiplib):
    """d_vol with strides of its own through the raw entry: the gradient lands in the view and nowhere else."""
    fs = DG.small_state(*DG.small_scene())
    ref, ref32 = fs["st"]["ref"], fs["st"]["ref32"]
    for what, buf, view in (("sliced", torch.full((14, 12, 16), 7.0, device=fs["vol"].device), lambda b: b[2:12, 1:10, 3:14]),
                            ("permuted", torch.full((11, 12, 9), 7.0, device=fs["vol"].device), lambda b: b.permute(1, 2, 0)[:10])):
        d_vol = view(buf)
        assert d_vol.shape == fs["vol"].shape and not d_vol.is_contiguous()
        d_vol.zero_()
        d_tf = torch.zeros_like(fs["tf"])
        DG.raw_bwd(fs, dev(fs["st"]["gm"]), d_vol, d_tf)
        bound(C(d_vol), ref["dvol"], ref32["dvol"], f"dvol into a {what} buffer")
        bound(C(d_tf)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], f"dtf alpha beside a {what} buffer")
        d_vol.fill_(7.0)
        assert bool((buf == 7.0).all()), what   # nothing was written around the view


# ---- 9. max_samples = 1 and 2 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", DG.FEW_SAMPLES)
def test_one_and_two_samples_forward_and_backward(hiplib, S):
    """S = 1: every live ray composites one sample, at t0 = entry + 0.5 (exit - entry) / n: M1 = A t0, M2 = A t0^2. S = 2: the
    second sample sits at f = 1 / (n - 1) of the unclipped n, not at the exit (check_premise: n > 2 on more than 100 rays)."""
    fs = _state(DG.variant("b_sr2_ert", S=S))
    e, x, r, n = fs["rays"]
    live = n.cpu().numpy() > 1
    assert int(fs["steps"].max()) == S and fs["counts"]["clipped"] > 100
    _fwd_bwd(fs, f"S {S}")
    if S == 1:
        got = C(fs["out"])[live]
        t0 = (C(e) + 0.5 * (C(x) - C(e)) / np.maximum(n.cpu().numpy(), 1))[live]
        assert got[:, 3].min() > 0
        assert np.allclose(got[:, 0], got[:, 3] * t0, rtol=1e-6, atol=0) and np.allclose(got[:, 1], got[:, 3] * t0 * t0, rtol=1e-6, atol=0)


@POSED
@pytest.mark.parametrize("S", DG.FEW_SAMPLES)
def test_one_and_two_samples_camera_and_pose(hiplib, S, posed):
    DG.both_passes(DG.variant("b_sr2_ert", posed, S=S), columns_nonzero=True)


# ---- 10. non-finite upstream gradients in march_depth_bwd ------------------------------------------------------------------------

def _finite_close(got, ref, ref32, what):
    """Equal finiteness patterns, and the finite elements under `bound`."""
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), (what, int((np.isfinite(got) != fin).sum()))
    assert (np.isfinite(ref32) == fin).all(), what
    assert fin.any() and (~fin).any(), what
    bound(np.where(fin, got, 0.0), np.where(fin, ref, 0.0), np.where(fin, ref32, 0.0), what)


def test_non_finite_upstream_gradients_propagate_as_in_the_transliteration(hiplib):
    """A NaN pixel, a pixel with +inf in one channel and a pixel of -inf in grad_out: functional.march_depth_bwd's d_vol and
    d_tf are non-finite exactly where the float32 and float64 transliterations' are and within `bound` elsewhere ("NaN
    propagates; the caller sanitises"); DepthRaycaster's volume.grad and tf.grad are finite for such an upstream gradient."""
    vol, tf, cams, g = DG.small_scene(R=64)
    fs = DG.small_state(vol, tf, cams, g)
    e, x, r, n = fs["rays"]
    mask = fs["st"]["mask"]
    ii, jj = np.nonzero(mask[0])
    (na, nb), (pa, pb), (ma, mb) = ((ii[k], jj[k]) for k in (len(ii) // 5, len(ii) // 2, 4 * len(ii) // 5))
    gm = fs["st"]["gm"].copy()
    gm[0, na, nb] = np.nan
    gm[0, pa, pb, 0] = np.inf
    gm[0, ma, mb] = -np.inf
    args = (vol, tf, cams, C(e), C(x), C(r), n.cpu().numpy(), gm, fs["S"], fs["sr"])
    ref, ref32 = DR.run(*args, pixels=mask), DR.run(*args, dtype=torch.float32, pixels=mask)
    d_vol, d_tf = _F().march_depth_bwd(fs["vol"], fs["tf"], fs["cam"], e, x, r, n, fs["S"], fs["sr"], dev(gm), fs["out"])
    _finite_close(C(d_vol), ref["dvol"], ref32["dvol"], "dvol")
    assert (C(d_tf)[:, :3] == 0).all()
    _finite_close(C(d_tf)[:, 3], ref["dtf"][:, 3], ref32["dtf"][:, 3], "dtf alpha")

    from differender_amd.depth import DepthRaycaster
    D, H, W = 9, 11, 10   # the module's (D, H, W) of the kernels' (W, D, H) = (10, 9, 11)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=fs["vol"].device)
    user_vol = t(vol.transpose(1, 2, 0)[None]).requires_grad_(True)
    user_tf = t(tf.T).requires_grad_(True)
    m = DepthRaycaster((D, H, W), (12, 10), tf.shape[0], jitter=False)(user_vol, user_tf, t(cams[0]))
    hit = torch.nonzero(m[2] > 0).tolist()   # rays that collect something
    assert len(hit) > 20
    w = torch.ones_like(m)
    (ni, nj), (pi, pj), (mi, mj) = (hit[k] for k in (len(hit) // 5, len(hit) // 2, 4 * len(hit) // 5))
    w[:, ni, nj] = float("nan")
    w[0, pi, pj] = float("inf")
    w[:, mi, mj] = float("-inf")
    (m * w).sum().backward()
    for grad in (user_vol.grad, user_tf.grad):
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
