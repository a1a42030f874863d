"""The ray-bundle march at its edges, on the GPU: direction components that are exactly 0 (axis-parallel rays,
rays with one zero component, the pinhole scenes with such rays), the sample cap under a ray gradient, a t_near that some rays
take, that kills others and that is combined with jitter, single-sample rays in a wave of live ones, the partial backwards in
the three table tiers, and the ray gradients at those tiers, on an f16 and on a strided volume, and through the module on a cone
beam handed over as (H, W, 3) with directions that are not unit.

No tolerance of its own: images, d_vol and d_tf are held by light_gpu.bound, the ray gradients by test_gpu_bundle.ray_rule
(D8), a source gradient by proj_bundle_reference.d8_check, all against the float64 and float32 references of
tests/bundle_reference.py run at test time on the inputs the kernels read. tests/test_bundle.py shows without a GPU that every
bundle here keeps 80 % of its rays and that each edge changes the gradient by more than 1e-2 of its scale.

Out of scope: an origin with a coordinate of exactly +-1 on an axis whose direction component is 0. The kernels see
0 * inf = NaN there, which fminf / fmaxf drop; the reference's torch.minimum propagates it. The two programs define different
things, and no bundle of this file holds such a ray (asserted in tests/test_bundle.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bundle_reference as BR  # noqa: E402
import camgrad_gpu as K  # noqa: E402
import light_gpu as LG  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402
import pose_gpu as PG  # noqa: E402
import proj_bundle_reference as PB  # noqa: E402
from test_gpu_bundle import (D_JITTER_SEED, C, _F, _forward, _masked_refs, _opts, _parity, _pinhole, _state, bits, dev,  # noqa: E402
                             ray_rule)

pytestmark = pytest.mark.gpu


# ---- 1. the pinhole scenes with axial rays, bit for bit --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, D_JITTER_SEED], ids=["no_jitter", "jitter"])
@pytest.mark.parametrize("name", ("g_plane_y0", "h_plane_x0", "i_on_x_axis"))
def test_pinhole_scenes_with_zero_direction_components_bit_for_bit(hiplib, name, seed):
    """test_a_pinhole_cameras_rays_give_its_buffers_image_and_steps_bit_for_bit on the scenes whose camera lies in a coordinate
    plane: a row or column of the image has a direction component of exactly 0."""
    F, N = _F(), LG.native()
    inp, vol, tf, cam, (e0, x0, r0, n0), o, d = _pinhole(name, seed)
    zero = (d == 0).any(1)
    assert int(zero.sum()) >= 15 and int((n0.reshape(-1)[zero] > 1).sum()) >= 8   # such rays exist, and some of them hit
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    e, x, n = F.bundle_setup(o, d, vol.shape, sr, None, seed, ray_base=CG.VIEW)
    assert torch.equal(bits(e), bits(e0.reshape(-1))) and torch.equal(bits(x), bits(x0.reshape(-1)))
    assert torch.equal(n, n0.reshape(-1)) and int((n > 1).sum()) > 50
    out0, steps0 = F.march_fwd(vol, tf, cam, e0, x0, r0, n0, S, sr, variant=N.DR_VARIANT_BASELINE)
    out, steps = F.march_bundle_fwd(vol, tf, o, d, e, x, n, S, sr)
    assert torch.equal(bits(out), bits(out0.reshape(-1, 4))) and torch.equal(steps, steps0.reshape(-1))


# ---- 2. image, d_vol, d_tf, n and steps of every edge case -----------------------------------------------------------------------------

@pytest.mark.parametrize("scene,bundle", BR.EDGE_CASES, ids=lambda v: str(v))
def test_image_d_vol_and_d_tf_of_the_edge_cases_match_the_f64_reference(hiplib, scene, bundle):
    """test_image_d_vol_and_d_tf_match_the_f64_reference's comparison (_parity). Measured on the MI355X, d_vol as err / err32 /
    scale: a_orbit_sr1 axial 1.5e-4 / 4.6e-4 / 3.1, one_zero 8.7e-5 / 6.4e-4 / 3.9; b_sr2_ert axial 4.3e-4 / 9.8e-4 / 9.5,
    one_zero 2.0e-4 / 9.6e-4 / 10.7; c_clip random 4.7e-4 / 8.4e-4 / 3.0, ortho 1.2e-4 / 5.2e-4 / 2.9, interior_near0 1.3e-4 /
    1.2e-3 / 3.8; a_orbit_sr1 random_near2 5.4e-4 / 1.5e-3 / 6.0, random_near3 1.4e-4 / 1.5e-3 / 3.6, interior_near0_jitter
    1.1e-4 / 7.6e-4 / 2.9. d_tf: the largest err / err32 is b_sr2_ert one_zero's 2.6e-4 / 2.2e-4 of 6.2; the images are within
    1.4e-5 (err32 1.1e-5) everywhere."""
    inp, ref, ref32 = _state(scene, bundle)
    vol, tf, o, d, e, x, n, out, steps, mask = _parity(inp, ref, ref32, (scene, bundle))
    if scene == "c_clip":
        assert int(steps.max()) == 23 == int(inp["max_samples"]) and int(n.max()) > 23   # the cap bites, on the kernel's buffer
    if bundle == "random_near3":   # t_near past the exit: the ray dies (tmin > tmax)
        off = BR.run(dict(inp, t_near=None), grads=False)
        killed = ((ref["n"] == 0) & (off["n"] > 1)).reshape(-1)
        assert killed.sum() >= 8
        k = torch.from_numpy(killed).cuda()
        assert bool((n[k] == 0).all()) and bool((steps[k] == 0).all()) and bool((out[k] == 0).all())


# ---- 3. the ray gradients of every edge case ----------------------------------------------------------------------------------------------

def _ray_gradients(inp, ref, ref32, what, vol=None):
    """test_ray_gradients_match_the_f64_reference_on_the_well_conditioned_rays' body up to the rule -> the kernel's (P, 1, 6)
    gradients for the upstream gradient of the mask's rays, the mask, and the forward's buffers."""
    F = _F()
    fwd = _forward(inp, vol)
    vol, tf, o, d, e, x, n, out, steps = fwd
    good = K.well_conditioned(ref, ref32, BR.keep(ref, ref32), "dray", BR.COLUMNS, what)
    agree = (steps.cpu().numpy().reshape(-1, 1) == ref["steps"]) & (n.cpu().numpy().reshape(-1, 1) == ref["n"])
    mask = good & agree
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * mask[..., None]).reshape(-1, 4)
    d_o, d_d = F.march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]), g, out,
                                       **_opts(inp))
    return np.concatenate([C(d_o), C(d_d)], -1).reshape(-1, 1, 6), mask, fwd


def _raw_ray_gradients(inp, fwd):
    """d_origin, d_dir (P, 3) numpy for the whole upstream gradient: what the kernel stores, before any mask."""
    vol, tf, o, d, e, x, n, out, steps = fwd
    d_o, d_d = _F().march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]),
                                          dev(inp["grad_out"]), out, **_opts(inp))
    return C(d_o), C(d_d)


@pytest.mark.parametrize("scene,bundle", BR.EDGE_CASES, ids=lambda v: str(v))
def test_ray_gradients_of_the_edge_cases_match_the_f64_reference(hiplib, scene, bundle):
    """The body of test_ray_gradients_match_the_f64_reference_on_the_well_conditioned_rays and ray_rule. Measured on the MI355X,
    err / err32 over the scale, d_origin | d_dir: a_orbit_sr1 axial 2.0e-6 / 8.4e-5 | 2.6e-6 / 8.0e-5, one_zero 1.7e-5 / 9.1e-5 |
    1.7e-5 / 8.0e-5; b_sr2_ert axial 3.5e-6 / 2.2e-5 | 3.1e-6 / 2.1e-5, one_zero 9.3e-6 / 9.6e-5 | 1.1e-5 / 7.3e-5; c_clip random
    1.3e-5 / 3.9e-5 | 1.5e-5 / 3.8e-5 (unclipped 9.2e-6 / 6.8e-5 | 1.3e-5 / 9.6e-5), ortho 9.2e-6 / 6.1e-5 | 8.1e-6 / 6.0e-5
    (unclipped 9.3e-6 / 6.0e-5 | 8.2e-6 / 6.0e-5), interior_near0 5.3e-6 / 5.5e-5 | 7.3e-6 / 8.1e-5 (unclipped 4.9e-6 / 6.1e-5 |
    3.5e-6 / 6.2e-5); a_orbit_sr1 random_near2 1.0e-5 / 1.3e-4 | 1.1e-5 / 1.4e-4, random_near3 2.0e-5 / 1.4e-4 | 2.4e-5 / 1.4e-4,
    interior_near0_jitter 7.9e-6 / 5.4e-5 | 8.7e-6 / 9.7e-5.
    (With the float32 normal bundle_ray_grad_kernel had before shade_for_ray_adjoint: 2.6e-5 .. 3.5e-4, e.g. random_near2
    3.5e-4 / 1.3e-4 and b_sr2_ert one_zero 2.2e-4 / 9.6e-5, all inside the rule.)"""
    inp, ref, ref32 = _state(scene, bundle)
    ray, mask, fwd = _ray_gradients(inp, ref, ref32, (scene, bundle))
    if bundle in ("axial", "one_zero"):   # before any comparison: 1 / 0 in the slab test and in the tail's ivmin, ivmax
        d_o, d_d = _raw_ray_gradients(inp, fwd)
        live = ref["n"].reshape(-1) > 1
        assert np.isfinite(d_o).all() and np.isfinite(d_d).all()
        # no live ray's six floats are all zero: finite_or_zero did not swallow a NaN
        assert (np.concatenate([d_o, d_d], 1)[live] != 0).any(1).all(), (scene, bundle)
        if bundle == "axial":
            # the exit-face term: d_origin along the axis of travel, wherever the reference's is non-zero. (Non-zero beyond
            # float64 rounding, 1e-9 of the scale: the samples do not move with the origin along the ray, only the light at
            # origin + e_y does, and for the rays along +-y it stays on the ray's line -- their reference is 1e-16, an exact 0.)
            axis, i = np.abs(inp["dirs"]).argmax(1), np.arange(len(d_o))
            want = ref["dray"].reshape(-1, 6)[i, axis]
            there = np.abs(want) > 1e-9 * np.abs(ref["dray"][..., :3]).max()
            assert there.sum() >= 48 and not there[axis == 1].any() and (d_o[i, axis][there] != 0).all()
    ray_rule(ray, ref, ref32, mask, (scene, bundle))
    if scene == "c_clip":
        # max_samples raised to the largest n: the unclipped reference is reproduced, and it is another gradient
        free = dict(inp, max_samples=int(ref["n"].max()))
        fref, fref32 = _free_refs(bundle, free["max_samples"])
        fray, fmask, ffwd = _ray_gradients(free, fref, fref32, (scene, bundle, "unclipped"))
        assert int(ffwd[8].max()) > 23
        ray_rule(fray, fref, fref32, fmask, (scene, bundle, "unclipped"))
        both = mask & fmask
        assert np.abs(fray - ray)[both].max() > 1e-2 * np.abs(fref["dray"][both]).max()


@functools.lru_cache(maxsize=None)
def _free_refs(bundle, S):
    return BR.refs(dict(BR.inputs("c_clip", bundle), max_samples=S))


# ---- 4. single-sample rays among live ones -------------------------------------------------------------------------------------------------

def test_single_sample_rays_get_zero_ray_gradients_and_leave_their_wave_alone(hiplib):
    """What the forward writes for an n == 1 ray, read from sample_pos and Composite: f = 0 / 0 is NaN and so is the position;
    tri_cell's fmaxf(0, NaN) is 0, so the intensity tap and the six normal taps all read voxel (0, 0, 0) with zero fractions, the
    normal is flat (L = 0.4, the ambient term) and the one sample is composited: the pixel is 0.4 op(tf(vol[0,0,0])) (rgb, 1 / 0.4),
    the same finite pixel for every such ray, steps 1. (The reference marches no such ray, H6: its pixel is 0.) The volume / TF
    backward scatters that sample's adjoint to voxel (0, 0, 0) and its texels, finite; bundle_ray_grad_kernel skips the ray."""
    F = _F()
    inp = BR.inputs("a_orbit_sr1", "single_sample")
    ref = BR.run(inp, grads=False)
    one = BR.SINGLE
    assert (ref["n"][one] == 1).all() and (ref["n"][~one] > 1).all()
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    assert (n.cpu().numpy() == ref["n"][:, 0]).all()
    g = dev(inp["grad_out"])   # non-zero on the single-sample rays too
    d_vol, d_tf = F.march_bundle_bwd(vol, tf, o, d, e, x, n, S, sr, g, out)
    d_o, d_d = F.march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    for t in (out, d_vol, d_tf, d_o, d_d):
        assert bool(torch.isfinite(t).all())
    t1, rest = torch.from_numpy(one).cuda(), torch.from_numpy(~one).cuda()
    assert bool((steps[t1] == 1).all()) and bool((steps[rest] > 1).all())
    assert bool((bits(out[t1]) == bits(out[t1][:1])).all()) and float(out[t1][0, 3]) > 0
    assert bool((d_o[t1] == 0).all()) and bool((d_d[t1] == 0).all())
    assert float(d_o[rest].abs().max()) > 0 and float(d_d[rest].abs().max()) > 0
    # the n > 1 rays alone (no jitter: nothing depends on a ray's index)
    alone = dict(inp, origins=inp["origins"][~one], dirs=inp["dirs"][~one], grad_out=inp["grad_out"][~one])
    vol2, tf2, o2, d2, e2, x2, n2, out2, steps2 = _forward(alone)
    d_o2, d_d2 = F.march_bundle_bwd_rays(vol2, tf2, o2, d2, e2, x2, n2, steps2, S, sr, dev(alone["grad_out"]), out2, **_opts(alone))
    assert torch.equal(bits(out[rest]), bits(out2)) and torch.equal(steps[rest], steps2)
    assert torch.equal(bits(d_o[rest]), bits(d_o2)) and torch.equal(bits(d_d[rest]), bits(d_d2))


# ---- 5. the partial backwards, in the three table tiers -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _smooth_tier_state(R):
    inp = BR.smooth_tier_inputs(R)
    return (inp,) + BR.refs(inp)


PARTIAL = {"R8": lambda: _state("a_orbit_sr1", "random"), "R3393": lambda: _smooth_tier_state(3393),
           "R10177": lambda: _smooth_tier_state(10177)}


@pytest.mark.parametrize("case", sorted(PARTIAL))
def test_partial_backwards_match_the_f64_reference(hiplib, monkeypatch, case):
    """want_vol=False and want_tf=False where d_tf is summed in LDS (R = 8), by global atomics beside a table in LDS (3393) and
    with the table in global memory (10177). Float atomics reorder: each result is held to the reference, not to the full
    call's bits.
    Measured on the MI355X, err / err32 / scale: R = 8 d_tf 2.3e-4 / 5.4e-4 / 252, d_vol 3.0e-4 / 1.6e-3 / 5.0; R = 3393 d_tf
    1.1e-3 / 1.0e-3 / 3.3, d_vol 2.5e-4 / 2.8e-1 / 3.2 (the float32 transliteration puts one sample in the neighbouring texel:
    its own d_vol is 9 % off, and the bound is that wide there); R = 10177 d_tf 2.5e-3 / 2.6e-3 / 2.5, d_vol 1.2e-4 / 1.5e-3 /
    3.1."""
    F = _F()
    inp, ref, ref32 = PARTIAL[case]()
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    mask = BR.keep(ref, ref32) & (ref["n"] > 1)
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * mask[..., None]).reshape(-1, 4)
    r, r32 = _masked_refs(inp, ref, ref32, mask)
    args = (vol, tf, o, d, e, x, n, int(inp["max_samples"]), float(inp["sr"]), g, out)
    none, d_tf = F.march_bundle_bwd(*args, want_vol=False)
    assert none is None
    LG.bound(C(d_tf), r["dtf"], r32["dtf"], f"{case} tf alone dtf")
    d_vol, none = F.march_bundle_bwd(*args, want_tf=False)
    assert none is None and d_vol.shape == vol.shape
    LG.bound(C(d_vol), r["dvol"], r32["dvol"], f"{case} vol alone dvol")

    def no_launch(*a, **k):
        raise AssertionError("a launch with nothing wanted")

    monkeypatch.setattr(F, "_call", no_launch)
    assert F.march_bundle_bwd(*args, want_vol=False, want_tf=False) == (None, None)


# ---- 6. the ray gradients at the table tiers ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", BR.TIER_EDGE_R)
def test_ray_gradients_and_d_vol_at_the_table_tiers_match_the_f64_reference(hiplib, R):
    """bundle_ray_grad_kernel with the table in LDS (R <= 10176) and in global memory (10177), on a table as smooth as the
    scene's (bundle_reference.smooth_tier_inputs), where d_vol is conditioned too.
    Measured on the MI355X, ray gradients as err / err32 over the scale, d_origin | d_dir: R = 3393 5.7e-6 / 5.9e-5 | 1.7e-5 /
    9.7e-5 (59 rays), 10176 5.4e-5 / 9.0e-5 | 6.1e-5 / 7.4e-5 (64), 10177 1.2e-5 / 1.9e-5 | 9.4e-6 / 1.7e-5 (62). d_vol as err /
    err32 / scale: 2.5e-4 / 2.8e-1 / 3.2, 1.6e-4 / 2.4e-4 / 2.5, 1.2e-4 / 1.5e-3 / 3.1; d_tf 1.1e-3 / 1.0e-3 / 3.3, 3.3e-3 /
    2.8e-3 / 2.6, 2.5e-3 / 2.6e-3 / 2.5."""
    inp, ref, ref32 = _smooth_tier_state(R)
    _parity(inp, ref, ref32, ("smooth R", R), dvol=True)
    ray, mask, _ = _ray_gradients(inp, ref, ref32, ("smooth R", R))
    ray_rule(ray, ref, ref32, mask, ("smooth R", R))


# ---- 7. an f16 volume, a strided volume: the ray gradients --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _f16_state():
    base = BR.inputs("a_orbit_sr1", "random")
    inp = dict(base, vol=PG.F16(base["vol"]))
    assert not np.array_equal(inp["vol"], base["vol"])
    return (inp,) + BR.refs(inp)


def test_ray_gradients_of_an_f16_volume_match_the_f64_reference_on_the_volume_the_kernel_reads(hiplib):
    """Measured on the MI355X, err / err32 over the scale: d_origin 1.7e-5 / 9.75e-5, d_dir 8.8e-6 / 9.6e-5 (185 rays).
    This case is why bundle_ray_grad_kernel shades a sample for the adjoint with a normal from double taps around the sample's
    position in double (march_bundle.hip, shade_for_ray_adjoint). With its float32 normal d_origin was 4.258e-3 off against
    3 err32 + 1e-4 scale = 4.241e-3 (err / scale 3.94e-4), bit for bit the same with the same values held as a float32 volume
    (bundle_ray_grad_kernel<__half> was not the cause). All of it was ray 1's, six components 6.4e-4 too large alike, where
    the float32 transliteration is 7e-6 off. In float64, dL/dpos of its sample 7 is -6.646 of the ray's d_origin.y = -6.625:
    that sample sits 0.0027 voxels above a cell boundary in y, so its y taps (+-0.0075 voxels) straddle the boundary, and it
    has the smallest |grad| of the ray, 1.46e-4; the float64 gradient moves by 1.3e-4 of its size for 1e-8 on a direction
    component (an ordinary ray: 1e-7 .. 1e-6). Double taps around the float32 position gave 1.12e-4 here and broke c_clip x
    ortho (4.74e-4 / 6.06e-5, from 4.56e-5: ray 33, sample 17, z taps across a boundary at |grad| 2.4e-4), where the 1e-7 of a
    float32 position decides; with the position in double as well both are at 1e-5."""
    inp, ref, ref32 = _f16_state()
    vol = dev(inp["vol"]).half()
    assert vol.dtype == torch.float16 and np.array_equal(C(vol), inp["vol"])
    ray, mask, _ = _ray_gradients(inp, ref, ref32, "f16", vol=vol)
    ray_rule(ray, ref, ref32, mask, "f16")


def test_ray_gradients_of_a_permuted_volume_match_the_f64_reference(hiplib):
    """Measured on the MI355X, err / err32 over the scale: d_origin 1.9e-5 / 7.6e-5, d_dir 1.0e-5 / 7.5e-5 (186 rays)."""
    inp, ref, ref32 = _state("a_orbit_sr1", "random")
    vol = dev(np.ascontiguousarray(inp["vol"].transpose(2, 0, 1))).permute(1, 2, 0)
    assert not vol.is_contiguous() and vol.stride(0) != 1 and np.array_equal(C(vol), inp["vol"])
    ray, mask, _ = _ray_gradients(inp, ref, ref32, "permuted", vol=vol)
    ray_rule(ray, ref, ref32, mask, "permuted")


# ---- 8. the module on a cone beam ------------------------------------------------------------------------------------------------------------

def test_module_on_a_cone_beam_gives_the_source_and_table_gradients(hiplib, monkeypatch):
    """RayBundleRaycaster(ray_grad=True, jitter=False) on cone_beam_rays handed over as (H, W, 3), the directions scaled by a
    per-ray factor in [0.5, 2] (the gradient passes through the module's normalisation), one detector column with an x
    component of exactly 0; the source and the table require grad, the volume does not. source.grad and tf.grad of sum(out g)
    against float64 autograd through cone_beam_rays, the scaling and bundle_reference.run's program (cone_gradient).
    Measured on the MI355X: all 120 rays kept; image err 3.0e-6 (err32 2.9e-6); d_source err 1.2e-4, err32 1.3e-3, scale 2.0;
    d_tf err 2.0e-4, err32 2.3e-4, scale 96."""
    from differender_amd import functional as Fn
    from differender_amd.bundle import RayBundleRaycaster, cone_beam_rays
    cone = BR.CONE
    H, W = cone["det"]
    inp = BR.cone_inputs()
    ref, ref32 = BR.cone_gradient(inp, grads=False), BR.cone_gradient(inp, torch.float32, grads=False)
    S, sr, R = int(inp["max_samples"]), float(inp["sr"]), inp["tf"].shape[0]
    field = dev(inp["vol"])
    vol = field.permute(1, 2, 0)[None]   # (1, D, H, W) of the field (W, D, H)
    tf = dev(inp["tf"]).t().contiguous().requires_grad_(True)
    source = dev(np.array(cone["source"])).requires_grad_(True)
    o, d = cone_beam_rays(source, cone["det_center"], cone["det_u"], cone["det_v"], cone["det"])
    d = d * dev(BR.cone_scale())
    assert o.shape == d.shape == (H, W, 3) and bool((d[:, BR.CONE_ZERO_COLUMN, 0] == 0).all()) and int((d == 0).sum()) == H
    assert float(((d * d).sum(-1).sqrt() - 1).abs().min().detach()) > 1e-4
    calls = []
    bwd = Fn.march_bundle_bwd

    def spy(*a, **k):
        res = bwd(*a, **k)
        calls.append((k["want_vol"], k["want_tf"], res[0]))
        return res

    monkeypatch.setattr(Fn, "march_bundle_bwd", spy)
    rc = RayBundleRaycaster(vol.shape[-3:], R, sampling_rate=sr, jitter=False, max_samples=S, ray_grad=True)
    out = rc(vol, tf, o, d)
    assert out.shape == (H, W, 4) and rc._steps.shape == (H, W)
    # n as the module's kernels saw it: its own statements on the same rays
    dk = (d / torch.sqrt((d * d).sum(-1, keepdim=True))).detach().reshape(-1, 3)
    n = Fn.bundle_setup(o.detach().reshape(-1, 3), dk, field.shape, sr)[2]
    live = ref["n"] > 1
    mask = (BR.keep(ref, ref32) & live & (n.cpu().numpy().reshape(-1, 1) == ref["n"]) &
            (rc._steps.cpu().numpy().reshape(-1, 1) == ref["steps"]))
    assert live.sum() > 0.8 * H * W and mask.sum() >= 0.8 * live.sum(), (mask.sum(), live.sum())
    m4 = mask[..., None]
    LG.bound(C(out).reshape(-1, 1, 4) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "cone rgba")
    want, want32 = (BR.cone_gradient(inp, dt, pixels=mask.reshape(-1)) for dt in (torch.float64, torch.float32))
    (out.reshape(-1, 4) * dev(inp["grad_out"] * mask)).sum().backward()
    assert calls == [(False, True, None)] and vol.grad is None   # the volume wanted no gradient and got none
    assert np.abs(want["d_source"]).min() > 0
    PB.d8_check(C(source.grad), want["d_source"], want32["d_source"], "cone d_source")
    LG.bound(C(tf.grad).T, want["dtf"], want32["dtf"], "cone dtf")
