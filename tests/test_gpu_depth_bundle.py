"""The depth march over ray bundles on the GPU: a pinhole camera's rays give march_depth_fwd's moments and steps
bit for bit, and any bundle's A and steps are march_bundle_fwd's; the launch tail; the moments, d_vol, d_tf and the per-ray
d_origin / d_dir against the float64 autograd reference of tests/depth_bundle_reference.py (light_gpu.bound for the former,
test_gpu_bundle.ray_rule over the well-conditioned rays for the latter -- no other tolerance); air; the table tiers; rates and
caps; volume layouts; single-sample rays; D5; the module beside DepthRaycaster; the example."""
import math
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
import depth_bundle_reference as DB  # noqa: E402
import depth_gpu as DG  # noqa: E402
import depth_reference as DR  # noqa: E402
import light_gpu as LG  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402
import pose_gpu as PG  # noqa: E402
from test_gpu_bundle import ray_rule  # noqa: E402

pytestmark = pytest.mark.gpu

C = LG.C
dev = PG.dev
bits = lambda t: t.contiguous().view(torch.int32)
PREFILL = 0.25   # what d_tf holds before a backward: the colour columns must come back as they were


def _F():
    from differender_amd import functional as F
    return F


def _opts(inp):
    return dict(t_near=inp.get("t_near"), jitter_seed=int(inp["jitter_seed"]), ray_base=int(inp["ray_base"]))


def _forward(inp, vol=None):
    """bundle_setup + march_depth_bundle_fwd of inp on the device (vol: the device volume in the place of inp's) ->
    (vol, tf, o, d, e, x, n, out, steps)."""
    F = _F()
    vol = dev(inp["vol"]) if vol is None else vol
    tf, o, d = dev(inp["tf"]), dev(inp["origins"]), dev(inp["dirs"])
    e, x, n = F.bundle_setup(o, d, vol.shape, float(inp["sr"]), **_opts(inp))
    out, steps = F.march_depth_bundle_fwd(vol, tf, o, d, e, x, n, int(inp["max_samples"]), float(inp["sr"]))
    return vol, tf, o, d, e, x, n, out, steps


def _raw_bwd(vol, tf, o, d, e, x, n, S, sr, g, out, d_vol=None):
    """dr_march_depth_bundle_bwd on the caller's d_vol (default: a zeroed one of the volume's layout) and a d_tf pre-filled with
    PREFILL -> (d_vol, the alpha column's gradient as float64 numpy). The colour columns come back bit for bit."""
    F, N = _F(), LG.native()
    head = F._bundle_head(vol, tf, o, d, e, x, n, S, sr)[3]
    d_vol = torch.zeros(vol.shape, dtype=torch.float32, device="cuda") if d_vol is None else d_vol
    d_tf = torch.full(tf.shape, PREFILL, dtype=torch.float32, device="cuda")
    g, out = g.contiguous(), out.contiguous()
    rc = N.lib().dr_march_depth_bundle_bwd(*head, g.data_ptr(), out.data_ptr(), d_vol.data_ptr(), *d_vol.stride(), d_tf.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((d_tf[:, :3] == PREFILL).all()), "a colour column of d_tf was written"
    return d_vol, C(d_tf)[:, 3] - PREFILL


def _masked_refs(inp, ref, ref32, mask):
    """The references' d_vol and d_tf for the upstream gradient of the rays in `mask` alone: the full runs' when that is every
    n > 1 ray of both, else two more runs over those rays."""
    if (mask == (ref["n"] > 1)).all() and (mask == (ref32["n"] > 1)).all():
        return ref, ref32
    return DB.run(inp, pixels=mask.reshape(-1)), DB.run(inp, torch.float32, pixels=mask.reshape(-1))


def _parity(inp, ref, ref32, what, vol=None, dvol=True, d_vol_buf=None, tf_sum=False):
    """n equals the float32 transliteration's on the kept rays (bundle_reference.keep's rule), and steps on those that are marched
    (the references march no single-sample ray, H6); the moments, d_vol and d_tf's alpha column are within light_gpu.bound of
    float64, the upstream gradient zero off the kept n > 1 rays. dvol=False: d_vol is only finite (the caller holds it).
    tf_sum: the sum of d_tf's alpha column by the same bar. -> the forward's tuple, mask, d_vol."""
    vol, tf, o, d, e, x, n, out, steps = _forward(inp, vol)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    keep = BR.keep(ref, ref32)
    live = keep & (ref["n"] > 1)
    n_k, steps_k = n.cpu().numpy().reshape(-1, 1), steps.cpu().numpy().reshape(-1, 1)
    assert (n_k[keep] == ref32["n"][keep]).all() and (steps_k[live] == ref32["steps"][live]).all(), what
    miss = ref["n"] <= 1
    assert (steps_k[miss] == 0).all() and (C(out).reshape(-1, 1, 4)[miss] == 0).all(), what
    assert bool((out[:, 2] == 0).all())
    mask = live
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    m4 = mask[..., None]
    LG.bound(C(out).reshape(-1, 1, 4) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, f"{what} moments")
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * m4).reshape(-1, 4)
    r, r32 = _masked_refs(inp, ref, ref32, mask)
    d_vol, d_alpha = _raw_bwd(vol, tf, o, d, e, x, n, S, sr, g, out, d_vol_buf)
    assert (r["dtf"][:, :3] == 0).all()
    if dvol:
        LG.bound(C(d_vol), r["dvol"], r32["dvol"], f"{what} dvol")
    else:
        assert bool(torch.isfinite(d_vol).all())
    LG.bound(d_alpha, r["dtf"][:, 3], r32["dtf"][:, 3], f"{what} dtf alpha")
    if tf_sum:
        LG.bound(np.array([d_alpha.sum()]), np.array([r["dtf"][:, 3].sum()]), np.array([r32["dtf"][:, 3].sum()]), f"{what} dtf alpha sum")
    return (vol, tf, o, d, e, x, n, out, steps), mask, d_vol


def _ray_gradients(inp, ref, ref32, what, fw=None):
    """march_depth_bundle_bwd_rays with the upstream gradient of the well-conditioned rays whose march stops where the
    reference's does -> (ray (P,1,6), mask)."""
    F = _F()
    vol, tf, o, d, e, x, n, out, steps = _forward(inp) if fw is None else fw
    good = K.well_conditioned(ref, ref32, BR.keep(ref, ref32), "dray", BR.COLUMNS, what, lit=False)
    agree = (steps.cpu().numpy().reshape(-1, 1) == ref["steps"]) & (n.cpu().numpy().reshape(-1, 1) == ref["n"])
    mask = good & agree
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * mask[..., None]).reshape(-1, 4)
    d_o, d_d = F.march_depth_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]), g, out,
                                             **_opts(inp))
    return np.concatenate([C(d_o), C(d_d)], -1).reshape(-1, 1, 6), mask


# ---- 1. a pinhole camera's rays: march_depth_fwd's moments and steps, bit for bit --------------------------------------------------

D_JITTER_SEED = CG.CASES["d_jitter"][7]


@pytest.mark.parametrize("seed", [0, D_JITTER_SEED], ids=["no_jitter", "jitter"])
@pytest.mark.parametrize("name", ["a_orbit_sr1", "j_inside"])
def test_a_pinhole_cameras_rays_give_march_depth_fwds_moments_and_steps_bit_for_bit(hiplib, name, seed):
    F = _F()
    inp = CG.make_inputs(name)
    W, H = inp["grad_out"].shape[:2]
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    vol, tf, cam = dev(inp["vol"]), dev(inp["tf"]), dev(inp["cam"][None])
    e0, x0, r0, n0 = F.ray_setup(cam, (W, H), vol.shape, sr, jitter_seed=seed, view_base=CG.VIEW)
    o, d = cam.expand(W * H, 3).contiguous(), r0.reshape(W * H, 3)
    e, x, n = F.bundle_setup(o, d, vol.shape, sr, None, seed, ray_base=CG.VIEW)
    assert torch.equal(bits(e), bits(e0.reshape(-1))) and torch.equal(n, n0.reshape(-1)) and int((n > 1).sum()) > 50
    out0, steps0 = F.march_depth_fwd(vol, tf, cam, e0, x0, r0, n0, S, sr)
    out, steps = F.march_depth_bundle_fwd(vol, tf, o, d, e, x, n, S, sr)
    assert torch.equal(bits(out), bits(out0.reshape(-1, 4))) and torch.equal(steps, steps0.reshape(-1))
    assert float(out[:, 0].abs().max()) > 0
    if name == "j_inside":
        assert float(out[:, 0].min()) < 0   # the camera is inside the box: negative distances behind it


# ---- 2. A and steps are the colour bundle march's ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bundle", ["random", "interior_near0", "random_jitter"])
def test_alpha_and_steps_are_march_bundle_fwds_bits(hiplib, bundle):
    F = _F()
    inp = DB.inputs("a_orbit_sr1", bundle)
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    colour, csteps = F.march_bundle_fwd(vol, tf, o, d, e, x, n, int(inp["max_samples"]), float(inp["sr"]))
    many = n != 1   # (a single-sample ray is where the two differ by definition, H6: the colour march samples it at 0 / 0)
    assert int((n > 1).sum()) > 100 and float(out[:, 3].max()) > 0
    assert torch.equal(bits(out[:, 3][many]), bits(colour[:, 3][many])) and torch.equal(steps[many], csteps[many])


# ---- 3. the launch tail -------------------------------------------------------------------------------------------------------------

TAIL = (1, 63, 64, 65, 255, 256, 257)
CANARY = 12345.0


def _tail_run(inp, g_all, count, vol, tf, S, sr):
    """The first `count` rays through the three entries on buffers 8 rays longer, pre-filled with CANARY."""
    F, N = _F(), LG.native()
    o, d = dev(inp["origins"][:count]), dev(inp["dirs"][:count])
    pad = count + 8
    fbuf = lambda *k: torch.full((pad, *k), CANARY, device="cuda")
    e, x, n = F.bundle_setup(o, d, vol.shape, sr)
    stream = torch.cuda.current_stream().cuda_stream
    head = F._bundle_head(vol, tf, o, d, e, x, n, S, sr)[3]
    out, steps = fbuf(4), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    assert N.lib().dr_march_depth_bundle_fwd(*head, out.data_ptr(), steps.data_ptr(), stream) == 0
    g = g_all[:count].contiguous()
    d_o, d_d = fbuf(3), fbuf(3)
    assert N.lib().dr_march_depth_bundle_bwd_rays(*head, steps.data_ptr(), -math.inf, 0, 0, g.data_ptr(), out.data_ptr(),
                                                  d_o.data_ptr(), d_d.data_ptr(), stream) == 0
    d_vol, d_alpha = _raw_bwd(vol, tf, o, d, e, x, n, S, sr, g, out[:count])
    return dict(n=n, out=out, steps=steps, d_o=d_o, d_d=d_d), d_vol, d_alpha


def test_the_launch_tail_writes_its_own_rays_and_nothing_else(hiplib):
    """out, steps, d_origins and d_dirs past N are untouched and the first N are the full bundle's bits; d_vol and d_tf are
    those of the first N rays: the float64 reference over those rays alone, by light_gpu.bound. (The upstream gradient is zero
    off bundle_reference.keep's rays, as everywhere.)"""
    inp = BR.inputs("a_orbit_sr1", "random", rays=BR.random_bundle(max(TAIL)))
    inp = dict(inp, jitter_seed=0)
    ref, ref32 = DB.refs(inp)
    vol, tf, S, sr = dev(inp["vol"]), dev(inp["tf"]), int(inp["max_samples"]), float(inp["sr"])
    steps = _forward(inp)[8].cpu().numpy().reshape(-1, 1)
    mask = BR.keep(ref, ref32) & (ref["n"] > 1) & (steps == ref["steps"])
    assert mask.sum() > 0.8 * max(TAIL) and mask[0, 0]
    g_all = dev(inp["grad_out"] * mask)
    full, _, _ = _tail_run(inp, g_all, max(TAIL), vol, tf, S, sr)
    assert int((full["n"] > 1).sum()) == max(TAIL)
    assert float(full["d_o"][:max(TAIL)].abs().max()) > 0 and float(full["d_d"][:max(TAIL)].abs().max()) > 0
    for count in TAIL:
        got, d_vol, d_alpha = _tail_run(inp, g_all, count, vol, tf, S, sr)
        for k, t in got.items():
            assert torch.equal(bits(t[:count]), bits(full[k][:count])), (count, k)
            if k != "n":
                canary = t[count:]
                assert bool((canary == (77 if t.dtype == torch.int32 else CANARY)).all()), (count, k)
        first = mask.reshape(-1) & (np.arange(max(TAIL)) < count)
        r, r32 = DB.run(inp, pixels=first), DB.run(inp, torch.float32, pixels=first)
        LG.bound(C(d_vol), r["dvol"], r32["dvol"], f"tail {count} dvol")
        LG.bound(d_alpha, r["dtf"][:, 3], r32["dtf"][:, 3], f"tail {count} dtf alpha")


# ---- 4. / 5. moments, d_vol, d_tf and the ray gradients off the pinhole ------------------------------------------------------------------

@pytest.mark.parametrize("scene,bundle", DB.GRAD_CASES, ids=lambda v: str(v))
def test_moments_d_vol_and_d_tf_match_the_f64_reference(hiplib, scene, bundle):
    """Measured on the MI355X over these cases: d_vol at most 0.22 of its bar (b_sr2_ert x random), d_tf's alpha column at
    most 0.53 (b_sr2_ert x one_zero), the moments at most 0.15; DESIGN.md D22 has the figures."""
    inp, ref, ref32 = DB.state(scene, bundle)
    _parity(inp, ref, ref32, (scene, bundle))


@pytest.mark.parametrize("scene,bundle", DB.GRAD_CASES, ids=lambda v: str(v))
def test_ray_gradients_match_the_f64_reference_on_the_well_conditioned_rays(hiplib, scene, bundle):
    inp, ref, ref32 = DB.state(scene, bundle)
    ray, mask = _ray_gradients(inp, ref, ref32, (scene, bundle))
    ray_rule(ray, ref, ref32, mask, (scene, bundle))


# ---- 6. an object in air: the frozen 0 < x_tf switch at values of exactly 0 ------------------------------------------------------------

@pytest.mark.parametrize("scene,bundle", DB.AIR_CASES, ids=lambda v: str(v))
def test_an_object_in_air(hiplib, scene, bundle):
    """The moments, d_tf and the ray gradients as everywhere. d_vol: the float32 program's own is 1.2 of a scale of 8.5 (ortho)
    off float64 -- a sample whose intensity is exactly 0 passes no gradient, and whether a sample next to the object reads 0 is
    decided within rounding -- so the bar would accept anything. Instead d_vol is finite, and exactly 0 on every voxel a sample's
    cell touches whose 27-neighbourhood is air."""
    inp, ref, ref32 = DB.state(scene, bundle)
    fw, mask, d_vol = _parity(inp, ref, ref32, (scene, bundle), dvol=False)
    ray, rmask = _ray_gradients(inp, ref, ref32, (scene, bundle), fw)
    ray_rule(ray, ref, ref32, rmask, (scene, bundle))
    P = inp["origins"].shape[0]
    I, live, cell = DG.sample_values(inp["vol"], inp["origins"], ref["entry"].reshape(P), ref["exit"].reshape(P), inp["dirs"],
                                     ref["n"].reshape(P), ref["steps"].reshape(P))
    air = DG.deep_air(inp["vol"], cell, live)
    assert air.sum() > 100 and float(d_vol.abs().max()) > 0
    assert (C(d_vol)[air] == 0).all()


# ---- 7. the table tiers ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", DB.TIER_R)
def test_table_tiers_match_the_f64_reference(hiplib, R):
    """R = 3392: the last table with its [R] doubles beside it in LDS; 3393: the table in LDS, d_tf by global atomics; 10176: the
    last table in LDS; 10177: read where it lies. The sum of d_tf's alpha column does not depend on which side of a texel
    boundary a sample falls: it catches a tier that loses or doubles adds."""
    inp, ref, ref32 = DB.tier_state(R)
    assert inp["tf"].shape[0] == R
    _parity(inp, ref, ref32, ("R", R), tf_sum=True)
    ray, mask = _ray_gradients(inp, ref, ref32, ("R", R))
    ray_rule(ray, ref, ref32, mask, ("R", R))


# ---- 8. rates and caps ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,bundle,over", DB.RATE_CASES, ids=lambda v: str(v))
def test_rates_and_caps(hiplib, scene, bundle, over):
    inp, ref, ref32 = DB.state(scene, bundle, tuple(sorted(over.items())))
    fw, _, _ = _parity(inp, ref, ref32, (scene, bundle, over))
    ray, mask = _ray_gradients(inp, ref, ref32, (scene, bundle, over), fw)
    ray_rule(ray, ref, ref32, mask, (scene, bundle, over))


# ---- 9. volume layouts ------------------------------------------------------------------------------------------------------------------

def test_an_f16_volume_matches_the_f64_reference_on_the_volume_the_kernel_reads(hiplib):
    base = DB.inputs("a_orbit_sr1", "random")
    inp = dict(base, vol=PG.F16(base["vol"]))
    vol = dev(inp["vol"]).half()
    assert np.array_equal(C(vol), inp["vol"]) and not np.array_equal(inp["vol"], base["vol"])
    ref, ref32 = DB.refs(inp)
    fw, _, _ = _parity(inp, ref, ref32, "f16", vol=vol)
    ray, mask = _ray_gradients(inp, ref, ref32, "f16", fw)
    ray_rule(ray, ref, ref32, mask, "f16")


@pytest.mark.parametrize("layout", ["permuted", "sliced", "d_vol_strided"])
def test_volume_layouts_match_the_f64_reference(hiplib, layout):
    """A permuted volume (no unit stride first), a slice of a larger tensor (an offset and strides of the parent), and a d_vol
    buffer whose strides are not the volume's: the values the kernel reads are the reference's."""
    inp, ref, ref32 = DB.state("a_orbit_sr1", "random")
    VX, VY, VZ = inp["vol"].shape
    vol, d_vol_buf = None, None
    if layout == "permuted":
        vol = dev(np.ascontiguousarray(inp["vol"].transpose(2, 0, 1))).permute(1, 2, 0)
        assert not vol.is_contiguous() and vol.stride(0) != 1
    elif layout == "sliced":
        big = torch.full((VX + 3, VY + 2, VZ + 5), 7.0, device="cuda")
        big[2:2 + VX, 1:1 + VY, 3:3 + VZ] = dev(inp["vol"])
        vol = big[2:2 + VX, 1:1 + VY, 3:3 + VZ]
        assert not vol.is_contiguous() and vol.storage_offset() > 0
    else:
        big = torch.zeros((VZ + 1, VX + 2, VY + 3), device="cuda")
        d_vol_buf = big.permute(1, 2, 0)[1:1 + VX, 2:2 + VY, :VZ]
        assert d_vol_buf.shape == (VX, VY, VZ) and d_vol_buf.stride() != dev(inp["vol"]).stride()
    if vol is not None:
        assert np.array_equal(C(vol), inp["vol"])
    fw, _, d_vol = _parity(inp, ref, ref32, layout, vol=vol, d_vol_buf=d_vol_buf)
    if layout == "d_vol_strided":   # nothing outside the view was written
        outside = big.clone()
        outside.permute(1, 2, 0)[1:1 + VX, 2:2 + VY, :VZ] = 0
        assert bool((outside == 0).all()) and float(d_vol.abs().max()) > 0
    else:
        plain = _forward(inp)
        assert torch.equal(bits(fw[7]), bits(plain[7])) and torch.equal(fw[8], plain[8])   # same values, same arithmetic
        ray, mask = _ray_gradients(inp, ref, ref32, layout, fw)
        ray_rule(ray, ref, ref32, mask, layout)


# ---- 10. single-sample rays ---------------------------------------------------------------------------------------------------------------

def test_single_sample_rays_contribute_nothing_and_leave_their_wave_alone(hiplib):
    """Eight lanes of one wave have n == 1 (H6): moments 0, steps 0, exact zeros in all six ray-gradient components; the other
    56 lanes are held to the reference."""
    F = _F()
    inp, ref, ref32 = DB.state(*DB.SINGLE_CASE)
    one = BR.SINGLE
    (vol, tf, o, d, e, x, n, out, steps), mask, _ = _parity(inp, ref, ref32, "single")
    assert bool((n.cpu()[one] == 1).all()) and bool((n.cpu()[~one] > 1).all()) and not mask[one].any()
    assert bool((out.cpu()[one] == 0).all()) and bool((steps.cpu()[one] == 0).all())
    g = dev(inp["grad_out"])   # (an upstream gradient on the single-sample rays too)
    d_o, d_d = F.march_depth_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]), g, out,
                                             **_opts(inp))
    assert bool((bits(d_o.cpu()[one]) == 0).all()) and bool((bits(d_d.cpu()[one]) == 0).all())
    ray, rmask = _ray_gradients(inp, ref, ref32, "single", (vol, tf, o, d, e, x, n, out, steps))
    assert not rmask[one].any() and rmask[~one].sum() > 0.8 * (~one).sum()
    ray_rule(ray, ref, ref32, rmask, "single")


# ---- 11. non-finite upstream gradients (D5) --------------------------------------------------------------------------------------------------

def test_non_finite_upstream_rays_get_zeros_or_clamped_values_and_leave_the_others_alone(hiplib):
    from differender_amd.depth import RayBundleDepthRaycaster
    F = _F()
    inp, ref, _ = DB.state("a_orbit_sr1", "random")
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    bad = {7: float("nan"), 70: float("inf"), 133: float("-inf")}
    assert all(ref["n"][p, 0] > 1 for p in bad)
    g = dev(inp["grad_out"])
    clean = F.march_depth_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    g_bad = g.clone()
    for p, v in bad.items():
        g_bad[p, 1] = v
    got = F.march_depth_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, S, sr, g_bad, out, **_opts(inp))
    others = torch.ones(len(g), dtype=torch.bool, device="cuda")
    others[list(bad)] = False
    for a, b in zip(got, clean):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) <= 1e30
        assert bool((a[7] == 0).all()) and float(b[7].abs().max()) > 0          # NaN: zeros
        for p in (70, 133):   # +-inf: zeros (inf - inf is a NaN) or values clamped to +-1e30 -- finite, and not the clean ray's
            assert not torch.equal(bits(a[p]), bits(b[p]))
        assert torch.equal(bits(a[others]), bits(b[others]))
    # the plain backward propagates the NaN like the reference; the module's gradients end in nan_to_num
    d_vol, d_tf = F.march_depth_bundle_bwd(vol, tf, o, d, e, x, n, S, sr, g_bad, out)
    assert not bool(torch.isfinite(d_vol).all()) and not bool(torch.isfinite(d_tf).all())
    rc = RayBundleDepthRaycaster(vol.permute(1, 2, 0).shape, tf.shape[0], jitter=False, max_samples=S, ray_grad=True)
    v, t = vol.permute(1, 2, 0)[None].clone().requires_grad_(True), tf.t().clone().requires_grad_(True)
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    (rc(v, t, oo, dd) * g_bad[:, (0, 1, 3)]).sum().backward()
    for leaf in (v, t, oo, dd):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert bool((oo.grad[7] == 0).all()) and bool((dd.grad[7] == 0).all())


# ---- 12. the module, end to end ------------------------------------------------------------------------------------------------------------

POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
CAM = (-1.3, 0.9, 2.0)


def test_module_on_pinhole_rays_gives_depth_raycasters_moments_and_pose_gradients(hiplib):
    from differender_amd.bundle import pinhole_rays
    from differender_amd.depth import DepthRaycaster, RayBundleDepthRaycaster
    inp = PG.inputs("a_orbit_sr1", look_from=np.array(CAM), **POSE)
    ref, ref32 = DR.run_case(inp), DR.run_case(inp, dtype=torch.float32)
    W, H = ref["n"].shape
    S, R = int(inp["max_samples"]), inp["tf"].shape[0]
    vol = dev(inp["vol"]).permute(1, 2, 0)[None]   # (1, D, H, W) of the field (W, D, H)
    tf = dev(inp["tf"]).t()
    kernel_order = lambda img: torch.flip(img, (0,)).transpose(0, 1)   # (H, W, ...) user orientation -> (W, H, ...)
    leaves = lambda: [torch.tensor(np.asarray(a, np.float64), dtype=torch.float32, device="cuda").requires_grad_(True)
                      for a in (inp["look_from"], inp["look_at"], inp["up"], math.degrees(float(inp["fov_rad"])))]

    def ten(ls):   # the gradients as the reference's ten columns: fov per radian
        return np.concatenate([C(ls[0].grad), C(ls[1].grad), C(ls[2].grad), [float(ls[3].grad) * 180.0 / math.pi]])

    rb = RayBundleDepthRaycaster(vol.shape[-3:], R, jitter=False, max_samples=S, ray_grad=True)
    lb = leaves()
    vb, tb = vol.clone().requires_grad_(True), tf.clone().requires_grad_(True)
    m_b = rb(vb, tb, *pinhole_rays(*lb, (W, H)))
    assert m_b.shape == (H, W, 3) and rb._steps.shape == (H, W)
    steps_b = kernel_order(rb._steps).cpu().numpy()
    with torch.no_grad():   # the same rays as (N, 3): the same bits, _steps in the rays' leading shape
        o, d = pinhole_rays(*lb, (W, H))
        flat = rb(vol, tf, o.reshape(-1, 3), d.reshape(-1, 3))
        assert flat.shape == (H * W, 3) and rb._steps.shape == (H * W,)
        assert torch.equal(bits(flat), bits(m_b.detach().reshape(-1, 3)))
    rr = DepthRaycaster(vol.shape[-3:], (W, H), R, jitter=False, max_samples=S, camera_grad=True)
    lr = leaves()
    m_r = rr(vol, tf, lr[0], look_at=lr[1], up=lr[2], fov=lr[3])
    assert m_r.shape == (3, H, W)
    four = lambda m3: torch.stack([m3[..., 0], m3[..., 1], torch.zeros_like(m3[..., 0]), m3[..., 2]], -1)   # (M1, M2, 0, A)
    img_b, img_r = four(kernel_order(m_b)), four(m_r.permute(2, 1, 0).flip(1))
    steps_r = rr._steps.cpu().numpy().reshape(W, H)
    mask = PG.keep(ref, ref32) & (ref["n"] > 1) & (steps_b == ref["steps"]) & (steps_r == ref["steps"])
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    m4 = mask[..., None]
    LG.bound(C(img_b) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "bundle module moments")
    LG.bound(C(img_r) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "DepthRaycaster moments")
    g = dev(inp["grad_out"] * m4)   # (W, H, 4), zero off the mask
    (img_b * g).sum().backward()
    (img_r * g).sum().backward()
    PG.pose_total_rule(ten(lb), ref["dpose_ray"], ref32["dpose_ray"], mask, "bundle module")
    PG.pose_total_rule(ten(lr), ref["dpose_ray"], ref32["dpose_ray"], mask, "DepthRaycaster")
    for leaf in (vb, tb):   # the volume's and the table's gradients come along; the colour rows are exactly 0
        assert leaf.grad.shape == leaf.shape and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert bool((tb.grad[:3] == 0).all())


def test_a_module_without_ray_grad_refuses_rays_that_require_grad(hiplib):
    from differender_amd.depth import RayBundleDepthRaycaster, ray_expected_depth
    rc = RayBundleDepthRaycaster((8, 9, 10), 6, jitter=False, t_near=0.0)
    vol = torch.rand(1, 8, 9, 10, device="cuda").requires_grad_(True)
    tf = torch.rand(4, 6, device="cuda")
    o = torch.tensor([[0.1, 0.2, 3.0]] * 5, device="cuda")
    d = torch.tensor([[0.0, 0.0, -2.0]] * 5, device="cuda")   # (not unit vectors: the module normalises)
    with pytest.raises(ValueError, match="no gradient w.r.t. origins.*ray_grad=True"):
        rc(vol, tf, o.clone().requires_grad_(True), d)
    with pytest.raises(ValueError, match="no gradient w.r.t. directions.*ray_grad=True"):
        rc(vol, tf, o, d.clone().requires_grad_(True))
    m = rc(vol, tf, o, d)   # without them it renders, and the volume gets its gradient
    m.sum().backward()
    assert m.shape == (5, 3) and float(m.detach().abs().max()) > 0 and float(vol.grad.abs().max()) > 0
    rng = ray_expected_depth(m.detach())   # the box spans z in [-1, 1]: a range from z = 3 lies in [2, 4]
    assert rng.shape == (5,) and bool(((rng >= 2.0) & (rng <= 4.0)).all())


# ---- 13. the example ------------------------------------------------------------------------------------------------------------------------

def test_the_ray_batch_example_runs_and_its_loss_falls(hiplib, capsys):
    sys.path.insert(0, ROOT)
    from examples.depth_ray_batch_synthetic import main
    res = main(["--vol", "16", "--img", "16", "--views", "4", "--rays", "512", "--iterations", "30", "--quiet"])
    print("depth ray batch: loss", res["losses"][0], "->", res["losses"][-1], "volume mse", res["vol_mse"])
    assert np.isfinite(res["losses"]).all() and res["losses"][-1] < res["losses"][0]
    text = capsys.readouterr().out
    assert "loss " in text and "volume mse to vol_gt" in text
