"""The ray-bundle march on the GPU: a pinhole camera's rays give that camera's buffers, image and steps bit for
bit; the launch tail; the image, d_vol, d_tf and the per-ray d_origin / d_dir off the pinhole against the float64 autograd
reference of tests/bundle_reference.py, run at test time on the inputs the kernels read (light_gpu.bound for the former, D8's
rule on the well-conditioned rays for the latter -- no other tolerance); the table tiers; f16 and strided volumes; the module
against Raycaster's pose gradients; a NaN upstream gradient (D5)."""
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

import bundle_reference as BR  # noqa: E402
import camgrad_gpu as K  # noqa: E402
import light_gpu as LG  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402
import pose_gpu as PG  # noqa: E402

pytestmark = pytest.mark.gpu

C = LG.C
dev = PG.dev
bits = lambda t: t.contiguous().view(torch.int32)


def _F():
    from differender_amd import functional as F
    return F


def _opts(inp):
    return dict(t_near=inp.get("t_near"), jitter_seed=int(inp["jitter_seed"]), ray_base=int(inp["ray_base"]))


def _forward(inp, vol=None):
    """bundle_setup + march_bundle_fwd of inp on the device (vol: the device volume in the place of inp's, as float32) ->
    (vol, tf, o, d, e, x, n, out, steps)."""
    F = _F()
    vol = dev(inp["vol"]) if vol is None else vol
    tf, o, d = dev(inp["tf"]), dev(inp["origins"]), dev(inp["dirs"])
    e, x, n = F.bundle_setup(o, d, vol.shape, float(inp["sr"]), **_opts(inp))
    out, steps = F.march_bundle_fwd(vol, tf, o, d, e, x, n, int(inp["max_samples"]), float(inp["sr"]))
    return vol, tf, o, d, e, x, n, out, steps


@functools.lru_cache(maxsize=None)
def _state(scene, bundle):
    """The inputs and the two references of a gradient case (computed once and shared; nobody writes to them)."""
    inp = BR.inputs(scene, bundle)
    return (inp,) + BR.refs(inp)


def _masked_refs(inp, ref, ref32, mask):
    """The references' d_vol and d_tf for the upstream gradient of the rays in `mask` alone: the full runs' when that is every
    n > 1 ray of both, else two more runs over those rays."""
    if (mask == (ref["n"] > 1)).all() and (mask == (ref32["n"] > 1)).all():
        return ref, ref32
    return BR.run(inp, pixels=mask.reshape(-1)), BR.run(inp, torch.float32, pixels=mask.reshape(-1))


def _parity(inp, ref, ref32, what, vol=None, also=None, dvol=True):
    """Group 3's comparison. n equals the float32 transliteration's on the kept rays (pose_gpu.keep's rule), and steps on those
    that are marched (the references march no single-sample ray, H6); the image, d_vol and d_tf are within light_gpu.bound of
    float64, the upstream gradient zero off the kept n > 1 rays.
    also(vol, tf, o, d, e, x, n, g, out) -> (d_vol, d_tf): a second backward to hold to the same bar. dvol=False: the image and
    d_tf only."""
    F = _F()
    vol, tf, o, d, e, x, n, out, steps = _forward(inp, vol)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    keep = BR.keep(ref, ref32)
    live = keep & (ref["n"] > 1)
    n_k, steps_k = n.cpu().numpy().reshape(-1, 1), steps.cpu().numpy().reshape(-1, 1)
    assert (n_k[keep] == ref32["n"][keep]).all() and (steps_k[live] == ref32["steps"][live]).all(), what
    miss = ref["n"] == 0
    assert (n_k[miss] == 0).all() and (steps_k[miss] == 0).all() and (C(out).reshape(-1, 1, 4)[miss] == 0).all(), what
    mask = live
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    m4 = mask[..., None]
    LG.bound(C(out).reshape(-1, 1, 4) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, f"{what} rgba")
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * m4).reshape(-1, 4)
    r, r32 = _masked_refs(inp, ref, ref32, mask)
    backwards = [("bundle", F.march_bundle_bwd(vol, tf, o, d, e, x, n, S, sr, g, out))]
    if also is not None:
        backwards.append(("also", also(vol, tf, o, d, e, x, n, g, out)))
    for tag, (d_vol, d_tf) in backwards:
        if dvol:
            LG.bound(C(d_vol), r["dvol"], r32["dvol"], f"{what} {tag} dvol")
        LG.bound(C(d_tf), r["dtf"], r32["dtf"], f"{what} {tag} dtf")
    return vol, tf, o, d, e, x, n, out, steps, mask


# ---- 1. a pinhole camera's rays: its buffers, image and steps, bit for bit ----------------------------------------------------------

PINHOLE = ("a_orbit_sr1", "b_sr2_ert", "c_clip", "j_inside")
D_JITTER_SEED = CG.CASES["d_jitter"][7]


def _pinhole(name, seed):
    """Case `name` of make_camgrad_golden on the device, its ray_setup buffers, and the same rays as a bundle in [W][H] order."""
    F = _F()
    inp = CG.make_inputs(name)
    W, H = inp["grad_out"].shape[:2]
    vol, tf, cam = dev(inp["vol"]), dev(inp["tf"]), dev(inp["cam"][None])
    rays = F.ray_setup(cam, (W, H), vol.shape, float(inp["sr"]), jitter_seed=seed, view_base=CG.VIEW)
    o, d = cam.expand(W * H, 3).contiguous(), rays[2].reshape(W * H, 3)
    return inp, vol, tf, cam, rays, o, d


@pytest.mark.parametrize("seed", [0, D_JITTER_SEED], ids=["no_jitter", "jitter"])
@pytest.mark.parametrize("name", PINHOLE)
def test_a_pinhole_cameras_rays_give_its_buffers_image_and_steps_bit_for_bit(hiplib, name, seed):
    F, N = _F(), LG.native()
    inp, vol, tf, cam, (e0, x0, r0, n0), o, d = _pinhole(name, seed)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    # (view 0 of a launch whose view_base is CG.VIEW hashes (seed, CG.VIEW, pixel i H + j): ray_base = CG.VIEW, p = i H + j)
    e, x, n = F.bundle_setup(o, d, vol.shape, sr, None, seed, ray_base=CG.VIEW)
    assert torch.equal(bits(e), bits(e0.reshape(-1))) and torch.equal(bits(x), bits(x0.reshape(-1)))
    assert torch.equal(n, n0.reshape(-1)) and int((n > 1).sum()) > 50
    out0, steps0 = F.march_fwd(vol, tf, cam, e0, x0, r0, n0, S, sr, variant=N.DR_VARIANT_BASELINE)
    out, steps = F.march_bundle_fwd(vol, tf, o, d, e, x, n, S, sr)
    assert torch.equal(bits(out), bits(out0.reshape(-1, 4))) and torch.equal(steps, steps0.reshape(-1))
    if seed != 0:
        assert not torch.equal(bits(e), bits(F.bundle_setup(o, d, vol.shape, sr, None, seed, ray_base=CG.VIEW + 1)[0]))


@pytest.mark.parametrize("name", PINHOLE)
def test_a_pinhole_bundles_d_vol_and_d_tf_and_the_baselines_match_the_f64_reference(hiplib, name):
    """Float atomics reorder: both backwards are held to the float64 reference, not to each other's bits."""
    F, N = _F(), LG.native()
    base, vol, tf, cam, (e0, x0, r0, n0), o, d = _pinhole(name, 0)
    W, H = n0.shape[1:]
    S, sr = int(base["max_samples"]), float(base["sr"])
    inp = dict(vol=BR.F32(base["vol"]), tf=BR.F32(base["tf"]), origins=C(o), dirs=C(d), grad_out=BR.F32(base["grad_out"]).reshape(-1, 4),
               sr=base["sr"], max_samples=base["max_samples"], jitter_seed=0, ray_base=0)
    ref, ref32 = BR.run(inp), BR.run(inp, torch.float32)

    def baseline(vol, tf, o, d, e, x, n, g, out):
        return F.march_bwd(vol, tf, cam, e.reshape(1, W, H), x.reshape(1, W, H), d.reshape(1, W, H, 3), n.reshape(1, W, H), S, sr,
                           g.reshape(1, W, H, 4), out.reshape(1, W, H, 4), variant=N.DR_VARIANT_BASELINE)

    _parity(inp, ref, ref32, name, also=baseline)


# ---- 2. the launch tail --------------------------------------------------------------------------------------------------------------

TAIL = (1, 63, 64, 65, 255, 256, 257)
CANARY = 12345.0


def _tail_run(inp, count, vol, tf, S, sr):
    """The first `count` rays through the four entries on buffers 8 rays longer, pre-filled with CANARY."""
    F, N = _F(), LG.native()
    o, d = dev(inp["origins"][:count]), dev(inp["dirs"][:count])
    pad = count + 8
    fbuf = lambda *k: torch.full((pad, *k), CANARY, device="cuda")
    e, x, n = fbuf(), fbuf(), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = N.lib().dr_bundle_setup(o.data_ptr(), d.data_ptr(), count, *vol.shape, sr, -math.inf, 0, 0, e.data_ptr(), x.data_ptr(),
                                 n.data_ptr(), stream)
    assert rc == 0
    head = F._bundle_head(vol, tf, o, d, e[:count], x[:count], n[:count], S, sr)[3]
    out, steps = fbuf(4), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    assert N.lib().dr_march_bundle_fwd(*head, out.data_ptr(), steps.data_ptr(), stream) == 0
    g = dev(inp["grad_out"][:count])
    d_o, d_d = fbuf(3), fbuf(3)
    assert N.lib().dr_march_bundle_bwd_rays(*head, steps.data_ptr(), -math.inf, 0, 0, g.data_ptr(), out.data_ptr(), d_o.data_ptr(),
                                            d_d.data_ptr(), stream) == 0
    d_vol, d_tf = F.march_bundle_bwd(vol, tf, o, d, e[:count], x[:count], n[:count], S, sr, g, out[:count])
    torch.cuda.synchronize()
    return dict(e=e, x=x, n=n, out=out, steps=steps, d_o=d_o, d_d=d_d), d_vol, d_tf


def test_the_launch_tail_writes_its_own_rays_and_nothing_else(hiplib):
    inp = BR.inputs("a_orbit_sr1", "random", rays=BR.random_bundle(max(TAIL)))
    vol, tf, S, sr = dev(inp["vol"]), dev(inp["tf"]), int(inp["max_samples"]), float(inp["sr"])
    full, d_vol, d_tf = _tail_run(inp, max(TAIL), vol, tf, S, sr)
    assert int((full["n"][:max(TAIL)] > 1).sum()) == max(TAIL) and float(d_vol.abs().max()) > 0 and float(d_tf.abs().max()) > 0
    assert float(full["d_o"][:max(TAIL)].abs().max()) > 0 and float(full["d_d"][:max(TAIL)].abs().max()) > 0
    for count in TAIL:
        got, d_vol, d_tf = _tail_run(inp, count, vol, tf, S, sr)
        assert bool(torch.isfinite(d_vol).all()) and bool(torch.isfinite(d_tf).all())
        for k, t in got.items():
            assert torch.equal(bits(t[:count]), bits(full[k][:count])), (count, k)
            canary = t[count:]
            assert bool((canary == (77 if t.dtype == torch.int32 else CANARY)).all()), (count, k)


# ---- 3. float64 parity off the pinhole: image, d_vol, d_tf, n, steps -----------------------------------------------------------------

PARITY = [(s, b) for s, b in BR.GRAD_CASES if s != "m_object_in_air" and b != "random_jitter"]


@pytest.mark.parametrize("scene,bundle", PARITY, ids=lambda v: str(v))
def test_image_d_vol_and_d_tf_match_the_f64_reference(hiplib, scene, bundle):
    """Measured on the MI355X, d_vol as err / err32 / scale: a_orbit_sr1 ortho 1.7e-4 / 3.7e-3 / 2.8, random 3.0e-4 / 1.6e-3 /
    5.0, interior 2.4e-4 / 7.9e-4 / 3.7, interior_near0 7.4e-5 / 2.4e-3 / 3.1; b_sr2_ert ortho 2.6e-4 / 1.3e-3 / 10.5, random
    4.6e-4 / 1.2e-3 / 8.7, interior 7.3e-4 / 7.8e-3 / 13.0, interior_near0 1.9e-4 / 1.3e-3 / 9.4.
    b_sr2_ert x random is why march_bundle_bwd_kernel projects its adjoints with a normal from double taps (shade_for_adjoint):
    with the baseline kernels' float32 normal its d_vol was 6.6e-3 off (5.3 x err32), all of it ray 84's, at voxel (17, 12, 23),
    a corner of the cell of its first three samples. The central differences of the normal are 1.2e-4 .. 2.2e-4 there (1e-3
    elsewhere on the ray) and the taps float32 numbers near 0.5, good to 3e-8 each: the unit normal g / |g| carries 1e-3 of
    rounding noise in any float32 evaluation, and its adjoint scales with 1 / |g| (the float32 transliteration with its lerps
    spelled x + (y - x) a is 4.4e-3 off on that ray, with y - (y - x)(1 - a) 2.5e-3, as it stands 1.2e-3; march_bwd with
    variant=BASELINE on the same 192 rays, one 1 x 1 view each, 6.594e-3)."""
    inp, ref, ref32 = _state(scene, bundle)
    if bundle == "ortho":
        assert (ref["n"] == 0).sum() == 4   # four rays of the grid miss the box: pixel 0, steps 0 (_parity), gradients 0 (below)
    if "near0" in bundle:
        off = BR.run(dict(inp, t_near=None), grads=False)
        assert (ref["n"] < off["n"]).all()   # every interior ray is shorter than its line
    _parity(inp, ref, ref32, (scene, bundle))


# ---- 4. the ray gradients -----------------------------------------------------------------------------------------------------------

def ray_rule(ray, ref, ref32, mask, what=None):
    """D8's rule (camgrad_gpu.d8_rule's per-ray part) for the columns of d_origin and of d_dir, each by its own scale: the
    compared rays are more than 80 % of the n > 1 rays, per ray err <= 3 err32 + 1e-4 scale, exact zeros off the mask."""
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum(), (what, mask.sum(), (ref["n"] > 1).sum())
    assert np.isfinite(ray).all() and (ray[~mask] == 0).all(), what
    for name, sl in BR.COLUMNS:
        want = ref["dray"][..., sl] * mask[..., None]
        scale = np.abs(want).max()
        err = np.abs(ray[..., sl] - want)[mask].max()
        err32 = np.abs(ref32["dray"][..., sl] - ref["dray"][..., sl])[mask].max()
        print("raygrad", what, name, "err/scale %.3g err32/scale %.3g rays %d" % (err / scale, err32 / scale, mask.sum()))
        assert scale > 0 and err <= 3.0 * err32 + 1e-4 * scale, (what, name, err / scale, err32 / scale)


@pytest.mark.parametrize("scene,bundle", BR.GRAD_CASES, ids=lambda v: str(v))
def test_ray_gradients_match_the_f64_reference_on_the_well_conditioned_rays(hiplib, scene, bundle):
    F = _F()
    inp, ref, ref32 = _state(scene, bundle)
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    good = K.well_conditioned(ref, ref32, BR.keep(ref, ref32), "dray", BR.COLUMNS, (scene, bundle))
    agree = (steps.cpu().numpy().reshape(-1, 1) == ref["steps"]) & (n.cpu().numpy().reshape(-1, 1) == ref["n"])
    mask = good & agree   # rays whose f32 march stops elsewhere get a zero upstream gradient, as camgrad_gpu.launch gives them
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * mask[..., None]).reshape(-1, 4)
    d_o, d_d = F.march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]), g, out,
                                       **_opts(inp))
    ray = np.concatenate([C(d_o), C(d_d)], -1).reshape(-1, 1, 6)
    ray_rule(ray, ref, ref32, mask, (scene, bundle))
    if bundle == "random_jitter":   # the draw matters: the jitter-free gradient is another one
        assert np.abs(_state(scene, "random")[1]["dray"] - ref["dray"]).max() > 1e-2 * np.abs(ref["dray"]).max()


def test_the_ray_rule_rejects_a_one_percent_error():
    """camgrad_gpu.mutation_check's idea, with arrays in the kernel's place: the float32 reference passes the rule, the float64
    reference made 1 % too large does not."""
    inp, ref, ref32 = _state("a_orbit_sr1", "random")
    good = K.well_conditioned(ref, ref32, BR.keep(ref, ref32), "dray", BR.COLUMNS)
    m = good[..., None]
    ray_rule(ref32["dray"] * m, ref, ref32, good)
    with pytest.raises(AssertionError):
        ray_rule(1.01 * ref["dray"] * m, ref, ref32, good)


# ---- 5. the table tiers -------------------------------------------------------------------------------------------------------------

TIER_R = (3392, 3393, 10176, 10177)


@functools.lru_cache(maxsize=None)
def _tier_state(R):
    from oracle import oracle as O
    rng = np.random.RandomState(R)
    vol = np.clip(O.synth_volume((13, 12, 14), dtype=np.float64) + 0.02 * rng.standard_normal((13, 12, 14)), 0.0, 1.0)
    tf = rng.uniform(0.05, 0.95, size=(R, 4))
    tf[:, 3] = rng.uniform(0.01, 0.08, size=R)
    inp = BR.inputs("a_orbit_sr1", "random", vol=vol, tf=tf, head=64)
    return inp, BR.run(inp), BR.run(inp, torch.float32)


@pytest.mark.parametrize("R", TIER_R)
def test_table_tiers_match_the_f64_reference(hiplib, R):
    """The image and d_tf. (Not d_vol: with thousands of unrelated texels a sample's intensity adjoint is the slope between two
    random neighbours times R - 1, and whether I (R - 1) falls left or right of a texel boundary is decided within float32
    rounding for a sample or two of every run: the float32 transliteration itself is then percents of the scale off.)"""
    inp, ref, ref32 = _tier_state(R)
    _parity(inp, ref, ref32, ("R", R), dvol=False)


@pytest.mark.parametrize("Ra,Rb", [(3392, 3393), (10176, 10177)])
def test_neighbouring_table_sizes_differ_as_the_reference_does(hiplib, Ra, Rb):
    (ia, ra, ra32), (ib, rb, rb32) = _tier_state(Ra), _tier_state(Rb)
    mask = (BR.keep(ra, ra32) & BR.keep(rb, rb32) & (ra["n"] > 1))[..., None]
    got = [C(_forward(i)[7]).reshape(-1, 1, 4) for i in (ia, ib)]
    assert np.abs(ra["rgba"] - rb["rgba"]).max() > 1e-3
    LG.bound((got[0] - got[1]) * mask, (ra["rgba"] - rb["rgba"]) * mask, (ra32["rgba"] - rb32["rgba"]) * mask, ("R", Ra, Rb))


# ---- 6. an f16 volume, a strided volume ---------------------------------------------------------------------------------------------

def test_an_f16_volume_matches_the_f64_reference_on_the_volume_the_kernel_reads(hiplib):
    base = BR.inputs("a_orbit_sr1", "random")
    inp = dict(base, vol=PG.F16(base["vol"]))
    vol = dev(inp["vol"]).half()
    assert np.array_equal(C(vol), inp["vol"]) and not np.array_equal(inp["vol"], base["vol"])
    _parity(inp, BR.run(inp), BR.run(inp, torch.float32), "f16", vol=vol)


def test_a_permuted_volume_matches_the_f64_reference(hiplib):
    inp, ref, ref32 = _state("a_orbit_sr1", "random")
    vol = dev(np.ascontiguousarray(inp["vol"].transpose(2, 0, 1))).permute(1, 2, 0)
    assert not vol.is_contiguous() and vol.stride(0) != 1 and np.array_equal(C(vol), inp["vol"])
    _parity(inp, ref, ref32, "permuted", vol=vol)


# ---- 7. the module, end to end --------------------------------------------------------------------------------------------------------

POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
CAM = (-1.3, 0.9, 2.0)


def test_module_on_pinhole_rays_gives_raycasters_image_and_pose_gradients(hiplib):
    from differender_amd.bundle import RayBundleRaycaster, pinhole_rays
    from differender_amd.volume_raycaster import Raycaster
    inp = PG.inputs("a_orbit_sr1", look_from=np.array(CAM), **POSE)
    ref, ref32 = PG.refs(inp)
    W, H = ref["n"].shape
    S, R = int(inp["max_samples"]), inp["tf"].shape[0]
    vol = dev(inp["vol"]).permute(1, 2, 0)[None]   # (1, D, H, W) of the field (W, D, H)
    tf = dev(inp["tf"]).t()
    kernel_order = lambda img: torch.flip(img, (0,)).transpose(0, 1)   # (H, W, ...) user orientation -> (W, H, ...)
    leaves = lambda: [torch.tensor(np.asarray(a, np.float64), dtype=torch.float32, device="cuda").requires_grad_(True)
                      for a in (inp["look_from"], inp["look_at"], inp["up"], math.degrees(float(inp["fov_rad"])))]

    def ten(ls):   # the gradients as the reference's ten columns: fov per radian
        return np.concatenate([C(ls[0].grad), C(ls[1].grad), C(ls[2].grad), [float(ls[3].grad) * 180.0 / math.pi]])

    rb = RayBundleRaycaster(vol.shape[-3:], R, jitter=False, max_samples=S, ray_grad=True)
    lb = leaves()
    img_b = rb(vol, tf, *pinhole_rays(*lb, (W, H)))
    assert img_b.shape == (H, W, 4) and rb._steps.shape == (H, W)
    rr = Raycaster(vol.shape[-3:], (W, H), R, jitter=False, max_samples=S)
    lr = leaves()
    img_r = rr(vol, tf, lr[0], look_at=lr[1], up=lr[2], fov=lr[3])
    assert img_r.shape == (4, H, W)
    out_b, out_r = C(kernel_order(img_b)), C(img_r.permute(2, 1, 0).flip(1))
    steps_b, steps_r = kernel_order(rb._steps).cpu().numpy(), rr.vr._steps.cpu().numpy().reshape(W, H)
    mask = PG.keep(ref, ref32) & (ref["n"] > 1) & (steps_b == ref["steps"]) & (steps_r == ref["steps"])
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    m4 = mask[..., None]
    LG.bound(out_b * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "bundle module image")
    LG.bound(out_r * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "Raycaster image")
    g = dev(inp["grad_out"] * m4)   # (W, H, 4), zero off the mask
    (kernel_order(img_b) * g).sum().backward()
    (img_r.permute(2, 1, 0).flip(1) * g).sum().backward()
    PG.pose_total_rule(ten(lb), ref["dpose_ray"], ref32["dpose_ray"], mask, "bundle module")
    PG.pose_total_rule(ten(lr), ref["dpose_ray"], ref32["dpose_ray"], mask, "Raycaster")


# ---- 8. a NaN upstream gradient (D5) -------------------------------------------------------------------------------------------------

def test_a_nan_upstream_ray_gets_zeros_and_leaves_the_others_alone(hiplib):
    from differender_amd.bundle import RayBundleRaycaster
    F = _F()
    inp, ref, _ = _state("a_orbit_sr1", "random")
    vol, tf, o, d, e, x, n, out, steps = _forward(inp)
    S, sr, bad = int(inp["max_samples"]), float(inp["sr"]), 7
    assert ref["n"][bad, 0] > 1
    g = dev(inp["grad_out"])
    clean = F.march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    g_nan = g.clone()
    g_nan[bad, 1] = float("nan")
    got = F.march_bundle_bwd_rays(vol, tf, o, d, e, x, n, steps, S, sr, g_nan, out, **_opts(inp))
    others = torch.arange(len(g), device="cuda") != bad
    for a, b in zip(got, clean):
        assert bool((a[bad] == 0).all()) and float(b[bad].abs().max()) > 0
        assert torch.equal(bits(a[others]), bits(b[others]))
    # the plain backward propagates the NaN like the reference; the module's gradients end in nan_to_num
    d_vol, d_tf = F.march_bundle_bwd(vol, tf, o, d, e, x, n, S, sr, g_nan, out)
    assert bool(torch.isnan(d_vol).any()) and bool(torch.isnan(d_tf).any())
    rc = RayBundleRaycaster(vol.permute(1, 2, 0).shape, tf.shape[0], jitter=False, max_samples=S, ray_grad=True)
    v, t = vol.permute(1, 2, 0)[None].clone().requires_grad_(True), tf.t().clone().requires_grad_(True)
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    (rc(v, t, oo, dd) * g_nan).sum().backward()
    for leaf in (v, t, oo, dd):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert bool((oo.grad[bad] == 0).all()) and bool((dd.grad[bad] == 0).all())
