"""The RGBA march over ray bundles on the GPU: a pinhole camera's rays give RaycasterRGBA's buffers, image and
steps bit for bit; the launch tail; the image, d_vol and the per-ray d_origin / d_dir against the float64 autograd reference of
tests/rgba_bundle_reference.py, run at test time on the inputs the kernels read (light_gpu.bound for the former,
test_gpu_bundle.ray_rule on the well-conditioned rays for the latter -- no other tolerance); f16, strided, interleaved and
misaligned volumes; single-sample rays; the module against RaycasterRGBA's pose gradients; a NaN upstream gradient (D5)."""
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
import pose_gpu as PG  # noqa: E402
import rgba_bundle_reference as RB  # noqa: E402
import rgba_camera_scenes as SC  # noqa: E402
import rgba_pose_reference as RP  # noqa: E402
from test_gpu_bundle import ray_rule  # noqa: E402

pytestmark = pytest.mark.gpu

C = LG.C
dev = PG.dev
bits = lambda t: t.contiguous().view(torch.int32)


def _F():
    from differender_amd import functional as F
    return F


def _opts(inp):
    return dict(t_near=inp.get("t_near"), jitter_seed=int(inp["jitter_seed"]), ray_base=int(inp["ray_base"]))


def _volume(vol, layout="planar", dtype=torch.float32):
    """The host volume (4, VX, VY, VZ) on the device as `dtype`, the same logical tensor in one of four layouts: planar
    (contiguous), interleaved (rgba.interleaved: the one-load path), offset (interleaved, its storage one element off a voxel's
    alignment) or permuted (the z axis outermost in memory)."""
    from differender_amd.rgba import interleaved
    v = dev(vol).to(dtype)
    if layout == "interleaved":
        v = interleaved(v)
        assert v.stride(0) == 1 and v.data_ptr() % (4 * v.element_size()) == 0
    elif layout == "offset":
        buf = torch.empty(v.numel() + 1, dtype=dtype, device=v.device)
        w = buf[1:].view(*v.shape[1:], 4).movedim(-1, 0)
        w.copy_(v)
        assert w.stride(0) == 1 and w.data_ptr() % (4 * w.element_size()) == w.element_size()
        v = w
    elif layout == "permuted":
        v = v.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
        assert not v.is_contiguous() and v.stride(3) != 1
    else:
        assert layout == "planar" and v.is_contiguous()
    assert np.array_equal(C(v), np.asarray(vol, np.float64) if dtype == torch.float32 else PG.F16(vol))
    return v


def _forward(inp, vol=None):
    """bundle_setup + march_rgba_bundle_fwd of inp on the device (vol: the device volume in the place of inp's, as float32) ->
    (vol, o, d, e, x, n, out, steps)."""
    F = _F()
    vol = _volume(inp["vol"]) if vol is None else vol
    o, d = dev(inp["origins"]), dev(inp["dirs"])
    e, x, n = F.bundle_setup(o, d, vol.shape[-3:], float(inp["sr"]), **_opts(inp))
    out, steps = F.march_rgba_bundle_fwd(vol, o, d, e, x, n, int(inp["max_samples"]), float(inp["sr"]))
    return vol, o, d, e, x, n, out, steps


def _masked_refs(inp, ref, ref32, mask):
    """The references' d_vol for the upstream gradient of the rays in `mask` alone: the full runs' when that is every n > 1 ray
    of both, else two more runs over those rays."""
    if (mask == (ref["n"] > 1)).all() and (mask == (ref32["n"] > 1)).all():
        return ref, ref32
    return RB.run(inp, pixels=mask.reshape(-1)), RB.run(inp, torch.float32, pixels=mask.reshape(-1))


def _parity(inp, ref, ref32, what, vol=None, d_vol_like=()):
    """Group 3's comparison. n equals the float32 transliteration's on the kept rays (bundle_reference.keep's rule), and steps on
    those that are marched (the references march no single-sample ray, H6); rays that miss the box give pixel 0, steps 0 and zero
    gradients; the image and d_vol are within light_gpu.bound of float64, the upstream gradient zero off the kept n > 1 rays,
    which are more than 80 % of the n > 1 rays.
    d_vol_like: layouts (_volume's) of further zeroed gradient buffers the backward is to accumulate into, each held to the same
    bar. -> (vol, o, d, e, x, n, out, steps, mask)."""
    F = _F()
    vol, o, d, e, x, n, out, steps = _forward(inp, vol)
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    keep = RB.keep(ref, ref32)
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
    d_vol = F.march_rgba_bundle_bwd(vol, o, d, e, x, n, S, sr, g, out)
    assert d_vol.dtype == torch.float32 and d_vol.shape == vol.shape and d_vol.stride() == vol.stride()
    LG.bound(C(d_vol), r["dvol"], r32["dvol"], f"{what} dvol")
    for layout in d_vol_like:
        buf = _volume(np.zeros(vol.shape), layout)
        got = F.march_rgba_bundle_bwd(vol, o, d, e, x, n, S, sr, g, out, d_vol=buf)
        assert got is buf
        LG.bound(C(buf), r["dvol"], r32["dvol"], f"{what} dvol into a {layout} buffer")
    d_o, d_d = F.march_rgba_bundle_bwd_rays(vol, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    off = ~mask.reshape(-1)
    assert bool((d_o.cpu()[off] == 0).all()) and bool((d_d.cpu()[off] == 0).all()), what   # (the rays that miss among them)
    return vol, o, d, e, x, n, out, steps, mask


def _ray_gradients(inp, ref, ref32, what, vol=None):
    """Group 4's launch: the upstream gradient on the well-conditioned rays (camgrad_gpu.well_conditioned, no lighting) whose n
    and steps are the reference's, zero elsewhere -> (ray (P, 1, 6), mask, (vol, o, d, e, x, n, out, steps))."""
    F = _F()
    fw = _forward(inp, vol)
    vol, o, d, e, x, n, out, steps = fw
    good = K.well_conditioned(ref, ref32, RB.keep(ref, ref32), "dray", RB.COLUMNS, what, lit=False)
    agree = (steps.cpu().numpy().reshape(-1, 1) == ref["steps"]) & (n.cpu().numpy().reshape(-1, 1) == ref["n"])
    mask = good & agree
    g = dev(inp["grad_out"].reshape(-1, 1, 4) * mask[..., None]).reshape(-1, 4)
    d_o, d_d = F.march_rgba_bundle_bwd_rays(vol, o, d, e, x, n, steps, int(inp["max_samples"]), float(inp["sr"]), g, out,
                                            **_opts(inp))
    return np.concatenate([C(d_o), C(d_d)], -1).reshape(-1, 1, 6), mask, fw


# ---- 1. a pinhole camera's rays: its buffers, image and steps, bit for bit ----------------------------------------------------------

VIEW = 2
CAMERAS = {"outside": (2.2, 1.1, 1.7), "inside": (0.3, 0.2, 0.4)}


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("seed", [0, 4242], ids=["no_jitter", "jitter"])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("volume", ["thin_sr1", "opaque_sr2"])
def test_a_pinhole_cameras_rays_give_its_buffers_image_and_steps_bit_for_bit(hiplib, volume, camera, seed, layout):
    F = _F()
    shape, kind, sr, S = RB.VOLUMES[volume]
    W, H = 13, 10
    vol = _volume(RB.RG.volume(shape, kind).double().numpy(), layout)
    cam = dev(np.array([CAMERAS[camera]]))
    e0, x0, r0, n0 = F.ray_setup(cam, (W, H), shape, sr, jitter_seed=seed, view_base=VIEW)
    o, d = cam.expand(W * H, 3).contiguous(), r0.reshape(W * H, 3)
    # (view 0 of a launch whose view_base is VIEW hashes (seed, VIEW, pixel i H + j): ray_base = VIEW, p = i H + j)
    e, x, n = F.bundle_setup(o, d, shape, sr, None, seed, ray_base=VIEW)
    assert torch.equal(bits(e), bits(e0.reshape(-1))) and torch.equal(bits(x), bits(x0.reshape(-1)))
    assert torch.equal(n, n0.reshape(-1)) and int((n > 1).sum()) > 50
    if camera == "inside":
        assert bool((e0 < 0).all()) and bool((n0 > 1).all())
    out0, steps0 = F.march_rgba_fwd(vol, cam, e0, x0, r0, n0, S, sr)
    out, steps = F.march_rgba_bundle_fwd(vol, o, d, e, x, n, S, sr)
    assert torch.equal(bits(out), bits(out0.reshape(-1, 4))) and torch.equal(steps, steps0.reshape(-1))
    assert float(out.abs().max()) > 0
    if volume == "opaque_sr2":
        assert int((steps < n).sum()) > 10   # rays that terminate early
    if seed != 0:
        assert not torch.equal(bits(e), bits(F.bundle_setup(o, d, shape, sr, None, seed, ray_base=VIEW + 1)[0]))


# ---- 2. the launch tail --------------------------------------------------------------------------------------------------------------

TAIL = (1, 63, 64, 65, 255, 256, 257)
CANARY = 12345.0


def _tail_run(inp, count, vol, S, sr):
    """The first `count` rays through the setup and the three entries on buffers 8 rays longer, pre-filled with CANARY."""
    F, N = _F(), LG.native()
    o, d = dev(inp["origins"][:count]), dev(inp["dirs"][:count])
    pad = count + 8
    fbuf = lambda *k: torch.full((pad, *k), CANARY, device="cuda")
    e, x, n = fbuf(), fbuf(), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = N.lib().dr_bundle_setup(o.data_ptr(), d.data_ptr(), count, *vol.shape[-3:], sr, -math.inf, 0, 0, e.data_ptr(),
                                 x.data_ptr(), n.data_ptr(), stream)
    assert rc == 0
    head = F._rgba_bundle_head(vol, o, d, e[:count], x[:count], n[:count], S, sr)[3]
    out, steps = fbuf(4), torch.full((pad,), 77, dtype=torch.int32, device="cuda")
    assert N.lib().dr_march_rgba_bundle_fwd(*head, out.data_ptr(), steps.data_ptr(), stream) == 0
    g = dev(inp["grad_out"][:count])
    d_o, d_d = fbuf(3), fbuf(3)
    assert N.lib().dr_march_rgba_bundle_bwd_rays(*head, steps.data_ptr(), -math.inf, 0, 0, g.data_ptr(), out.data_ptr(),
                                                 d_o.data_ptr(), d_d.data_ptr(), stream) == 0
    d_vol = F.march_rgba_bundle_bwd(vol, o, d, e[:count], x[:count], n[:count], S, sr, g, out[:count])
    torch.cuda.synchronize()
    return dict(e=e, x=x, n=n, out=out, steps=steps, d_o=d_o, d_d=d_d), d_vol


def test_the_launch_tail_writes_its_own_rays_and_nothing_else(hiplib):
    inp = RB.inputs("thin_sr1", "random", rays=BR.random_bundle(max(TAIL)))
    vol, S, sr = _volume(inp["vol"]), int(inp["max_samples"]), float(inp["sr"])
    full, d_vol = _tail_run(inp, max(TAIL), vol, S, sr)
    assert int((full["n"][:max(TAIL)] > 1).sum()) == max(TAIL) and float(d_vol.abs().max()) > 0
    assert float(full["d_o"][:max(TAIL)].abs().max()) > 0 and float(full["d_d"][:max(TAIL)].abs().max()) > 0
    for count in TAIL:
        got, d_vol = _tail_run(inp, count, vol, S, sr)
        assert bool(torch.isfinite(d_vol).all()) and float(d_vol.abs().max()) > 0
        for k, t in got.items():
            assert torch.equal(bits(t[:count]), bits(full[k][:count])), (count, k)
            canary = t[count:]
            assert bool((canary == (77 if t.dtype == torch.int32 else CANARY)).all()), (count, k)


# ---- 3. float64 parity: image, d_vol, n, steps ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("volume,bundle", RB.PARITY_CASES, ids=lambda v: str(v))
def test_image_and_d_vol_match_the_f64_reference(hiplib, volume, bundle):
    inp, ref, ref32 = RB.state(volume, bundle)
    if bundle == "ortho":
        assert (ref["n"] == 0).sum() == 4   # four rays of the grid miss the box: pixel 0, steps 0, gradients 0 (_parity)
    if "near0" in bundle:
        off = RB.run(dict(inp, t_near=None), grads=False)
        assert (ref["n"] < off["n"]).all()   # every interior ray is shorter than its line
    _parity(inp, ref, ref32, (volume, bundle))


# ---- 4. the ray gradients ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("volume,bundle", RB.RAY_CASES, ids=lambda v: str(v))
def test_ray_gradients_match_the_f64_reference_on_the_well_conditioned_rays(hiplib, volume, bundle):
    inp, ref, ref32 = RB.state(volume, bundle)
    live = ref["n"] > 1
    if bundle == "random_jitter":   # the draw matters: the jitter-free gradient is another one
        assert np.abs(RB.state(volume, "random")[1]["dray"] - ref["dray"]).max() > 1e-2 * np.abs(ref["dray"]).max()
    if bundle == "interior_near0":
        assert (ref["entry"] == 0).all()   # the clamp is taken on every ray
    if bundle in ("axial", "one_zero"):
        assert (((inp["dirs"] == 0).sum(1)) == (2 if bundle == "axial" else 1)).all()
    if volume == "thin_clip":
        assert int(inp["max_samples"]) < ref["n"].min()
    if volume == "opaque_sr2":
        assert (ref["steps"][live] < ref["n"][live]).sum() > 0.2 * live.sum()   # early termination, frozen by steps
    ray, mask, _ = _ray_gradients(inp, ref, ref32, (volume, bundle))
    ray_rule(ray, ref, ref32, mask, (volume, bundle))


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,dtype,d_vol_like", [
    ("planar", torch.float16, ()), ("interleaved", torch.float16, ()), ("permuted", torch.float32, ()),
    ("interleaved", torch.float32, ("planar",)), ("planar", torch.float32, ("interleaved",)), ("offset", torch.float32, ()),
], ids=["planar_f16", "interleaved_f16", "permuted", "interleaved_into_planar", "planar_into_interleaved", "offset"])
def test_volume_layouts_match_the_f64_reference_on_the_volume_the_kernel_reads(hiplib, layout, dtype, d_vol_like):
    """f16 (the reference runs on the half-rounded values), permuted strides, the interleaved one-load path, and an interleaved
    volume one element off its alignment, which takes the scalar path; d_vol into a buffer of the other layout. The image,
    d_vol and the ray gradients, each under its own bar."""
    base = RB.inputs("thin_sr1", "random")
    if dtype == torch.float16:
        inp = dict(base, vol=PG.F16(base["vol"]))
        assert not np.array_equal(inp["vol"], base["vol"])
        ref, ref32 = RB.refs(inp)
    else:
        inp, ref, ref32 = RB.state("thin_sr1", "random")
    vol = _volume(inp["vol"], layout, dtype)
    _parity(inp, ref, ref32, (layout, dtype), vol=vol, d_vol_like=d_vol_like)
    ray, mask, fw = _ray_gradients(inp, ref, ref32, (layout, dtype), vol=vol)
    ray_rule(ray, ref, ref32, mask, (layout, dtype))
    if layout in ("offset", "interleaved", "permuted") and dtype == torch.float32:
        # both paths read the same values and do the same arithmetic in the same order: the planar volume's bits
        ray_p, mask_p, fw_p = _ray_gradients(inp, ref, ref32, "planar")
        assert torch.equal(bits(fw[6]), bits(fw_p[6])) and torch.equal(fw[7], fw_p[7])
        assert np.array_equal(mask, mask_p) and np.array_equal(ray, ray_p)


# ---- 6. single-sample rays ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_single_sample_rays_contribute_nothing_and_leave_their_wave_alone(hiplib, layout):
    """Eight lanes of one wave have n == 1 (H6): pixel 0, steps 0, zero ray gradients, nothing in d_vol (the float64 reference
    marches no such ray); the other 56 lanes' bits are those of the 56 rays marched alone."""
    F = _F()
    inp, ref, ref32 = RB.state(*RB.SINGLE_CASE)
    one = BR.SINGLE
    vol = _volume(inp["vol"], layout)
    vol, o, d, e, x, n, out, steps, mask = _parity(inp, ref, ref32, ("single", layout), vol=vol)
    assert bool((n.cpu()[one] == 1).all()) and bool((n.cpu()[~one] > 1).all()) and not mask[one].any()
    assert bool((out.cpu()[one] == 0).all()) and bool((steps.cpu()[one] == 0).all())
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    g = dev(inp["grad_out"])
    d_o, d_d = F.march_rgba_bundle_bwd_rays(vol, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    assert bool((d_o.cpu()[one] == 0).all()) and bool((d_d.cpu()[one] == 0).all())
    alone = dict(inp, origins=inp["origins"][~one], dirs=inp["dirs"][~one])
    _, o2, d2, e2, x2, n2, out2, steps2 = _forward(alone, vol)
    rest = torch.from_numpy(~one).cuda()
    d_o2, d_d2 = F.march_rgba_bundle_bwd_rays(vol, o2, d2, e2, x2, n2, steps2, S, sr, g[rest], out2, **_opts(inp))
    for a, b in ((out, out2), (steps, steps2), (e, e2), (x, x2), (n, n2), (d_o, d_o2), (d_d, d_d2)):
        assert torch.equal(bits(a[rest]), bits(b))
    assert float(d_o2.abs().max()) > 0 and float(d_d2.abs().max()) > 0


# ---- 7. the module, end to end ----------------------------------------------------------------------------------------------------------------

POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
CAM = (-1.3, 0.9, 2.0)


def test_module_on_pinhole_rays_gives_raycaster_rgbas_image_and_pose_gradients(hiplib):
    from differender_amd.bundle import pinhole_rays
    from differender_amd.rgba import RayBundleRaycasterRGBA, RaycasterRGBA
    inp = SC.make(vshape=(10, 9, 11), WH=(12, 10), sr=1.0, S=512, seed=0, look_from=CAM, **POSE)
    ref, ref32 = RP.run_case(inp), RP.run_case(inp, dtype=torch.float32)
    W, H = ref["n"].shape
    S = int(inp["max_samples"])
    vol = dev(inp["vol"]).permute(0, 2, 3, 1)   # (4, D, H, W) of the field (4, W, D, H)
    kernel_order = lambda img: torch.flip(img, (0,)).transpose(0, 1)   # (H, W, ...) user orientation -> (W, H, ...)
    leaves = lambda: [torch.tensor(np.asarray(a, np.float64), dtype=torch.float32, device="cuda").requires_grad_(True)
                      for a in (inp["look_from"], inp["look_at"], inp["up"], math.degrees(float(inp["fov_rad"])))]

    def ten(ls):   # the gradients as the reference's ten columns: fov per radian
        return np.concatenate([C(ls[0].grad), C(ls[1].grad), C(ls[2].grad), [float(ls[3].grad) * 180.0 / math.pi]])

    rb = RayBundleRaycasterRGBA(vol.shape[-3:], jitter=False, max_samples=S, ray_grad=True)
    lb = leaves()
    vb = vol.clone().requires_grad_(True)
    img_b = rb(vb, *pinhole_rays(*lb, (W, H)))
    assert img_b.shape == (H, W, 4) and rb._steps.shape == (H, W)
    steps_b = kernel_order(rb._steps).cpu().numpy()
    with torch.no_grad():   # the same rays as (N, 3): the same bits
        o, d = pinhole_rays(*lb, (W, H))
        flat = rb(vol, o.reshape(-1, 3), d.reshape(-1, 3))
        assert flat.shape == (H * W, 4) and rb._steps.shape == (H * W,)
        assert torch.equal(bits(flat), bits(img_b.detach().reshape(-1, 4)))
    rr = RaycasterRGBA(vol.shape[-3:], (W, H), jitter=False, max_samples=S, camera_grad=True)
    lr = leaves()
    vr = vol.clone().requires_grad_(True)
    img_r = rr(vr, lr[0], look_at=lr[1], up=lr[2], fov=lr[3])
    assert img_r.shape == (4, H, W)
    out_b, out_r = C(kernel_order(img_b)), C(img_r.permute(2, 1, 0).flip(1))
    steps_r = rr._steps.cpu().numpy().reshape(W, H)
    mask = PG.keep(ref, ref32) & (ref["n"] > 1) & (steps_b == ref["steps"]) & (steps_r == ref["steps"])
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum()
    m4 = mask[..., None]
    LG.bound(out_b * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "bundle module image")
    LG.bound(out_r * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "RaycasterRGBA image")
    g = dev(inp["grad_out"] * m4)   # (W, H, 4), zero off the mask
    (kernel_order(img_b) * g).sum().backward()
    (img_r.permute(2, 1, 0).flip(1) * g).sum().backward()
    PG.pose_total_rule(ten(lb), ref["dpose_ray"], ref32["dpose_ray"], mask, "bundle module")
    PG.pose_total_rule(ten(lr), ref["dpose_ray"], ref32["dpose_ray"], mask, "RaycasterRGBA")
    for leaf in (vb, vr):   # the volume's gradient comes along
        assert leaf.grad.shape == vol.shape and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0


def test_a_module_without_ray_grad_refuses_rays_that_require_grad(hiplib):
    from differender_amd.rgba import RayBundleRaycasterRGBA
    rc = RayBundleRaycasterRGBA((8, 9, 10), jitter=False)
    vol = torch.rand(4, 8, 9, 10, device="cuda").requires_grad_(True)
    o = torch.tensor([[0.1, 0.2, 3.0]] * 5, device="cuda")
    d = torch.tensor([[0.0, 0.0, -2.0]] * 5, device="cuda")   # (not unit vectors: the module normalises)
    with pytest.raises(ValueError, match="no gradient w.r.t. origins.*ray_grad=True"):
        rc(vol, o.clone().requires_grad_(True), d)
    with pytest.raises(ValueError, match="no gradient w.r.t. directions.*ray_grad=True"):
        rc(vol, o, d.clone().requires_grad_(True))
    out = rc(vol, o, d)   # without them it renders, and the volume gets its gradient
    out.sum().backward()
    assert out.shape == (5, 4) and float(out.detach().abs().max()) > 0 and float(vol.grad.abs().max()) > 0


# ---- 8. a NaN upstream gradient (D5) ---------------------------------------------------------------------------------------------------------

def test_a_nan_upstream_ray_gets_zeros_and_leaves_the_others_alone(hiplib):
    from differender_amd.rgba import RayBundleRaycasterRGBA
    F = _F()
    inp, ref, _ = RB.state("thin_sr1", "random")
    vol, o, d, e, x, n, out, steps = _forward(inp)
    S, sr, bad = int(inp["max_samples"]), float(inp["sr"]), 7
    assert ref["n"][bad, 0] > 1
    g = dev(inp["grad_out"])
    clean = F.march_rgba_bundle_bwd_rays(vol, o, d, e, x, n, steps, S, sr, g, out, **_opts(inp))
    g_nan = g.clone()
    g_nan[bad, 1] = float("nan")
    got = F.march_rgba_bundle_bwd_rays(vol, o, d, e, x, n, steps, S, sr, g_nan, out, **_opts(inp))
    others = torch.arange(len(g), device="cuda") != bad
    for a, b in zip(got, clean):
        assert bool((a[bad] == 0).all()) and float(b[bad].abs().max()) > 0
        assert torch.equal(bits(a[others]), bits(b[others]))
    # the plain backward propagates the NaN like the reference; the module's gradients end in nan_to_num
    assert bool(torch.isnan(F.march_rgba_bundle_bwd(vol, o, d, e, x, n, S, sr, g_nan, out)).any())
    user = vol.permute(0, 2, 3, 1)   # (4, D, H, W) of the field (4, W, D, H)
    rc = RayBundleRaycasterRGBA(user.shape[-3:], jitter=False, max_samples=S, ray_grad=True)
    v = user.clone().requires_grad_(True)
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    (rc(v, oo, dd) * g_nan).sum().backward()
    for leaf in (v, oo, dd):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert bool((oo.grad[bad] == 0).all()) and bool((dd.grad[bad] == 0).all())
