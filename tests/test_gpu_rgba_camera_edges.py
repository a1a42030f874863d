"""march_rgba_cam_kernel (csrc/march_rgba.hip) where the scenes of test_gpu_rgba_camera.py do not reach: images of
several workgroups (the f64 reduction across them, a last workgroup with idle waves, idle tiles off the object), three views
of several workgroups each with their own poses, fovs and volumes, the scalar-load instances on non-dense, channel-first,
misaligned and permuted volumes, sampling rates 0.6 ... 8, max_samples 1 and 2, stretched volumes and two-voxel axes, the camera
inside the box with jitter, an alpha above one (a NaN pixel, D5), colours outside [0, 1], and RaycasterRGBA(camera_grad=True)
with jitter. Every expected value is the float64 autograd reference of tests/rgba_pose_reference.py, run at test time on the
inputs the kernel reads, with the kernel on the reference's ray buffers; the bars are the family's own (pose_gpu.pose_rule for
dr_march_rgba_bwd_pose, camgrad_gpu.d8_rule for dr_march_rgba_bwd_cam under the default pose, their total rules where only a
total exists), over the kept rays and again over the well-conditioned ones. tests/test_rgba_camera.py holds every scene here
to the conditions of that second pass without a GPU (CONDITIONED)."""
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
import pose_gpu as PG  # noqa: E402
import rgba_camera_scenes as SC  # noqa: E402
import rgba_pose_reference as RP  # noqa: E402
import test_gpu_rgba_camera as TG  # noqa: E402
from pose_gpu import COLUMNS, dev  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SCENES = {"opaque": dict(opaque=True, sr=2.0, seed=77), "thin": dict(opaque=False, sr=1.0, seed=0)}


def _alpha_above_one(vol):
    vol = vol.copy()
    vol[3, 4:7, 3:6, 4:7] = 1.5
    return vol


def _colours_out_of_range(vol):
    vol = vol.copy()
    vol[:3] = vol[:3] * 3.0 - 1.0
    return SC.F32(vol)


EDITS = {"alpha_1.5": _alpha_above_one, "colours": _colours_out_of_range}


@functools.lru_cache(maxsize=None)
def _case(scene="opaque", posed=True, f16=False, edit=None, **over):
    """(inputs, float64 reference, float32 reference), computed once and shared (read only). scene: "opaque" (rate 2, jitter
    seed 77) or "thin" (rate 1, no jitter) under SC.POSED -- posed=False: the default pose, which dr_march_rgba_bwd_cam is held
    to -- or a case of rgba_camera_scenes.CASES with its own pose; `over` is laid over it; edit: a change of the volume's
    values (EDITS); f16: the references run on the f16-rounded volume the kernel reads."""
    if scene in SC.CASES:
        kw = dict(SC.CASES[scene])
    else:
        kw = dict(SCENES[scene])
        kw.update(SC.POSED if posed else {})
    kw.update(over)
    inp = SC.make(**kw)
    if edit is not None:
        inp["vol"] = EDITS[edit](inp["vol"])
    if f16:
        inp["vol"] = PG.F16(inp["vol"])
    return inp, RP.run_case(inp), RP.run_case(inp, dtype=torch.float32)


# id -> the arguments of _case; id + "_cam": the same scene under the default pose, for the look_from entry
EDGE = {
    "wg3_17x19": dict(scene="opaque", WH=(17, 19)),
    "wide_33x9": dict(scene="thin", WH=(33, 9)),
    "one_ray": dict(scene="opaque", WH=(1, 1)),
    "strides_f32": dict(scene="opaque"),
    "strides_f16": dict(scene="opaque", f16=True),
    "sr0.6": dict(scene="opaque", sr=0.6, seed=31),
    "sr1.3": dict(scene="thin", sr=1.3, seed=31),
    "sr4": dict(scene="opaque", sr=4.0, seed=0),
    "sr8": dict(scene="thin", sr=8.0, seed=5),
    "clip_S1": dict(scene="clip_S6", S=1),
    "clip_S2": dict(scene="clip_S6", S=2),
    "slopes_20x6x11": dict(scene="thin", vshape=(20, 6, 11)),
    "two_voxels_x": dict(scene="opaque", vshape=(2, 9, 11)),
    "two_voxels_y": dict(scene="opaque", vshape=(10, 2, 11)),
    "two_voxels_z": dict(scene="opaque", vshape=(10, 9, 2)),
    "inside_sr2_jit": dict(scene="inside", sr=2.0, seed=123),
    "alpha_1.5_sr1": dict(scene="thin", edit="alpha_1.5"),
    "alpha_1.5_sr2": dict(scene="thin", edit="alpha_1.5", sr=2.0),
    "colours": dict(scene="thin", edit="colours"),
}
BOTH_ENTRIES = ("wg3_17x19", "wide_33x9", "one_ray", "strides_f32", "strides_f16", "alpha_1.5_sr2")
EDGE.update({k + "_cam": dict(EDGE[k], posed=False) for k in BOTH_ENTRIES})
# (the look_from entry with the camera closer: the box fills the image, its corner in the last workgroup too)
EDGE["wg3_17x19_close_cam"] = dict(EDGE["wg3_17x19_cam"], look_from=(1.54, 0.77, 1.19))


def _edge(key, entry="pose"):
    return _case(**EDGE[key + ("_cam" if entry == "cam" else "")])


def _cam_refs(ref, ref32):
    """The look_from columns of the two references, as camgrad_gpu's rule reads them."""
    return tuple({"n": r["n"], "dcam_ray": r["dpose_ray"][..., :3]} for r in (ref, ref32))


def _columns(entry):
    return COLUMNS if entry == "pose" else K.LOOK_FROM


def _rule(entry, ray, total, ref, ref32, mask, what):
    if entry == "pose":
        PG.pose_rule(ray, total, ref, ref32, mask, what)
    else:
        K.d8_rule(ray, total, *_cam_refs(ref, ref32), mask, what)


def _good(entry, ref, ref32, keep, what=None):
    """The keep mask of the second pass: the rays on which the two references agree (D16: no lighting, no kinks)."""
    if entry == "pose":
        return PG.well_conditioned(ref, ref32, keep, what, lit=False)
    cref, cref32 = _cam_refs(ref, ref32)
    return K.well_conditioned(cref, cref32, keep, what=what, lit=False)


def _run(case, entry, keep, vol=None, upstream=None):
    """One launch of one view on the reference's ray buffers -> per-ray (W, H, k), total (k,), the mask of the compared rays."""
    inp, ref, _ = case
    vol = TG._volume(inp["vol"]) if vol is None else vol
    ray, total, mask, _ = TG._launch(vol, [inp], [ref], [keep], int(inp["jitter_seed"]), int(inp["view"]), upstream, entry)
    return ray[0], total[0], mask[0]


def _sum_share(entry, ray, total, what):
    """The total against its rays' sum, per camera tensor: within 1e-5 of the sum of the rays' magnitudes, the bound D8's rule
    states (test_image_shapes_match_the_f64_reference_and_sum_up spells it out too). -> the largest share."""
    worst = 0.0
    for name, sl in _columns(entry):
        mag = np.abs(ray[..., sl]).sum()
        diff = np.abs(total[sl] - ray[..., sl].sum((0, 1))).max()
        assert diff <= 1e-5 * mag, (what, name, diff, mag)
        worst = max(worst, diff / mag if mag > 0 else 0.0)
    print("sumshare", what, "%.3g" % worst)
    return worst


def _nonzero(entry, ray, mask, what, columns=None):
    """Every camera tensor has a gradient among the compared rays."""
    for name, sl in (columns or _columns(entry)):
        assert np.abs(ray[mask][:, sl]).max() > 0, (what, name)


def _both(case, entry="pose", vol=None, what=None, keep=None, refs=None, upstream=None, nonzero=None):
    """Both passes of one view: the rule over the kept rays, then over the well-conditioned ones alone. refs: (ref, ref32) for
    the rule where they are not the case's own (the NaN pixels' rows taken out). -> the first pass's (ray, total, mask)."""
    inp, ref, ref32 = case
    rref, rref32 = (ref, ref32) if refs is None else refs
    keep = PG.keep(ref, ref32) if keep is None else keep
    first = _run(case, entry, keep, vol, upstream)
    _rule(entry, first[0], first[1], rref, rref32, first[2], what)
    _nonzero(entry, first[0], first[2], what, nonzero)
    _sum_share(entry, first[0], first[1], what)
    good = _good(entry, rref, rref32, keep, what)
    ray, total, mask = _run(case, entry, good, vol, upstream)
    _rule(entry, ray, total, rref, rref32, mask, (what, "conditioned"))
    _nonzero(entry, ray, mask, (what, "conditioned"), nonzero)
    _sum_share(entry, ray, total, (what, "conditioned"))
    return first


def _early(ref, S=512):
    return ((ref["steps"] < np.minimum(ref["n"], S)) & (ref["n"] > 1)).sum()


# ---- 1. more than one workgroup, and several views at once -------------------------------------------------------------------------

def _tiles(WH):
    return -(-WH[0] // 8) * -(-WH[1] // 8)


@pytest.mark.parametrize("key,entry", [("wg3_17x19", "pose"), ("wg3_17x19", "cam"), ("wg3_17x19_close", "cam")])
def test_three_workgroups_the_last_with_one_live_wave(hiplib, key, entry):
    """17 x 19: 3 x 3 tiles of 8 x 8, a wave each, four to a workgroup -- three workgroups add to d_cam[view] and the last has
    one live wave; the total must be its rays' sum and the float64 reference's. Under the default pose of the look_from entry
    the box misses the image's corner -- the last workgroup's three rays add zeros like its idle waves -- so that entry runs
    a second time from 0.7 of the distance, where every ray of the image meets the box."""
    inp, ref, ref32 = _edge(key, entry)
    WH = ref["n"].shape
    assert _tiles(WH) == 9 and -(-_tiles(WH) // 4) == 3 and _tiles(WH) % 4 == 1
    assert (ref["n"] > 1).sum() > 200 and _early(ref) > 40
    ray, total, mask = _both((inp, ref, ref32), entry, what=(key, entry))
    for _, sl in _columns(entry):   # the rule's own bound, spelt out
        assert np.abs(total[sl] - ray[..., sl].sum((0, 1))).max() <= 1e-5 * np.abs(ray[..., sl]).sum()
    # rays of every workgroup are among the compared ones: a tile's wave is (i / 8) * tiles_j + j / 8 (dr_tile.h: tile_pixel)
    tile = 3 * (np.arange(WH[0])[:, None] // 8) + (np.arange(WH[1])[None, :] // 8)
    groups = {int(t) // 4 for t in np.unique(tile[mask])}
    corner_misses = (key, entry) == ("wg3_17x19", "cam")
    assert groups == ({0, 1} if corner_misses else {0, 1, 2})
    assert bool((ref["n"][16:, 16:] > 1).any()) == (not corner_misses)


@pytest.mark.parametrize("entry", ["pose", "cam"])
def test_a_wide_short_image_with_idle_tiles(hiplib, entry):
    """33 x 9: 5 x 2 tiles in three workgroups, most of them off the object (their lanes add zeros)."""
    key = "wide_33x9"
    inp, ref, ref32 = _edge(key, entry)
    assert _tiles(ref["n"].shape) == 10
    live = ref["n"] > 1
    assert 40 < live.sum() < 0.4 * live.size
    tiles_hit = {(i // 8, j // 8) for i, j in zip(*np.nonzero(live))}
    assert len(tiles_hit) < 10   # whole tiles without a ray that meets the box
    _both((inp, ref, ref32), entry, what=(key, entry))


@pytest.mark.parametrize("entry", ["pose", "cam"])
def test_an_image_of_one_ray(hiplib, entry):
    """1 x 1: one live lane in the launch. Its ray is the viewing direction itself, which does not depend on up or on the
    fov: those two gradients are exactly 0 in the reference, and the other tensors' are not."""
    key = "one_ray"
    inp, ref, ref32 = _edge(key, entry)
    assert ref["n"].shape == (1, 1) and ref["n"][0, 0] > 1 and _early(ref) == 1
    assert (ref["dpose_ray"][..., 6:] == 0).all()
    _both((inp, ref, ref32), entry, what=(key, entry), nonzero=_columns(entry)[:2])


VIEW_BASE, VIEW_SEED = 5, 90210
VIEW_POSES = [dict(),
              dict(look_from=(-1.9, 1.2, 1.6), look_at=(0.1, 0.15, -0.1), up=(-0.2, 1.0, 0.1), fov_rad=math.radians(28.0)),
              dict(look_from=(0.8, -1.4, -2.1), look_at=(-0.1, 0.05, 0.1), up=(0.1, 1.0, 0.3), fov_rad=math.radians(31.0))]


@functools.lru_cache(maxsize=None)
def _three_views(batched_vol, entry="pose"):
    """(inputs, float64 references, float32 references) of the three views at 17 x 19. batched_vol: every view reads a
    volume of its own (the scene's, and two mirror images of it), and so does its reference. entry "cam": the three
    look_from under the default pose."""
    flips = [lambda v: v, lambda v: v[:, ::-1].copy(), lambda v: v[:, :, ::-1].copy()]
    out = []
    for v, pose in enumerate(VIEW_POSES):
        kw = dict(SCENES["opaque"], WH=(17, 19), seed=VIEW_SEED, view=VIEW_BASE + v)
        kw.update(dict(SC.POSED, **pose) if entry == "pose" else {k: pose[k] for k in ("look_from",) if k in pose})
        inp = SC.make(**kw)
        if batched_vol:
            inp["vol"] = flips[v](inp["vol"])
        out.append((inp, RP.run_case(inp), RP.run_case(inp, dtype=torch.float32)))
    return tuple(zip(*out))


@pytest.mark.parametrize("entry", ["pose", "cam"])
@pytest.mark.parametrize("batched_vol", [False, True], ids=["shared_volume", "batched_volume"])
def test_three_views_of_three_workgroups_each(hiplib, batched_vol, entry):
    """blockIdx.y with more than one workgroup per view, view_base = 5 with jitter, a pose and a fov per view (the look_from
    entry: a camera per view): each view's per-ray gradients and its row of d_pose against that view's own float64 reference.
    batched_vol: the batch is every other item of six, the items between them NaN -- a wrong view stride reads those."""
    inps, refs_, refs32 = _three_views(batched_vol, entry)
    assert [int(i["view"]) for i in inps] == [VIEW_BASE + v for v in range(3)] and int(inps[0]["jitter_seed"]) == VIEW_SEED
    assert all(("look_at" in i) == (entry == "pose") for i in inps)
    for r in refs_:
        assert (r["n"] > 1).sum() > (200 if entry == "pose" else 100)
    if batched_vol:
        six = torch.full((6, *inps[0]["vol"].shape), NAN, device=torch.device("cuda"))
        vol = six[::2]
        vol.copy_(dev(np.stack([i["vol"] for i in inps])))
        assert vol.shape[0] == 3 and not vol.is_contiguous() and vol.stride(0) == 2 * six.stride(0)
        assert all(not np.array_equal(inps[a]["vol"], inps[b]["vol"]) for a in range(3) for b in range(a))
    else:
        vol = dev(inps[0]["vol"])
        assert all(np.array_equal(inps[0]["vol"], i["vol"]) for i in inps)
    what = ("three views", "batched" if batched_vol else "shared", entry)
    keeps = [PG.keep(a, b) for a, b in zip(refs_, refs32)]
    ray, total, masks, _ = TG._launch(vol, inps, refs_, keeps, VIEW_SEED, VIEW_BASE, entry=entry)
    for v in range(3):
        _rule(entry, ray[v], total[v], refs_[v], refs32[v], masks[v], what + (v,))
        _nonzero(entry, ray[v], masks[v], what + (v,))
        _sum_share(entry, ray[v], total[v], what + (v,))
    for got in (ray, total):   # no view got another view's row, camera, pose, fov or volume
        big = np.abs(got).max()
        assert all(np.abs(got[a] - got[b]).max() > 1e-3 * big for a in range(3) for b in range(a))
    goods = [_good(entry, refs_[v], refs32[v], keeps[v], what + (v,)) for v in range(3)]
    ray, total, masks, _ = TG._launch(vol, inps, refs_, goods, VIEW_SEED, VIEW_BASE, entry=entry)
    for v in range(3):
        _rule(entry, ray[v], total[v], refs_[v], refs32[v], masks[v], what + (v, "conditioned"))
        _sum_share(entry, ray[v], total[v], what + (v, "conditioned"))


# ---- 2. the scalar-load instances on real strides ----------------------------------------------------------------------------------

def _vec_ok(vol):
    """rgba_vec_ok (csrc/march_rgba.hip) restated: a voxel's four channels are one aligned load."""
    sc, sx, sy, sz = vol.stride()[-4:]
    return sc == 1 and sx % 4 == 0 and sy % 4 == 0 and sz % 4 == 0 and vol.data_ptr() % (4 * vol.element_size()) == 0


def _non_dense_planar(v):
    VX, VY, VZ = v.shape[-3:]
    big = torch.full((4, VX + 4, VY + 3, VZ + 5), NAN, device=v.device, dtype=v.dtype)   # (what lies around the view is never read)
    view = big[:, 2:2 + VX, 1:1 + VY, 3:3 + VZ]
    assert view.stride(0) > 1 and view.stride(1) != VY * VZ
    return view


def _channel_stride_one_voxel_stride_five(v):
    VX, VY, VZ = v.shape[-3:]
    view = torch.full((VX, VY, VZ, 5), NAN, device=v.device, dtype=v.dtype)[..., 1:5].permute(3, 0, 1, 2)
    assert view.stride() == (1, 5 * VY * VZ, 5 * VZ, 5)
    return view


def _interleaved_off_its_alignment(v):
    VX, VY, VZ = v.shape[-3:]
    count = 4 * VX * VY * VZ
    buf = torch.full((count + 4,), NAN, device=v.device, dtype=v.dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + count].view(VX, VY, VZ, 4).permute(3, 0, 1, 2)
    assert view.stride() == (1, 4 * VY * VZ, 4 * VZ, 4) and view.data_ptr() % (4 * view.element_size()) != 0
    return view


def _the_modules_permuted_view(v):
    from differender_amd import _layout as L
    VX, VY, VZ = v.shape[-3:]   # (W, D, H) of the user's (D, H, W)
    user = torch.full((4, VY, VZ, VX), NAN, device=v.device, dtype=v.dtype)
    view = L.field_view_rgba(user)
    assert user.is_contiguous() and view.stride() == (VX * VY * VZ, 1, VZ * VX, VX)
    return view


STRIDED = {"non_dense_planar": _non_dense_planar, "channel_stride_1_voxel_stride_5": _channel_stride_one_voxel_stride_five,
           "interleaved_off_alignment": _interleaved_off_its_alignment, "permuted_DHW": _the_modules_permuted_view}


@pytest.mark.parametrize("entry", ["pose", "cam"])
@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("layout", sorted(STRIDED))
def test_scalar_load_instances_on_strided_volumes(hiplib, layout, vdt, entry):
    """The VEC = false instances (tri_sample4_grad's eight corner fetches of four loads each) on views that are not dense
    planar, NaN around them: per ray the bits of the VEC instance on rgba.interleaved() of the same values (D16: the same
    arithmetic in the same order), all finite, and the float64 reference's by the rule in both passes."""
    from differender_amd.rgba import interleaved
    key = "strides_f16" if vdt == torch.float16 else "strides_f32"
    case = _edge(key, entry)
    inp, ref, ref32 = case
    dense = dev(inp["vol"]).to(vdt)
    assert np.array_equal(dense.double().cpu().numpy(), inp["vol"])   # the reference ran on what the kernel reads
    view = STRIDED[layout](dense)
    view.copy_(dense)
    assert view.shape == dense.shape and not view.is_contiguous() and not _vec_ok(view)
    fast = interleaved(dense)
    assert _vec_ok(fast)
    what = (layout, str(vdt)[6:], entry)
    ray, total, mask = _both(case, entry, view, what)
    assert np.isfinite(ray).all() and np.isfinite(total).all()
    vray, vtotal, vmask = _run(case, entry, PG.keep(ref, ref32), fast)
    assert np.array_equal(mask, vmask) and mask.sum() > 20
    assert np.array_equal(ray, vray) and np.abs(ray).max() > 0
    assert np.array_equal(total, vtotal)   # one workgroup: the same sums in the same order


# ---- 3. rates, clips and volume shapes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["sr0.6", "sr1.3", "sr4", "sr8"])
def test_other_sampling_rates(hiplib, key):
    """0.6: inv_sr > 1 (pow_spec, the derivative's exponent positive); 1.3: pow_spec; 4 and 8: nested square roots."""
    inp, ref, ref32 = _edge(key)
    sr = float(inp["sr"])
    assert sr == float(key[2:]) and (ref["n"] > 1).sum() > 80
    if EDGE[key]["scene"] == "opaque":
        assert _early(ref) >= 10
    _both((inp, ref, ref32), what=key)


@pytest.mark.parametrize("S", [1, 2])
def test_max_samples_one_and_two(hiplib, S):
    """S = 1: one sample at t0 (f = 0: all of G_s goes to s0); S = 2: the second sits at f = 1 / (n - 1) of the unclipped n."""
    inp, ref, ref32 = _edge("clip_S%d" % S)
    live = ref["n"] > 1
    assert int(inp["max_samples"]) == S and live.sum() > 40
    # every live ray is clipped (one ray of the scene plans exactly two samples: it marches both, like the clipped ones)
    assert (ref["steps"][live] == S).all() and (ref["n"][live] >= S).all() and (ref["n"][live] > S).sum() >= live.sum() - 1
    _both((inp, ref, ref32), what=("clip", S))


def test_slope_scales_of_a_stretched_volume(hiplib):
    """(20, 6, 11): scx : scy : scz = 19 : 5 : 10 -- slope scales handed to the wrong axes are off by factors of 2 to 4."""
    inp, ref, ref32 = _edge("slopes_20x6x11")
    assert [s - 1 for s in inp["vol"].shape[-3:]] == [19, 5, 10] and (ref["n"] > 1).sum() > 80
    _both((inp, ref, ref32), what="20x6x11")


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_a_volume_axis_of_two_voxels(hiplib, axis, layout):
    """One cell along the axis: at its far face the high index is clamped onto the low one (equal corners, a zero slope)."""
    case = _edge("two_voxels_" + axis)
    inp, ref, ref32 = case
    assert inp["vol"].shape[1 + "xyz".index(axis)] == 2 and sorted(inp["vol"].shape[-3:])[0] == 2 and (ref["n"] > 1).sum() > 80
    vol = TG._volume(inp["vol"], layout)
    assert _vec_ok(vol) == (layout == "interleaved")
    _both(case, vol=vol, what=("two voxels", axis, layout))


def test_the_camera_inside_the_box_at_rate_two_with_jitter(hiplib):
    inp, ref, ref32 = _edge("inside_sr2_jit")
    assert int(inp["jitter_seed"]) == 123 and float(inp["sr"]) == 2.0
    assert (ref["entry"] < 0).all() and (ref["n"] > 1).all() and ref["n"].size == 81
    _both((inp, ref, ref32), what="inside sr 2 jitter")


# ---- 4. values ---------------------------------------------------------------------------------------------------------------------

def _nan_pixels(ref, ref32):
    nan = np.isnan(ref["rgba"]).any(-1)
    assert np.array_equal(nan, np.isnan(ref32["rgba"]).any(-1))
    return nan


def _without_rows(ref, rows):
    """The reference with the per-ray gradients of `rows` (NaN there) set to 0, as the rule's arithmetic needs them."""
    return dict(ref, dpose_ray=np.where(rows[..., None], 0.0, ref["dpose_ray"]))


def _alpha_sr2(entry):
    """-> (case, NaN pixels, keep without them, references without their rows)"""
    case = _edge("alpha_1.5_sr2", entry)
    _, ref, ref32 = case
    nan = _nan_pixels(ref, ref32)
    return case, nan, PG.keep(ref, ref32) & ~nan, (_without_rows(ref, nan), _without_rows(ref32, nan))


@pytest.mark.parametrize("entry", ["pose", "cam"])
def test_a_nan_pixel_contributes_exactly_zero(hiplib, entry):
    """D16: "a ray whose ... pixel is NaN (the pixel an alpha > 1 produces at a rate != 1 is one) contributes exactly 0". A
    block of alpha 1.5 at rate 2: op = 1 - sqrt(1 - a) is NaN where a sample's a > 1, the pixel is NaN and the ray ends there.
    Those rays get their upstream gradient like the others; their per-ray rows are exactly 0, the totals finite, and every
    other ray is held to the rule in both passes."""
    from differender_amd import functional as F
    case, nan, keep, refs = _alpha_sr2(entry)
    inp, ref, ref32 = case
    assert nan.sum() >= 3 and np.isnan(ref["dpose_ray"][nan]).any()
    assert (ref["steps"][nan] < ref["n"][nan]).all()   # they stop early
    # the kernels' own forward has those pixels NaN, and no others
    one = lambda k, dt=torch.float32: dev(np.asarray(ref[k])[None], dt)
    e, x, r, n = one("entry"), one("exit"), one("rays"), one("n", torch.int32)
    out, _ = F.march_rgba_fwd(dev(inp["vol"]), dev(inp["look_from"][None]), e, x, r, n, int(inp["max_samples"]), float(inp["sr"]))
    assert np.array_equal(np.isnan(out[0].cpu().numpy()).any(-1), nan)

    def hand_in(g):
        g = g.clone()
        g[0][torch.from_numpy(nan).to(g.device)] = dev(inp["grad_out"][nan])
        return g

    what = ("alpha 1.5 sr 2", entry)
    ray, total, mask = _both(case, entry, what=what, keep=keep, refs=refs, upstream=hand_in)
    assert not mask[nan].any() and (ray[nan] == 0).all()
    assert np.isfinite(ray).all() and np.isfinite(total).all()
    assert mask.sum() > 0.8 * ((ref["n"] > 1).sum() - nan.sum())


def test_an_alpha_above_one_at_rate_one(hiplib):
    """At rate 1 op = a: nothing is NaN, pixels exceed 1, every ray is held to the rule."""
    inp, ref, ref32 = _edge("alpha_1.5_sr1")
    assert np.isfinite(ref["rgba"]).all() and np.isfinite(ref["dpose_ray"]).all()
    assert ref["rgba"][..., 3].max() > 1.0 and float(inp["vol"][3].max()) == 1.5
    _both((inp, ref, ref32), what="alpha 1.5 sr 1")


def test_colours_outside_zero_one(hiplib):
    inp, ref, ref32 = _edge("colours")
    assert inp["vol"][:3].min() < -0.5 and inp["vol"][:3].max() > 1.5 and 0 <= inp["vol"][3].min() and inp["vol"][3].max() <= 1
    _both((inp, ref, ref32), what="colours in [-1, 2]")


# ---- 5. RaycasterRGBA(camera_grad=True) with jitter against the reference ----------------------------------------------------------

MODULE_K, MODULE_WH = 2468, (20, 16)
MODULE_CAMS = [(-1.3, 0.9, 2.0), (2.3, 0.5, -0.9)]
MODULE_KINDS = ("batched_look_from", "batched_volume", "fixed_camera")


def _module_seed():
    """The jitter seed the module's forward draws after torch.manual_seed(MODULE_K) (the caller's generator is left alone)."""
    from differender_amd import functional as F
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(MODULE_K)
        return F.new_jitter_seed()


def _module_fov_rad():
    """SC.POSED's fov as the module hands it to the kernels: degrees in float32, converted in float32."""
    deg = torch.tensor(math.degrees(SC.POSED["fov_rad"]), dtype=torch.float32)
    return deg, float(torch.deg2rad(deg))


@functools.lru_cache(maxsize=None)
def _module_case(kind):
    """Per view (inputs, float64 reference, float32 reference) of the module's own launch: its seed, view = v, rate 1, the thin
    volume at 20 x 16, an upstream gradient per view."""
    seed = _module_seed()
    assert seed != 0
    views = []
    for v in range(1 if kind == "fixed_camera" else 2):
        kw = dict(opaque=False, sr=1.0, S=512, WH=MODULE_WH, seed=seed, view=v)
        if kind != "fixed_camera":
            kw.update(SC.POSED, fov_rad=_module_fov_rad()[1])
        if kind == "batched_look_from":
            kw.update(look_from=MODULE_CAMS[v])
        inp = SC.make(**kw)
        inp["grad_out"] = SC.F32(np.random.RandomState(23 + v).standard_normal((*MODULE_WH, 4)))
        if kind == "batched_volume" and v == 1:
            inp["vol"] = inp["vol"][:, ::-1].copy()
        views.append((inp, RP.run_case(inp), RP.run_case(inp, dtype=torch.float32)))
    return views


@pytest.mark.parametrize("kind", MODULE_KINDS)
def test_rgba_module_with_jitter_matches_the_f64_reference(hiplib, kind):
    """test_raycaster_with_jitter_matches_the_f64_reference for RaycasterRGBA(camera_grad=True, jitter=True): the backward must
    be handed the forward's jitter seed and view base (the grad t0 term). .grad of every camera tensor against the float64
    reference's totals; fov.grad is per degree, a shared tensor's gradient the sum over the views."""
    from differender_amd import functional as F
    from differender_amd.rgba import RaycasterRGBA
    views = _module_case(kind)
    seed = _module_seed()
    V, inp0 = len(views), views[0][0]
    VX, VY, VZ = inp0["vol"].shape[-3:]
    S, sr = int(inp0["max_samples"]), float(inp0["sr"])
    rc = RaycasterRGBA((VY, VZ, VX), MODULE_WH, sampling_rate=sr, jitter=True, max_samples=S, camera_grad=True)
    user_vol = lambda a: dev(a).permute(0, 2, 3, 1).contiguous()   # the kernels' (4, W, D, H) as the user's (4, D, H, W)
    if kind == "batched_volume":
        vol = torch.stack([user_vol(i["vol"]) for i, _, _ in views])
    else:
        vol = user_vol(inp0["vol"])
    lf0 = dev(np.stack([i["look_from"] for i, _, _ in views])) if kind == "batched_look_from" else dev(inp0["look_from"])
    fixed = kind == "fixed_camera"
    fov_deg, fov_rad = _module_fov_rad()
    firsts = [lf0] if fixed else [lf0, dev(inp0["look_at"]), dev(inp0["up"]), fov_deg.to(lf0.device)]
    if not fixed:
        assert float(inp0["fov_rad"]) == fov_rad

    # the rays the module will march (its own float32 ray setup, the replayed seed): the compared rays are those whose sample
    # count and live samples are the reference's, in float32 and float64 alike
    if fixed:
        batched, vol_in, lf_in = rc._determine_batch(vol, lf0)
        cam = lf_in.reshape(-1, 3).contiguous()
        e, x, r, n = F.ray_setup(cam, MODULE_WH, vol_in.shape[-3:], sr, jitter_seed=seed)
    else:
        batched, vol_in, lf_in, (la, up, fov) = rc._determine_batch(vol, lf0, tuple(firsts[1:]))
        pose = F.pack_pose(lf_in.reshape(-1, 3).expand(V, 3), la, up)
        cam = pose[:, :3].contiguous()
        e, x, r, n = F.ray_setup_pose(pose, MODULE_WH, vol_in.shape[-3:], sr, jitter_seed=seed, fov_v=torch.deg2rad(fov).contiguous())
    assert bool(batched) == (V == 2) and tuple(vol_in.shape[-3:]) == (VX, VY, VZ)
    steps = F.march_rgba_fwd(vol_in, cam, e, x, r, n, S, sr)[1]
    n, steps = n.cpu().numpy(), steps.cpu().numpy()
    masks = [(n[v] == ref["n"]) & (steps[v] == ref["steps"]) & PG.keep(ref, ref32) & (ref["n"] > 1)
             for v, (_, ref, ref32) in enumerate(views)]
    for m, (_, ref, _) in zip(masks, views):
        assert m.sum() > 0.8 * (ref["n"] > 1).sum() and (ref["n"] > 1).sum() > 100
    g = dev(np.stack([i["grad_out"] * m[..., None] for m, (i, _, _) in zip(masks, views)]))   # (V, W, H, 4)
    w = g.permute(0, 3, 2, 1).flip(-2)                                                          # (V, 4, H, W)
    assert torch.equal(w.flip(-2).permute(0, 3, 2, 1), g)
    if not batched:
        w = w[0]

    leaves = [t.clone().requires_grad_(True) for t in firsts]
    torch.manual_seed(MODULE_K)
    img = rc(vol, leaves[0]) if fixed else rc(vol, leaves[0], look_at=leaves[1], up=leaves[2], fov=leaves[3])
    assert img.shape == w.shape
    (img * w).sum().backward()
    for leaf, first in zip(leaves, firsts):
        assert leaf.grad is not None and leaf.grad.shape == first.shape and leaf.grad.dtype == first.dtype
        assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    grads = [leaf.grad.double().cpu().numpy() for leaf in leaves]

    want = np.concatenate([ref["dpose_ray"] for _, ref, _ in views], 0)       # the views' rays, one after the other
    want32 = np.concatenate([ref32["dpose_ray"] for _, _, ref32 in views], 0)
    mask = np.concatenate(masks, 0)
    if fixed:
        K.d8_total_rule(grads[0], want[..., :3], want32[..., :3], mask, kind)
        return
    if kind == "batched_look_from":   # look_from per view; look_at, up and fov are shared: the sum over the views
        for v, (_, ref, ref32) in enumerate(views):
            K.d8_total_rule(grads[0][v], ref["dpose_ray"][..., :3], ref32["dpose_ray"][..., :3], masks[v], (kind, v))
        assert np.abs(grads[0][0] - grads[0][1]).max() > 1e-3 * np.abs(grads[0]).max()
    total = np.concatenate([grads[0].reshape(-1, 3).sum(0), grads[1], grads[2], grads[3].reshape(1) * (180.0 / math.pi)])
    PG.pose_total_rule(total, want, want32, mask, kind)


# ---- 6. what the conditioned pass is fed, for tests/test_rgba_camera.py to hold to its conditions without a GPU --------------------

def _entries(cases, keep=None):
    return [(ref, ref32, PG.keep(ref, ref32) if keep is None else keep, None) for _, ref, ref32 in cases]


def _alpha_sr2_entries(entry):
    _, _, keep, (ref, ref32) = _alpha_sr2(entry)
    return [(ref, ref32, keep, None)]


# id -> a function that returns [(float64 reference, float32 reference, keep mask, None)], one entry per view
CONDITIONED = {key: (lambda k=key: _entries([_case(**EDGE[k])])) for key in sorted(EDGE) if not key.startswith("alpha_1.5_sr2")}
CONDITIONED.update({"alpha_1.5_sr2": lambda: _alpha_sr2_entries("pose"), "alpha_1.5_sr2_cam": lambda: _alpha_sr2_entries("cam"),
                    "three_views_shared": lambda: _entries(zip(*_three_views(False))),
                    "three_views_batched": lambda: _entries(zip(*_three_views(True))),
                    "three_views_shared_cam": lambda: _entries(zip(*_three_views(False, "cam"))),
                    "three_views_batched_cam": lambda: _entries(zip(*_three_views(True, "cam")))})
CONDITIONED.update({"module_" + kind: (lambda k=kind: _entries(_module_case(k))) for kind in MODULE_KINDS})
