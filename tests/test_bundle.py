"""Ray bundles, DESIGN.md D19, without a GPU: the C ABI and its argument checks, the two torch helpers against the float64
pose reference, the new reference (tests/bundle_reference.py) pinned to that one through torch autograd of pinhole_rays, the
conditions every bundle of the GPU files owes the conditioned pass (and, for the edge bundles, that each edge changes the
gradient), and the module's argument checks."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import bundle_reference as BR  # noqa: E402
import camgrad_gpu as K  # noqa: E402
import pose_gpu as PG  # noqa: E402
import pose_reference as PR  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_bundle_setup", "dr_march_bundle_fwd", "dr_march_bundle_bwd", "dr_march_bundle_bwd_rays")
POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
CAM = (-1.3, 0.9, 2.0)
INF = float("inf")


# --- 1. the C ABI -----------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    assert N.lib().dr_abi_version() == 9   # the entries are additive
    for name in ENTRIES:
        params = _header_params(name)
        assert hasattr(raw, name)
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
                    ctypes.c_float if p.startswith("float") else ctypes.c_double if p.startswith("double") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)
    # the three marches share their head, up to sampling_rate
    fwd, bwd, rays = (_header_params(n) for n in ENTRIES[1:])
    head = fwd[:fwd.index("float sampling_rate") + 1]
    assert bwd[:len(head)] == head and rays[:len(head)] == head
    assert all(ps[-1] == "void *stream" for ps in (fwd, bwd, rays))


def _setup_args(b, **kw):
    a = dict(origins=b.p[0], dirs=b.p[1], N=16, VX=8, VY=8, VZ=8, sr=1.0, t_near=-INF, seed=0, base=0, entry=b.p[3], exit=b.p[4],
             n=b.p[6], stream=None)
    a.update(kw)
    return list(a.values())


def _args(b, which, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, tf=b.p[1], R=8, origins=b.p[2], dirs=b.p[5], entry=b.p[3],
             exit=b.p[4], n=b.p[6], N=16, S=64, sr=1.0)
    if which == "fwd":
        a.update(out=b.p[7], steps=None)
    elif which == "bwd":
        a.update(go=b.p[7], out=b.p[7], dvol=None, dsx=0, dsy=0, dsz=0, dtf=None)
    else:
        a.update(steps=b.p[6], t_near=-INF, seed=0, base=0, go=b.p[7], out=b.p[7], d_o=b.p[0], d_d=b.p[1])
    a.update(stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null tf": dict(tf=None), "null origins": dict(origins=None), "null dirs": dict(dirs=None),
    "null entry": dict(entry=None), "null exit": dict(exit=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7),
    "N 0": dict(N=0), "N -5": dict(N=-5), "N 2^31": dict(N=2 ** 31), "N 2^40": dict(N=2 ** 40), "VX 1": dict(VX=1),
    "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0), "R 0": dict(R=0), "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-1),
    "sampling rate 0": dict(sr=0.0), "sampling rate nan": dict(sr=float("nan")),
}
SETUP_KEYS = ("origins", "dirs", "entry", "exit", "n", "N", "VX", "VY", "VZ", "sr")


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    bad = INVALID[case]
    assert hiplib.dr_march_bundle_fwd(*_args(b, "fwd", **bad)) == -1
    assert hiplib.dr_march_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], dtf=b.p[1], **bad)) == -1
    assert hiplib.dr_march_bundle_bwd(*_args(b, "bwd", **bad)) == -1   # (checked before "nothing requested")
    assert hiplib.dr_march_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1
    if set(bad) <= set(SETUP_KEYS):
        assert hiplib.dr_bundle_setup(*_setup_args(b, **bad)) == -1


def test_nan_t_near_missing_outputs_and_nothing_requested(hiplib):
    b = _Bufs()
    assert hiplib.dr_bundle_setup(*_setup_args(b, t_near=float("nan"))) == -1
    assert hiplib.dr_march_bundle_bwd_rays(*_args(b, "rays", t_near=float("nan"))) == -1
    assert hiplib.dr_march_bundle_fwd(*_args(b, "fwd", out=None)) == -1
    assert hiplib.dr_march_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], go=None)) == -1
    assert hiplib.dr_march_bundle_bwd(*_args(b, "bwd", dtf=b.p[1], out=None)) == -1
    assert hiplib.dr_march_bundle_bwd(*_args(b, "bwd")) == 0   # d_vol == NULL && d_tf == NULL: nothing to do, no HIP call
    for bad in (dict(steps=None), dict(go=None), dict(out=None), dict(d_o=None), dict(d_d=None)):
        assert hiplib.dr_march_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1, bad


# --- 2. the helpers, in float64 ---------------------------------------------------------------------------------------------------

def kernel_order(img):
    """(H, W, ...) in the user image's orientation -> (W*H, ...) in the kernels' [W][H] order (image row h is column H-1-h)."""
    return torch.flip(img, (0,)).transpose(0, 1).reshape(img.shape[0] * img.shape[1], *img.shape[2:])


@pytest.mark.parametrize("pose", [POSE, {}], ids=["posed", "fixed"])
@pytest.mark.parametrize("WH", [(16, 16), (14, 9)], ids=str)
def test_pinhole_rays_are_the_pose_reference_s(pose, WH):
    from differender_amd.bundle import pinhole_rays
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    lf, la, up = T(CAM), T(pose.get("look_at", PR.ORIGIN)), T(pose.get("up", PR.UP_Y))
    fov_rad = pose.get("fov_rad", math.radians(PR.FOV_DEG))
    _, _, want, _ = PR.ray_setup(lf, la, up, fov_rad, *WH, (16, 16, 16), 1.0)
    o, d = pinhole_rays(lf, la, up, math.degrees(fov_rad), WH)
    assert o.shape == d.shape == (WH[1], WH[0], 3) and o.dtype == torch.float64
    assert float((kernel_order(d) - want).abs().max()) <= 1e-12
    assert bool((o == lf).all())


def test_orthographic_rays_are_parallel_coplanar_and_evenly_spaced():
    from differender_amd.bundle import orthographic_rays
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    lf, la, up, extent, (W, H) = T(CAM), T(POSE["look_at"]), T(POSE["up"]), 2.4, (10, 12)
    o, d = orthographic_rays(lf, la, up, extent, (W, H))
    assert o.shape == d.shape == (H, W, 3)
    view = (la - lf) / (la - lf).norm()
    assert float((d - view).abs().max()) <= 1e-15 and bool((d == d[0, 0]).all())
    assert float(((o - lf) @ view).abs().max()) <= 1e-12   # in the plane through look_from
    down, across = o[1:] - o[:-1], o[:, 1:] - o[:, :-1]
    assert float((down.norm(dim=-1) - extent / H).abs().max()) <= 1e-12
    assert float((across.norm(dim=-1) - extent / H).abs().max()) <= 1e-12   # square pixels: the width is extent W / H
    assert float((down * across[:1, :1]).sum(-1).abs().max()) <= 1e-12
    centre = o.reshape(-1, 3).mean(0)
    assert float((centre - lf).abs().max()) <= 1e-12
    # image rows run downwards: against up
    assert float((down[0, 0] * up).sum()) < 0


# --- 3. the new reference pinned to the old one ---------------------------------------------------------------------------------

def test_bundle_reference_on_pinhole_rays_is_the_pose_reference():
    """bundle_reference.run on pinhole_rays' output, its d_origin and d_dir pushed through torch autograd of pinhole_rays, is
    pose_reference.run_case: dpose_ray to 1e-9 of its scale, rgba exactly."""
    from differender_amd.bundle import pinhole_rays
    inp = PG.inputs("a_orbit_sr1", look_from=np.array(CAM), look_at=POSE["look_at"], up=POSE["up"])
    want = PR.run_case(inp)
    W, H = want["n"].shape
    theta = torch.from_numpy(np.concatenate([inp["look_from"], inp["look_at"], inp["up"], [math.radians(PR.FOV_DEG)]]))

    def rays(th):
        o, d = pinhole_rays(th[0:3], th[3:6], th[6:9], th[9] * (180.0 / math.pi), (W, H))
        return torch.cat([kernel_order(o), kernel_order(d)], -1)

    od = rays(theta)
    got = BR.run(dict(vol=inp["vol"], tf=inp["tf"], origins=od[:, :3].numpy(), dirs=od[:, 3:].numpy(),
                      grad_out=inp["grad_out"].reshape(-1, 4), sr=inp["sr"], max_samples=inp["max_samples"]))
    assert (got["n"].reshape(W, H) == want["n"]).all() and (got["steps"].reshape(W, H) == want["steps"]).all()
    assert (got["n"] > 1).sum() > W * H // 2   # (the box fills most of this view)
    assert (got["rgba"].reshape(W, H, 4) == want["rgba"]).all()
    J = torch.autograd.functional.jacobian(rays, theta, vectorize=True)   # (P, 6, 10)
    dpose = np.einsum("pk,pkt->pt", got["dray"].reshape(-1, 6), J.numpy()).reshape(W, H, 10)
    for name, sl in PG.COLUMNS:
        scale = np.abs(want["dpose_ray"][..., sl]).max()
        assert scale > 0 and np.abs(dpose[..., sl] - want["dpose_ray"][..., sl]).max() <= 1e-9 * scale, name


def test_t_near_clamp_of_the_reference():
    """t_near = 0 from inside the box: the entry is the origin, n counts the ray not the line, and the origin's gradient through
    the frozen clamp is gone (what remains is the exit face's)."""
    o = torch.tensor([[0.3, 0.2, -0.4], [2.5, 0.1, 0.2]], dtype=torch.float64, requires_grad=True)
    d = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], dtype=torch.float64)
    e0, x0, n0 = BR.slab(o, d, (16, 16, 16), 1.0)
    e1, x1, n1 = BR.slab(o, d, (16, 16, 16), 1.0, t_near=0.0)
    ap = lambda v: pytest.approx(v, abs=1e-15)
    assert e0.tolist() == ap([-1.3, 1.5]) and e1.tolist() == ap([0.0, 1.5]) and x0.tolist() == x1.tolist() == ap([0.7, 3.5])
    assert e1[0] == 0.0
    assert n1[0] < n0[0] and n1[1] == n0[1]
    g, = torch.autograd.grad(e1.sum(), o)
    assert g[0].tolist() == [0.0, 0.0, 0.0] and g[1].tolist() == [1.0, 0.0, 0.0]


# --- 4. conditioning, from the references alone -------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,bundle", BR.GRAD_CASES, ids=lambda v: str(v))
def test_every_gradient_bundle_keeps_its_well_conditioned_rays(scene, bundle):
    """camgrad_gpu.well_conditioned's own cap and rule (FLOOR of each tensor's scale, the columns origin and dir, near-kink rays
    excluded): at least 80 % of the n > 1 rays of every bundle the GPU gradient tests use."""
    inp = BR.inputs(scene, bundle)
    ref, ref32 = BR.refs(inp)
    K.check_conditions([(ref, ref32, BR.keep(ref, ref32), None)], "dray", BR.COLUMNS)
    if bundle == "ortho":
        assert (ref["n"] == 0).sum() == 4 and (ref["dray"][ref["n"][..., 0] == 0] == 0).all()
    if "near0" in bundle:
        assert (ref["entry"] == 0).all()   # every interior origin takes the clamp


def _differs(a, b, rays=None):
    """The float64 gradients a and b (over `rays`) differ by more than 1e-2 of a's scale."""
    rays = np.ones(a.shape[:2], bool) if rays is None else rays
    return np.abs(a - b)[rays].max() > 1e-2 * np.abs(a[rays]).max()


@pytest.mark.parametrize("scene,bundle", BR.EDGE_CASES, ids=lambda v: str(v))
def test_every_edge_bundle_keeps_its_well_conditioned_rays_and_tells_right_from_wrong(scene, bundle):
    """The same check for the bundles of tests/test_gpu_bundle_edges.py, the structure each is there for, and that the edge
    matters: the float64 d_origin / d_dir of the program without it is more than 1e-2 of the scale away.
    Good of n > 1 rays: a_orbit_sr1 axial 93 of 96, one_zero 94 of 96; b_sr2_ert axial 93 of 96, one_zero 89 of 96; c_clip random
    187 of 192 (all clipped), ortho 136 of 140 (126 clipped), interior_near0 123 of 128 (114 clipped); a_orbit_sr1 random_near2
    187 of 192 (135 rays take the clamp, 57 do not), random_near3 175 of 180 (12 killed), interior_near0_jitter 123 of 128.
    BR.keep keeps every ray of all of them."""
    inp = BR.inputs(scene, bundle)
    ref, ref32 = BR.refs(inp)
    K.check_conditions([(ref, ref32, BR.keep(ref, ref32), None)], "dray", BR.COLUMNS)
    live = ref["n"] > 1
    o, d = inp["origins"], inp["dirs"]
    assert not ((d == 0) & (np.abs(o) == 1)).any()   # no origin on a face plane of an axis the ray does not move along
    other = lambda **kw: BR.run(dict(inp, **kw))
    if bundle == "axial":
        assert ((d == 0).sum(1) == 2).all() and (np.abs(d).sum(1) == 1).all() and live.all()
        assert sorted(set(map(tuple, d))) == sorted(tuple(s * e) for e in np.eye(3) for s in (1.0, -1.0))
    if bundle == "one_zero":
        assert ((d == 0).sum(1) == 1).all() and (d[np.arange(len(d)), np.arange(len(d)) % 3] == 0).all() and live.all()
    if scene == "c_clip":
        S = int(inp["max_samples"])
        assert S == 23 and (ref["n"][live] > S).sum() >= 0.8 * live.sum() and ref["steps"].max() == S
        assert _differs(ref["dray"], other(max_samples=4096)["dray"])
    if bundle == "random_near2":
        off = other(t_near=None)
        clamped = ref["entry"] > off["entry"]
        assert (ref["entry"][clamped] == 2.0).all() and (ref["n"][clamped] <= off["n"][clamped]).all()
        assert (ref["n"][clamped] < off["n"][clamped]).sum() > 50   # (a clamp of less than a sample's spacing keeps n)
        assert (clamped & live).sum() > 50 and (~clamped & live).sum() > 50
        assert _differs(ref["dray"], off["dray"], clamped)
        assert np.array_equal(ref["dray"][~clamped], off["dray"][~clamped])
    if bundle == "random_near3":
        off = BR.run(dict(inp, t_near=None), grads=False)
        killed = (ref["n"] == 0) & (off["n"] > 1)
        assert killed.sum() >= 8 and (ref["dray"][killed] == 0).all() and (ref["rgba"][killed] == 0).all()
    if bundle == "interior_near0_jitter":
        assert (ref["entry"] > 0).all()   # every origin takes the clamp, and the draw moves the first sample off it
        assert _differs(ref["dray"], other(jitter_seed=0)["dray"])


def test_the_single_sample_set_has_single_sample_rays_among_rays_the_clamp_leaves_alone():
    inp = BR.inputs("a_orbit_sr1", "single_sample")
    ref, ref32 = BR.run(inp), BR.run(inp, torch.float32)
    off = BR.run(dict(inp, t_near=None), grads=False)
    one, rest = BR.SINGLE, ~BR.SINGLE
    assert one.sum() == 8 and (ref["n"][one] == 1).all() and (ref32["n"][one] == 1).all() and (off["n"][one] > 1).all()
    assert (ref["dray"][one] == 0).all() and (ref["rgba"][one] == 0).all()   # H6: the reference marches no such ray
    assert (ref["n"][rest] > 1).all() and np.array_equal(ref["n"][rest], off["n"][rest])
    assert np.array_equal(ref["entry"][rest], off["entry"][rest])


@pytest.mark.parametrize("R", BR.TIER_EDGE_R)
def test_the_smooth_table_tiers_keep_their_well_conditioned_rays(R):
    """Good of 64: R = 3393 59, 10176 64, 10177 62."""
    inp = BR.smooth_tier_inputs(R)
    assert inp["tf"].shape == (R, 4) and inp["origins"].shape == (64, 3)
    ref, ref32 = BR.refs(inp)
    assert (ref["n"] > 1).all()
    K.check_conditions([(ref, ref32, BR.keep(ref, ref32), None)], "dray", BR.COLUMNS)


def test_the_modules_cone_beam_has_a_zero_component_column_and_keeps_its_rays():
    """120 of 120 rays hit and are kept; detector column 4's x component is exactly 0 in both precisions."""
    inp = BR.cone_inputs()
    ref, ref32 = BR.cone_gradient(inp, grads=False), BR.cone_gradient(inp, torch.float32, grads=False)
    H, W = BR.CONE["det"]
    for r in (ref, ref32):
        d = r["dirs"].reshape(H, W, 3)
        assert (d[:, BR.CONE_ZERO_COLUMN, 0] == 0).all() and (d != 0).sum() == 3 * H * W - H
    live = ref["n"] > 1
    assert live.sum() > 0.8 * H * W and (BR.keep(ref, ref32) & live).sum() > 0.8 * live.sum()
    scale = BR.cone_scale()
    assert scale.min() >= 0.5 and scale.max() <= 2.0 and np.abs(scale - 1.0).min() > 1e-4   # no ray is handed over as a unit vector


# --- 5. the module's argument checks ------------------------------------------------------------------------------------------------

def test_module_argument_checks(hiplib):
    from differender_amd.bundle import RayBundleRaycaster
    with pytest.raises(ValueError):
        RayBundleRaycaster((8, 8), 4)
    with pytest.raises(ValueError):
        RayBundleRaycaster((8, 8, 8), 0)
    with pytest.raises(ValueError):
        RayBundleRaycaster((8, 8, 8), 4, max_samples=0)
    with pytest.raises(ValueError):
        RayBundleRaycaster((8, 8, 8), 4, t_near=float("nan"))
    rc = RayBundleRaycaster((8, 9, 10), 4)
    vol, tf, o, d = torch.rand(1, 8, 9, 10), torch.rand(4, 4), torch.zeros(5, 7, 3), torch.ones(5, 7, 3)
    for bad in ((vol[0], tf, o, d), (torch.rand(1, 8, 9, 11), tf, o, d), (vol, torch.rand(4, 5), o, d), (vol, tf.t()[:3], o, d),
                (vol, tf, o[0], d), (vol, tf, o[..., :2], d[..., :2]), (vol, tf, o[:0], d[:0]), (torch.rand(2, 8, 9, 10), tf, o, d)):
        with pytest.raises(ValueError):
            rc(*bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # shapes fine, tensors on the CPU: there is no CPU path
        rc(vol, tf, o, d)


def test_ray_tensors_that_require_grad_need_ray_grad(hiplib):
    from differender_amd.bundle import RayBundleRaycaster
    rc = RayBundleRaycaster((8, 8, 8), 4)
    vol, tf = torch.rand(1, 8, 8, 8), torch.rand(4, 4)
    for name in ("origins", "directions"):
        rays = dict(origins=torch.zeros(6, 3), directions=torch.ones(6, 3))
        rays[name].requires_grad_(True)
        with pytest.raises(ValueError, match=f"no gradient w.r.t. {name}.*ray_grad=True"):
            rc(vol, tf, **rays)
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):   # (nothing to refuse without autograd)
            rc(vol, tf, **rays)


def test_a_zero_length_direction_raises(hiplib):
    from differender_amd.bundle import RayBundleRaycaster
    rc = RayBundleRaycaster((8, 8, 8), 4, ray_grad=True)
    d = torch.ones(6, 3)
    d[4] = 0.0
    with pytest.raises(ValueError, match="zero length"):
        rc(torch.rand(1, 8, 8, 8), torch.rand(4, 4), torch.zeros(6, 3), d)
