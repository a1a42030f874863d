"""The depth march over ray bundles, DESIGN.md D22, without a GPU: the exports, the three C entries and their argument checks,
the float64 reference (tests/depth_bundle_reference.py) against central finite differences of itself and against
tests/depth_reference.py on a pinhole camera's rays, the conditions every case of the GPU file (tests/test_gpu_depth_bundle.py)
owes its comparisons, three mutations the GPU file's rules must reject, the channel-last helpers and the module's argument
checks."""
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
import depth_bundle_reference as DB  # noqa: E402
import depth_reference as DR  # noqa: E402
import light_gpu as LG  # noqa: E402
import pose_gpu as PG  # noqa: E402
from test_gpu_bundle import ray_rule  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_march_depth_bundle_fwd", "dr_march_depth_bundle_bwd", "dr_march_depth_bundle_bwd_rays")
D19 = ("dr_march_bundle_fwd", "dr_march_bundle_bwd", "dr_march_bundle_bwd_rays")
INF = float("inf")


# --- 1. exports and the C ABI ---------------------------------------------------------------------------------------------------

def test_exports():
    import differender_amd
    import differender_amd.depth as D
    import differender_amd.functional as F
    for name in ("RayBundleDepthRaycaster", "RayBundleDepthFunction", "ray_expected_depth", "ray_depth_variance"):
        assert name in D.__all__ and hasattr(D, name)
        assert not hasattr(differender_amd, name)   # the package re-exports none of them
    for name in ("march_depth_bundle_fwd", "march_depth_bundle_bwd", "march_depth_bundle_bwd_rays"):
        assert callable(getattr(F, name))
    import inspect
    for new, old in (("march_depth_bundle_fwd", "march_bundle_fwd"), ("march_depth_bundle_bwd", "march_bundle_bwd"),
                     ("march_depth_bundle_bwd_rays", "march_bundle_bwd_rays")):
        assert inspect.signature(getattr(F, new)) == inspect.signature(getattr(F, old))
    from differender_amd.bundle import RayBundleRaycaster
    assert inspect.signature(D.RayBundleDepthRaycaster.__init__) == inspect.signature(RayBundleRaycaster.__init__)


def test_header_library_and_signatures_agree(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    assert N.lib().dr_abi_version() == 9   # the entries are additive
    for name, d19 in zip(ENTRIES, D19):
        params = _header_params(name)
        assert hasattr(raw, name)
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
                    ctypes.c_float if p.startswith("float") else ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)
        assert params == _header_params(d19)   # exactly the D19 entry's argument list, names included
        assert N.SIGNATURES[name] == N.SIGNATURES[d19]


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
    "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0), "R 0": dict(R=0), "R -2": dict(R=-2), "max_samples 0": dict(S=0),
    "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0), "sampling rate < 0": dict(sr=-1.0),
    "sampling rate nan": dict(sr=float("nan")), "sampling rate inf": dict(sr=INF),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    """The D19 entries' return codes, before any HIP call (the buffers are host memory)."""
    b = _Bufs()
    bad = INVALID[case]
    assert hiplib.dr_march_depth_bundle_fwd(*_args(b, "fwd", **bad)) == -1
    assert hiplib.dr_march_depth_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], dtf=b.p[1], **bad)) == -1
    assert hiplib.dr_march_depth_bundle_bwd(*_args(b, "bwd", **bad)) == -1   # (checked before "nothing requested")
    assert hiplib.dr_march_depth_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1


def test_nan_t_near_missing_outputs_and_nothing_requested(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_depth_bundle_bwd_rays(*_args(b, "rays", t_near=float("nan"))) == -1
    assert hiplib.dr_march_depth_bundle_fwd(*_args(b, "fwd", out=None)) == -1
    assert hiplib.dr_march_depth_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], go=None)) == -1
    assert hiplib.dr_march_depth_bundle_bwd(*_args(b, "bwd", dtf=b.p[1], out=None)) == -1
    assert hiplib.dr_march_depth_bundle_bwd(*_args(b, "bwd")) == 0   # d_vol == d_tf == NULL: nothing to do, no HIP call
    for bad in (dict(steps=None), dict(go=None), dict(out=None), dict(d_o=None), dict(d_d=None)):
        assert hiplib.dr_march_depth_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1, bad


# --- 2. the float64 reference against central differences of itself --------------------------------------------------------------

FD_RAYS = (3, 40, 77, 150)
FD_STEP = 1e-6   # moves a sample by less than 3e-5 of a cell: none of these rays' samples lies that close to a face of its cell


def _objective(inp):
    res = DB.run(inp, grads=False)
    return float((res["rgba"][:, 0] * inp["grad_out"]).sum()), res


@pytest.mark.parametrize("scene,bundle", [("a_orbit_sr1", "random_jitter"), ("b_sr2_ert", "random")], ids=str)
def test_the_f64_reference_is_the_central_difference_of_its_own_forward(scene, bundle):
    """Four rays of a case (their origins and directions as free 3-vectors: dray's 24 numbers -- the direction steps change
    |d|, so they hold the definition of t as the march parameter), the alpha entries of d_tf and five voxels, each against
    (L(+h) - L(-h)) / 2h of the float64 forward with n and steps unchanged by the step."""
    full = DB.inputs(scene, bundle)
    idx = np.array(FD_RAYS)
    inp = dict(full, origins=full["origins"][idx], dirs=full["dirs"][idx], grad_out=full["grad_out"][idx])
    ref = DB.run(inp)   # (a jitter draw is per ray index: rays 0..3 of the sub-bundle draw their own, the same in every run)
    assert (ref["n"] > 1).all()
    scale = np.abs(ref["dray"]).max()
    for key, col in (("origins", 0), ("dirs", 3)):
        for p in range(len(idx)):
            for a in range(3):
                lo, hi = (dict(inp, **{key: inp[key].copy()}) for _ in range(2))
                lo[key][p, a] -= FD_STEP
                hi[key][p, a] += FD_STEP
                (Ll, rl), (Lh, rh) = _objective(lo), _objective(hi)
                assert (rl["n"] == ref["n"]).all() and (rh["n"] == ref["n"]).all()
                assert (rl["steps"] == ref["steps"]).all() and (rh["steps"] == ref["steps"]).all()
                fd = (Lh - Ll) / (2 * FD_STEP)
                assert abs(fd - ref["dray"][p, 0, col + a]) <= 1e-6 * scale, (key, p, a, fd, ref["dray"][p, 0, col + a])
    dt = ref["dtf"]
    assert (dt[:, :3] == 0).all() and np.abs(dt[:, 3]).max() > 0   # depth reads the alpha column alone
    for k in range(dt.shape[0]):
        lo, hi = (dict(inp, tf=inp["tf"].copy()) for _ in range(2))
        lo["tf"][k, 3] -= FD_STEP
        hi["tf"][k, 3] += FD_STEP
        fd = (_objective(hi)[0] - _objective(lo)[0]) / (2 * FD_STEP)
        assert abs(fd - dt[k, 3]) <= 1e-6 * np.abs(dt).max(), (k, fd, dt[k, 3])
    dv = ref["dvol"]
    for k in np.argsort(np.abs(dv).reshape(-1))[::-1][:5]:
        at = np.unravel_index(int(k), dv.shape)
        lo, hi = (dict(inp, vol=inp["vol"].copy()) for _ in range(2))
        lo["vol"][at] -= FD_STEP
        hi["vol"][at] += FD_STEP
        fd = (_objective(hi)[0] - _objective(lo)[0]) / (2 * FD_STEP)
        assert abs(fd - dv[at]) <= 1e-6 * np.abs(dv).max(), (at, fd, dv[at])


# --- 3. on a pinhole camera's rays the reference is tests/depth_reference.py --------------------------------------------------------

POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
CAM = (-1.3, 0.9, 2.0)


def test_on_pinhole_rays_the_reference_is_the_depth_references():
    """The moments to 1e-12; the ten pose columns, the bundle's d_origin and d_dir pushed through autograd of pinhole_rays (which
    normalises: the radial part of d_dir, where the two definitions of t differ, drops out), to 1e-9 of each tensor's scale."""
    from differender_amd.bundle import pinhole_rays
    inp = PG.inputs("a_orbit_sr1", look_from=np.array(CAM), **POSE)
    assert int(inp["jitter_seed"]) == 0
    want = DR.run_case(inp)
    W, H = want["n"].shape
    leaves = [torch.tensor(np.asarray(a, np.float64), requires_grad=True)
              for a in (inp["look_from"], inp["look_at"], inp["up"], math.degrees(float(inp["fov_rad"])))]
    o, d = pinhole_rays(*leaves, (W, H))
    kernel_order = lambda img: torch.flip(img, (0,)).transpose(0, 1)   # (H, W, ...) user orientation -> (W, H, ...)
    o, d = kernel_order(o).reshape(-1, 3), kernel_order(d).reshape(-1, 3)
    binp = dict(vol=inp["vol"], tf=inp["tf"], origins=o.detach().numpy(), dirs=d.detach().numpy(),
                grad_out=inp["grad_out"].reshape(-1, 4), sr=inp["sr"], max_samples=inp["max_samples"])
    got = DB.run(binp)
    assert (got["n"].reshape(W, H) == want["n"]).all() and (got["steps"].reshape(W, H) == want["steps"]).all()
    assert (want["n"] > 1).sum() > 50
    assert np.abs(got["rgba"].reshape(W, H, 4) - want["rgba"]).max() <= 1e-12
    ((o * torch.from_numpy(got["d_origin"][:, 0])).sum() + (d * torch.from_numpy(got["d_dir"][:, 0])).sum()).backward()
    ten = np.concatenate([leaves[0].grad.numpy(), leaves[1].grad.numpy(), leaves[2].grad.numpy(),
                          [float(leaves[3].grad) * 180.0 / math.pi]])
    for name, sl in PG.COLUMNS:
        scale = np.abs(want["dpose"][sl]).max()
        assert scale > 0 and np.abs(ten[sl] - want["dpose"][sl]).max() <= 1e-9 * scale, (name, ten[sl], want["dpose"][sl])


# --- 4. conditioning and premises, from the references alone ------------------------------------------------------------------------

def _all_states():
    for scene, bundle in DB.GRAD_CASES + DB.AIR_CASES + [DB.SINGLE_CASE]:
        yield (scene, bundle), DB.state(scene, bundle)
    for scene, bundle, over in DB.RATE_CASES:
        yield (scene, bundle, over), DB.state(scene, bundle, tuple(sorted(over.items())))


def test_every_case_of_the_gpu_file_is_well_conditioned():
    """camgrad_gpu.check_conditions over d_origin and d_dir (no lighting) on every case the GPU file compares ray gradients on:
    the float32 and float64 references agree on n and steps on bundle_reference.keep's rays, and more than 80 % of the n > 1
    rays are within camgrad_gpu.FLOOR of float64 in float32."""
    entries = []
    for what, (inp, ref, ref32) in _all_states():
        keep = DB.keep(ref, ref32)
        assert (ref32["n"][keep] == ref["n"][keep]).all() and (ref32["steps"][keep] == ref["steps"][keep]).all(), what
        entries.append((ref, ref32, keep, None))
    K.check_conditions(entries, key="dray", columns=BR.COLUMNS, lit=False)


def test_each_edge_cases_premise_holds():
    for near in ("random_near2", "random_near3"):
        inp, ref, _ = DB.state("a_orbit_sr1", near)
        off = DB.run(dict(inp, t_near=None), grads=False)
        clamped = (ref["entry"] == inp["t_near"]) & (ref["n"] > 0)
        dead = (ref["n"] == 0) & (off["n"] > 1)
        assert (clamped & (ref["n"] > 1)).any(), near
        if near == "random_near2":   # some rays take the clamp, others enter the box beyond it
            assert (~clamped & (ref["n"] > 1)).any() and not dead.any()
        else:                        # ... and some die: t_near lies past their exit
            assert dead.any()
    for bundle in ("random", "ortho", "interior_near0"):
        inp, ref, _ = DB.state("c_clip", bundle)
        S = int(inp["max_samples"])
        assert ((ref["n"] > S) & (ref["steps"] == S)).sum() > 0.2 * (ref["n"] > 1).sum(), bundle   # the cap bites
    inp, ref, ref32 = DB.state(*DB.SINGLE_CASE)
    one = BR.SINGLE
    assert (ref["n"][one] == 1).all() and (ref32["n"][one] == 1).all() and (ref["n"][~one] > 1).all()
    assert (ref["dray"][one] == 0).all() and (ref["rgba"][one] == 0).all()   # H6: the reference marches no such ray
    for scene, bundle, over in DB.RATE_CASES:
        inp, ref, _ = DB.state(scene, bundle, tuple(sorted(over.items())))
        if "max_samples" in over:
            assert (ref["steps"][ref["n"] > 1] == over["max_samples"]).all() and np.abs(ref["dray"]).max() > 0
    inp, ref, _ = DB.state("j_inside", "interior")
    assert (ref["rgba"][..., 0] < 0).any()   # an origin inside the box collects negative distances behind it ...
    inp, ref, _ = DB.state("j_inside", "interior_near0")
    assert (ref["rgba"][..., 0] >= 0).all() and (ref["entry"] == 0).all()   # ... and none under t_near = 0


# --- 5. three mutations, arrays in the kernel's place ---------------------------------------------------------------------------------

def test_the_gpu_files_rules_reject_three_mutations():
    inp, ref, ref32 = DB.state("a_orbit_sr1", "random")
    good = K.well_conditioned(ref, ref32, DB.keep(ref, ref32), "dray", BR.COLUMNS, lit=False)
    m = good[..., None]
    ray_rule(ref32["dray"] * m, ref, ref32, good)   # (the float32 transliteration passes)
    with pytest.raises(AssertionError):             # a ray gradient 1 % too large
        ray_rule(1.01 * ref["dray"] * m, ref, ref32, good)
    LG.bound(ref32["dtf"], ref["dtf"], ref32["dtf"], "dtf")
    with pytest.raises(AssertionError):             # d_tf shifted by one texel
        LG.bound(np.roll(ref["dtf"], 1, axis=0), ref["dtf"], ref32["dtf"], "dtf shifted")
    # the radial term 2 t e_s d in d_dir: the other definition of t, (pos - o) . d = t |d|^2. The directions are unit vectors up
    # to their rounding to float32 (| |d|^2 - 1 | <= 2e-7), so its forward and its d_origin are the same to 1e-6 ...
    rad = DB.run(inp, radial=True)
    assert np.abs((inp["dirs"] ** 2).sum(1) - 1.0).max() <= 2e-7
    assert np.abs(rad["rgba"] - ref["rgba"]).max() <= 1e-6 * np.abs(ref["rgba"]).max()
    assert np.abs(rad["d_origin"] - ref["d_origin"]).max() <= 1e-6 * np.abs(ref["d_origin"]).max()
    d = inp["dirs"][:, None, :]
    radial = ((rad["d_dir"] - ref["d_dir"]) * d).sum(-1, keepdims=True) * d    # ... and d_dir differs along d, by percents
    assert np.abs((rad["d_dir"] - ref["d_dir"]) - radial).max() <= 1e-6 * np.abs(ref["d_dir"]).max()
    assert np.abs(radial).max() > 1e-2 * np.abs(ref["d_dir"]).max()
    with pytest.raises(AssertionError):
        ray_rule(rad["dray"] * m, ref, ref32, good)


# --- 6. the channel-last helpers -------------------------------------------------------------------------------------------------------

def test_ray_helpers_are_the_channel_first_ones_and_differentiable():
    from differender_amd.depth import depth_variance, expected_depth, ray_depth_variance, ray_expected_depth
    g = torch.Generator().manual_seed(3)
    a = torch.rand(5, 7, generator=g, dtype=torch.float64)
    a[0, :3] = 0.0                               # rays that collected nothing
    m1 = a * (1.0 + torch.rand(5, 7, generator=g, dtype=torch.float64))
    m2 = m1 * m1 / torch.where(a > 0, a, torch.ones_like(a)) + 0.1 * a * torch.rand(5, 7, generator=g, dtype=torch.float64)
    last = torch.stack([m1, m2, a], -1)          # (5, 7, 3)
    first = last.permute(2, 0, 1)                # (3, 5, 7)
    assert torch.equal(ray_expected_depth(last, background=-2.0), expected_depth(first, background=-2.0))
    assert torch.equal(ray_depth_variance(last), depth_variance(first))
    assert ray_expected_depth(last[0, 0]).shape == () and ray_expected_depth(last, background=9.0)[0, 0] == 9.0
    assert float(ray_depth_variance(last)[0, 0]) == 0.0
    for bad in (first, torch.zeros(4), 3.0):
        with pytest.raises(ValueError):
            ray_expected_depth(bad)
        with pytest.raises(ValueError):
            ray_depth_variance(bad)
    hit = last[1:].clone().requires_grad_(True)   # gradcheck where A > eps and the variance's clamp is not at its kink
    assert torch.autograd.gradcheck(ray_expected_depth, (hit,))
    assert torch.autograd.gradcheck(ray_depth_variance, (hit,))
    assert (ray_depth_variance(hit) > 1e-4).all()


# --- 7. the module's argument checks ----------------------------------------------------------------------------------------------------

def test_module_argument_checks(hiplib):
    from differender_amd.depth import RayBundleDepthRaycaster
    with pytest.raises(ValueError):
        RayBundleDepthRaycaster((8, 8), 8)
    with pytest.raises(ValueError):
        RayBundleDepthRaycaster((8, 8, 8), 0)
    with pytest.raises(ValueError):
        RayBundleDepthRaycaster((8, 8, 8), 8, max_samples=0)
    with pytest.raises(ValueError):
        RayBundleDepthRaycaster((8, 8, 8), 8, t_near=float("nan"))
    rc = RayBundleDepthRaycaster((8, 9, 10), 6)
    vol, tf, o, d = torch.rand(1, 8, 9, 10), torch.rand(4, 6), torch.zeros(5, 7, 3), torch.ones(5, 7, 3)
    for bad in ((vol[0], tf, o, d), (torch.rand(1, 8, 9, 11), tf, o, d), (vol, tf[:3], o, d), (vol, torch.rand(4, 7), o, d),
                (vol, tf, o[0], d), (vol, tf, o[..., :2], d[..., :2]), (vol, tf, o[:0], d[:0])):
        with pytest.raises(ValueError):
            rc(*bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # shapes fine, tensors on the CPU: there is no CPU path
        rc(vol, tf, o, d)
    assert "ray_grad = False" in repr(rc) and "t_near = None" in repr(rc)


def test_ray_tensors_that_require_grad_need_ray_grad(hiplib):
    from differender_amd.depth import RayBundleDepthRaycaster
    rc = RayBundleDepthRaycaster((8, 8, 8), 6)
    vol, tf = torch.rand(1, 8, 8, 8), torch.rand(4, 6)
    for name in ("origins", "directions"):
        rays = dict(origins=torch.zeros(6, 3), directions=torch.ones(6, 3))
        rays[name].requires_grad_(True)
        with pytest.raises(ValueError, match=f"no gradient w.r.t. {name}.*ray_grad=True"):
            rc(vol, tf, **rays)


def test_a_zero_length_direction_raises(hiplib):
    from differender_amd.depth import RayBundleDepthRaycaster
    rc = RayBundleDepthRaycaster((8, 8, 8), 6, ray_grad=True)
    d = torch.ones(6, 3)
    d[4] = 0.0
    with pytest.raises(ValueError, match="zero length"):
        rc(torch.rand(1, 8, 8, 8), torch.rand(4, 6), torch.zeros(6, 3), d)
