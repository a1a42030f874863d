"""The RGBA march's camera gradient without a GPU: the float64 reference of tests/rgba_pose_reference.py against
central differences of itself and against the invariants of the camera model, the two C entries and their argument checks, and
the module's host rules (the default refusals, the camera_grad=True paths)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import pose_reference as PR  # noqa: E402
import rgba_camera_scenes as SC  # noqa: E402
import rgba_pose_reference as RP  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_march_rgba_bwd_cam", "dr_march_rgba_bwd_pose")
POSE_KEYS = ("look_from", "look_at", "up", "fov_rad")


def _theta(inp):
    return np.concatenate([np.asarray(inp[k], np.float64).reshape(-1) for k in POSE_KEYS])


def _at(inp, theta):
    return RP.run_case(dict(inp, look_from=theta[0:3], look_at=theta[3:6], up=theta[6:9], fov_rad=theta[9]))


# --- 1. the reference against central differences of itself ----------------------------------------------------------------

@pytest.mark.parametrize("opaque,sr,seed", [(False, 1.0, 0), (True, 2.0, 77)], ids=["thin_sr1", "opaque_sr2_jit"])
def test_reference_gradient_matches_central_differences_of_itself(opaque, sr, seed):
    """test_pose.py's method on the RGBA program: all ten parameters, ray by ray, h = 1e-6 (truncation 1e-12 relative, rounding
    1e-10 of the objective), on the rays whose n and live samples are the same at both ends of every difference and that are
    away from face ties. 1e-6 of the largest component leaves four digits of margin."""
    inp = SC.make(opaque=opaque, sr=sr, seed=seed, **SC.POSED)
    theta0 = _theta(inp)
    ref = _at(inp, theta0)
    if opaque:
        assert (ref["steps"] < np.minimum(ref["n"], int(inp["max_samples"])))[ref["n"] > 1].any()   # frozen live counts are exercised
    per_ray = lambda res: (res["rgba"] * inp["grad_out"]).sum(-1)
    h = 1e-6
    fd = np.zeros_like(ref["dpose_ray"])
    same = ref["n"] > 1
    same &= (PR.face_margin(theta0[:3], ref["rays"], True) > 1e-3) & (PR.face_margin(theta0[:3], ref["rays"], False) > 1e-3)
    for k in range(10):
        tp, tm = theta0.copy(), theta0.copy()
        tp[k] += h; tm[k] -= h
        rp, rm = _at(inp, tp), _at(inp, tm)
        fd[..., k] = (per_ray(rp) - per_ray(rm)) / (2.0 * h)
        same &= (rp["n"] == ref["n"]) & (rm["n"] == ref["n"]) & (rp["steps"] == ref["steps"]) & (rm["steps"] == ref["steps"])
    assert same.sum() >= 0.5 * (ref["n"] > 1).sum() and same.sum() >= 8
    scale = np.abs(ref["dpose_ray"][same]).max()
    err = np.abs(fd - ref["dpose_ray"])[same].max()
    cols = [np.abs(ref["dpose_ray"][same][:, k]).max() / scale for k in range(10)]
    print("rgba pose fd: rays %d of %d, err/scale %.3g, smallest column %.3g" % (same.sum(), (ref["n"] > 1).sum(), err / scale, min(cols)))
    assert err <= 1e-6 * scale
    for k in range(10):   # every parameter is exercised
        assert cols[k] > 1e-6, k


@pytest.mark.parametrize("jitter", [0, 99])
def test_pose_gradient_invariants(jitter):
    """What the camera model implies for every ray, to rounding (test_pose.py's three): the image does not change when look_at
    slides along the viewing direction, when up is scaled, or when up moves along the viewing direction."""
    inp = SC.make(opaque=True, sr=2.0, seed=jitter, **SC.POSED)
    res = RP.run_case(inp)
    d = res["dpose_ray"][res["n"] > 1]
    lf, la, up = (np.asarray(inp[k], np.float64) for k in ("look_from", "look_at", "up"))
    vdir = (la - lf) / np.linalg.norm(la - lf)
    scale = np.abs(d).max()
    assert len(d) >= 8 and scale > 0
    assert np.abs(d[:, 3:6] @ vdir).max() <= 1e-12 * scale
    assert np.abs(d[:, 6:9] @ up).max() <= 1e-12 * scale
    assert np.abs(d[:, 6:9] @ vdir).max() <= 1e-12 * scale


def test_default_pose_columns_are_the_fixed_cameras():
    """Under the default pose the look_from columns are the gradient of the fixed camera's program (look_at at the origin: the
    viewing direction depends on look_from alone), which is what dr_march_rgba_bwd_cam is held to."""
    inp = SC.case("default_sr1")
    res = RP.run_case(inp)
    posed = RP.run_case(dict(inp, look_at=PR.ORIGIN, up=PR.UP_Y, fov_rad=np.radians(PR.FOV_DEG)))
    assert np.array_equal(res["rgba"], posed["rgba"]) and np.array_equal(res["dpose_ray"], posed["dpose_ray"])
    assert np.abs(res["dpose_ray"][..., :3]).max() > 0


def _conditioned_cases():
    import test_gpu_rgba_camera as TG
    import test_gpu_rgba_camera_edges as TE
    assert not set(TG.CONDITIONED) & set(TE.CONDITIONED)
    return dict(TG.CONDITIONED, **TE.CONDITIONED)


CONDITIONED = _conditioned_cases()


@pytest.mark.parametrize("case", sorted(CONDITIONED))
def test_cases_keep_enough_well_conditioned_rays(case):
    """What test_gpu_rgba_camera.py and test_gpu_rgba_camera_edges.py feed to the conditioned pass (pose_gpu.well_conditioned),
    held to its conditions without a GPU: the rays on which the float32 and the float64 reference agree to 1e-4 of each pose
    tensor's scale are at least 80 % of the n > 1 rays, and err32 over them is within 1e-4 of the scale. (The scenes of the
    look_from entry, under the default pose, are held to all four tensors' conditions: no fewer rays than its own three
    columns would leave out.)"""
    import camgrad_gpu as K
    import pose_gpu as PG
    K.check_conditions(CONDITIONED[case](), "dpose_ray", PG.COLUMNS, lit=False)   # (D16: no lighting, no kinks)


def test_the_conditioned_rule_rejects_a_one_percent_error_in_a_multi_workgroup_total():
    """The 17 x 19 scene of test_gpu_rgba_camera_edges.py (three workgroups), with arrays in the kernel's place: eight rays put
    err32 at 0.9 % (d look_at) and 2.4 % (d up) of the scale, and the rule over all kept rays accepts gradients of those two
    tensors that are 1 % off in every column of every ray, with a total that is their sum; over the well-conditioned rays it
    does not (camgrad_gpu.mutation_check, tensor by tensor as pose_rule judges them). d look_from and d fov have an err32 of
    0.6 % and 0.2 % there: the first pass rejects their 1 % error already (the total's and the per-ray bound), and the
    conditioned pass rejects it as well."""
    import camgrad_gpu as K
    import pose_gpu as PG
    import test_gpu_rgba_camera_edges as TE
    _, ref, ref32 = TE._edge("wg3_17x19")
    assert ref["n"].shape == (17, 19)
    keep = PG.keep(ref, ref32)
    good = PG.well_conditioned(ref, ref32, keep, lit=False)
    assert good.sum() < (keep & (ref["n"] > 1)).sum()   # there are ill-conditioned rays to leave out

    def rule_of(sl):
        three = lambda r: {"n": ref["n"], "dcam_ray": PG._three(r["dpose_ray"], sl)}
        return lambda ray, total, ref, ref32, mask: K.d8_rule(PG._three(ray, sl), PG._three(total, sl), three(ref), three(ref32), mask)

    for name, sl in PG.COLUMNS:
        if name in ("look_at", "up"):
            K.mutation_check(rule_of(sl), ref["dpose_ray"], ref32["dpose_ray"], ref, ref32, keep, good)
        else:
            wrong = 1.01 * ref["dpose_ray"] * good[..., None]
            with pytest.raises(AssertionError):
                rule_of(sl)(wrong, wrong.sum((0, 1)), ref, ref32, good)
            right = ref32["dpose_ray"] * good[..., None]
            rule_of(sl)(right, right.sum((0, 1)), ref, ref32, good)
    with pytest.raises(AssertionError):   # and pose_rule as a whole, over the well-conditioned rays
        wrong = 1.01 * ref["dpose_ray"] * good[..., None]
        PG.pose_rule(wrong, wrong.sum((0, 1)), ref, ref32, good)


# --- 2. the C ABI -----------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    assert N.ABI_VERSION == 9 and N.lib().dr_abi_version() == 9   # the entries are additive
    kinds = (("int64_t", ctypes.c_int64), ("uint32_t", ctypes.c_uint32), ("float", ctypes.c_float), ("double", ctypes.c_double))
    for name in ENTRIES:
        params = _header_params(name)
        assert hasattr(raw, name)
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else next((t for k, t in kinds if p.startswith(k)), ctypes.c_int)
            assert a is want, (name, p, a)
    # _pose is _cam plus (pose, fov_v)
    assert len(N.SIGNATURES[ENTRIES[1]][1]) == len(N.SIGNATURES[ENTRIES[0]][1]) + 2


def _cam_args(b, pose_entry, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, sc=512, vs=0, cam=b.p[2], entry=b.p[3], exit=b.p[4],
             rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, fov=0.5, near=0.1, seed=0, view_base=0, steps=b.p[6], go=b.p[7],
             out=b.p[7])
    if pose_entry:
        a.update(pose=b.p[1], fov_v=None)
    a.update(dcam=b.p[1], dray=None, stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null cam": dict(cam=None), "null entry": dict(entry=None), "null exit": dict(exit=None),
    "null rays": dict(rays=None), "null n": dict(n=None), "null steps": dict(steps=None), "null grad_out": dict(go=None),
    "null out": dict(out=None), "null d_cam": dict(dcam=None), "unknown dtype": dict(dtype=7), "views 0": dict(V=0),
    "W 0": dict(W=0), "H -1": dict(H=-1), "VX 0": dict(VX=0), "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0),
    "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0), "sampling rate < 0": dict(sr=-1.0),
    "sampling rate inf": dict(sr=float("inf")), "sampling rate nan": dict(sr=float("nan")),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    assert hiplib.dr_march_rgba_bwd_cam(*_cam_args(b, False, **INVALID[case])) == -1
    assert hiplib.dr_march_rgba_bwd_pose(*_cam_args(b, True, **INVALID[case])) == -1
    assert hiplib.dr_march_rgba_bwd_pose(*_cam_args(b, True, fov_v=b.p[1], **INVALID[case])) == -1


def test_pose_entry_needs_a_pose(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_rgba_bwd_pose(*_cam_args(b, True, pose=None)) == -1
    assert hiplib.dr_march_rgba_bwd_pose(*_cam_args(b, True, pose=None, fov_v=b.p[1])) == -1   # fov_v without pose


# --- 3. the module ----------------------------------------------------------------------------------------------------------

def _module_inputs():
    return torch.zeros(4, 8, 8, 8), torch.tensor([2.0, 0.5, 1.0])


@pytest.mark.parametrize("name", ["look_from", "look_at", "up", "fov"])
def test_default_module_still_refuses_each_camera_tensor_by_name(hiplib, name):
    from differender_amd.rgba import RaycasterRGBA
    vol, lf = _module_inputs()
    t = dict(look_from=lf.clone(), look_at=torch.zeros(3), up=torch.tensor([0.1, 1.0, 0.0]), fov=torch.tensor(25.0))[name]
    t.requires_grad_(True)
    rc = RaycasterRGBA((8, 8, 8), (6, 6), jitter=False)
    assert rc.camera_grad is False
    with pytest.raises(ValueError, match=name) as exc:
        rc(vol, t) if name == "look_from" else rc(vol, lf, **{name: t})
    assert "camera_grad=True" in str(exc.value)


class _Reached(Exception):
    pass


def _reached(*a, **k):
    raise _Reached()


def _forbidden(what):
    def f(*a, **k):
        raise AssertionError(what)
    return f


def test_camera_grad_module_reaches_the_right_ray_setup(hiplib, monkeypatch):
    """camera_grad=True: a camera tensor that requires grad goes through F.ray_setup when look_at = up = fov = None and through
    F.ray_setup_pose otherwise. (No GPU here: the first functional call is intercepted, as test_pose.py does.)"""
    from differender_amd import functional as F
    from differender_amd.rgba import RaycasterRGBA
    vol, lf = _module_inputs()
    rc = RaycasterRGBA((8, 8, 8), (6, 6), jitter=False, camera_grad=True)
    monkeypatch.setattr(F, "ray_setup", _reached)
    monkeypatch.setattr(F, "ray_setup_pose", _forbidden("the pose path ran without a pose"))
    with pytest.raises(_Reached):
        rc(vol, lf.clone().requires_grad_(True))
    with pytest.raises(_Reached):
        rc(vol, lf.clone().requires_grad_(True), look_at=None, up=None, fov=None)
    monkeypatch.setattr(F, "ray_setup_pose", _reached)
    monkeypatch.setattr(F, "ray_setup", _forbidden("the fixed camera's path ran with a pose"))
    posed = [dict(look_at=torch.zeros(3, requires_grad=True)), dict(up=torch.tensor([0.1, 1.0, 0.0], requires_grad=True)),
             dict(fov=torch.tensor(25.0, requires_grad=True))]
    for kw in posed:
        with pytest.raises(_Reached):
            rc(vol, lf, **kw)
    with pytest.raises(_Reached):
        rc(vol, lf.clone().requires_grad_(True), fov=25.0)


def test_camera_grad_module_without_a_camera_gradient_takes_todays_path(hiplib, monkeypatch):
    """Nothing of the camera requires grad (or grad is disabled): RgbaCameraFunction is never built, whatever the volume asks."""
    from differender_amd import functional as F
    from differender_amd import rgba
    vol, lf = _module_inputs()
    rc = rgba.RaycasterRGBA((8, 8, 8), (6, 6), jitter=False, camera_grad=True)
    monkeypatch.setattr(rgba.RgbaCameraFunction, "apply", _forbidden("the camera function was built"))
    monkeypatch.setattr(F, "ray_setup", _reached)
    monkeypatch.setattr(F, "ray_setup_pose", _reached)
    calls = [lambda: rc(vol, lf), lambda: rc(vol.clone().requires_grad_(True), lf), lambda: rc(vol, lf, fov=25.0),
             lambda: rc(vol, lf, look_at=torch.zeros(3), up=torch.tensor([0.1, 1.0, 0.0]))]
    for call in calls:
        with pytest.raises(_Reached):
            call()
    with torch.no_grad(), pytest.raises(_Reached):
        rc(vol, lf.clone().requires_grad_(True), look_at=torch.zeros(3, requires_grad=True))
