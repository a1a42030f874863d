"""The free camera without a GPU: the float64 reference of tests/pose_reference.py against the fixed camera's
reference and against finite differences of itself, the invariants of the pose gradient, the C ABI's new entries and the host
rules (batching, the all-None path of every renderer)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_camgrad_golden as CG  # noqa: E402
import pose_reference as PR  # noqa: E402

POSE_ENTRIES = ("dr_ray_setup_pose_rows", "dr_march_fwd_rows_pose", "dr_march_bwd_rows_pose", "dr_march_bwd_pose",
                "dr_project_bwd_pose")


def _scene(seed=3, vshape=(12, 14, 10), WH=(7, 6), R=6):
    rng = np.random.RandomState(seed)
    ax = [np.linspace(-1.0, 1.0, n) for n in vshape]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    vol = np.clip(0.5 + 0.3 * np.sin(2.1 * X + 0.4) * np.cos(1.7 * Y) + 0.2 * Z * X + 0.02 * rng.standard_normal(vshape), 0.0, 1.0)
    tf = rng.uniform(0.05, 0.95, size=(R, 4))
    tf[:, 3] = np.linspace(0.01, 0.06, R)
    return dict(vol=vol, tf=tf, grad_out=rng.standard_normal((*WH, 4)), sr=np.float64(1.0), max_samples=np.int32(4096),
                jitter_seed=np.int64(0), view=np.int32(0))


PANNED = dict(look_from=(2.1, 0.7, 1.4), look_at=(0.15, -0.1, 0.2), up=(0.25, 1.0, -0.1), fov_rad=math.radians(24.0))


@pytest.mark.parametrize("seed", [0, 777])
@pytest.mark.parametrize("cam", [(2.2, 0.6, 1.1), (-1.5, 0.9, 1.9), (0.3, 0.2, -0.4)])
def test_default_pose_is_the_fixed_camera_exactly(cam, seed):
    W, H, vshape = 9, 7, (16, 20, 12)
    c = torch.tensor(cam, dtype=torch.float64)
    want = CG.ray_setup(c, W, H, vshape, 1.5, jitter_seed=seed, view=2)
    got = PR.ray_setup(c, torch.tensor(PR.ORIGIN), torch.tensor(PR.UP_Y), math.radians(PR.FOV_DEG), W, H, vshape, 1.5,
                       jitter_seed=seed, view=2)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def _objective(inp, theta):
    """sum(raycast * grad_out) of the whole image in float64 as a function of the ten parameters (one pose for all rays), with
    the branches the gradient freezes free to move: finite differences of it are only valid away from where they do."""
    i2 = dict(inp, look_from=theta[0:3], look_at=theta[3:6], up=theta[6:9], fov_rad=theta[9])
    res = PR.run_case(i2)
    return float((res["rgba"] * inp["grad_out"]).sum()), res


def test_reference_gradient_matches_central_differences_of_itself():
    """The autograd gradient of all ten parameters against central differences of the same float64 program, ray by ray, on the
    rays whose frozen decisions (sample count, live samples, picked faces) are the same at both ends of every difference and
    that are away from face ties. h = 1e-6: the truncation error of a central difference is O(h^2) = 1e-12 relative, its
    rounding error 1e-16 / h = 1e-10 of the objective; 1e-6 of the largest gradient component leaves four digits of margin."""
    inp = dict(_scene(), **PANNED)
    theta0 = np.concatenate([np.asarray(PANNED["look_from"]), np.asarray(PANNED["look_at"]), np.asarray(PANNED["up"]),
                             [PANNED["fov_rad"]]]).astype(np.float64)
    _, ref = _objective(inp, theta0)
    per_ray = lambda res: (res["rgba"] * inp["grad_out"]).sum(-1)
    h = 1e-6
    fd = np.zeros_like(ref["dpose_ray"])
    same = ref["n"] > 1
    same &= (PR.face_margin(theta0[:3], ref["rays"], True) > 1e-3) & (PR.face_margin(theta0[:3], ref["rays"], False) > 1e-3)
    for k in range(10):
        tp, tm = theta0.copy(), theta0.copy()
        tp[k] += h; tm[k] -= h
        _, rp = _objective(inp, tp)
        _, rm = _objective(inp, tm)
        fd[..., k] = (per_ray(rp) - per_ray(rm)) / (2.0 * h)
        same &= (rp["n"] == ref["n"]) & (rm["n"] == ref["n"]) & (rp["steps"] == ref["steps"]) & (rm["steps"] == ref["steps"])
    assert same.sum() >= 0.5 * (ref["n"] > 1).sum() and same.sum() >= 8
    scale = np.abs(ref["dpose_ray"][same]).max()
    assert np.abs(fd - ref["dpose_ray"])[same].max() <= 1e-6 * scale
    for k in range(10):   # every parameter is exercised
        assert np.abs(ref["dpose_ray"][same][:, k]).max() > 1e-6 * scale, k


@pytest.mark.parametrize("jitter", [0, 99])
def test_pose_gradient_invariants(jitter):
    """What the camera model implies for every ray, to rounding: the image does not change when look_at slides along the viewing
    direction, when up is scaled, or when up moves along the viewing direction (right = normalize(view_dir x up) does not), and
    moving look_from and look_at together is a translation: its gradient is the sum of the two."""
    inp = dict(_scene(5), **PANNED, jitter_seed=np.int64(jitter))
    res = PR.run_case(inp)
    d = res["dpose_ray"][res["n"] > 1]
    lf, la, up = (np.asarray(PANNED[k], np.float64) for k in ("look_from", "look_at", "up"))
    vdir = (la - lf) / np.linalg.norm(la - lf)
    scale = np.abs(d).max()
    assert np.abs(d[:, 3:6] @ vdir).max() <= 1e-12 * scale
    assert np.abs(d[:, 6:9] @ up).max() <= 1e-12 * scale
    assert np.abs(d[:, 6:9] @ vdir).max() <= 1e-12 * scale
    # the translation gradient against central differences of a common shift of look_from and look_at
    h = 1e-6
    got = d[:, 0:3] + d[:, 3:6]
    keep = np.ones(len(d), bool)
    fd = np.zeros((len(d), 3))
    per_ray = lambda r: (r["rgba"] * inp["grad_out"]).sum(-1)[res["n"] > 1]
    for a in range(3):
        sh = np.zeros(3); sh[a] = h
        rp = PR.run_case(dict(inp, look_from=lf + sh, look_at=la + sh))
        rm = PR.run_case(dict(inp, look_from=lf - sh, look_at=la - sh))
        fd[:, a] = (per_ray(rp) - per_ray(rm)) / (2.0 * h)
        for r in (rp, rm):
            keep &= ((r["n"] == res["n"]) & (r["steps"] == res["steps"]))[res["n"] > 1]
    keep &= (PR.face_margin(lf, res["rays"], True) > 1e-3)[res["n"] > 1] & (PR.face_margin(lf, res["rays"], False) > 1e-3)[res["n"] > 1]
    assert keep.sum() >= 8
    assert np.abs(fd - got)[keep].max() <= 1e-6 * scale


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_projection_reference_default_pose_matches_the_fixed_camera(mode):
    import proj_reference as PJ
    inp = _scene(8)
    inp["grad_out"] = inp["grad_out"][..., 0]
    inp["look_from"] = (1.9, 0.8, -1.3)
    res = PR.run_projection(dict(inp, max_samples=None), mode)
    W, H = inp["grad_out"].shape
    cpp = torch.tensor(inp["look_from"], dtype=torch.float64).expand(W * H, 3).clone().requires_grad_(True)
    out, _, _ = PJ.project_camera(torch.from_numpy(inp["vol"]), cpp, W, H, 1.0, None, mode)
    (out * torch.from_numpy(inp["grad_out"]).reshape(-1)).sum().backward()
    assert np.array_equal(res["out"].reshape(-1), out.detach().numpy())
    want = cpp.grad.numpy().reshape(W, H, 3)
    # look_at at the origin: view_dir depends on look_from alone, as the fixed camera's
    assert np.abs(res["dpose_ray"][..., :3] - want).max() <= 1e-12 * np.abs(want).max()


# ---- the conditioned pass of the GPU tests (pose_gpu.well_conditioned): its conditions, and that it bites -------------------------

def _conditioned_cases():
    """Everything test_gpu_pose.py and test_gpu_pose_edges.py feed to the conditioned pass: id -> a function that returns
    [(ref, ref32, keep, row bands or None)]. The cases of GRAD_RUNS, the float16-rounded volumes among them."""
    import pose_gpu as PG
    import test_gpu_pose as TP
    import test_gpu_pose_edges as TE

    def grad(name, f16):
        _, ref, ref32 = TP.grad_case(name, f16)
        return [(ref, ref32, PG.keep(ref, ref32), None)]

    cases = {"%s_%s" % (name, str(dt)[6:]): (lambda n=name, f=(dt == torch.float16): grad(n, f)) for name, dt in TP.GRAD_RUNS}
    cases.update({"edges_" + k: v for k, v in TE.CONDITIONED.items()})
    return cases


CONDITIONED = _conditioned_cases()


@pytest.mark.parametrize("case", sorted(CONDITIONED))
def test_cases_keep_enough_well_conditioned_rays(case):
    """The rays on which the float32 and the float64 reference agree to 1e-4 of each pose tensor's scale are at least 80 % of
    the n > 1 rays (in every row band where the rule is applied band by band), and err32 over them is within 1e-4 of the scale:
    the second pass of the GPU tests then bounds every ray by 4e-4 of it."""
    import camgrad_gpu as K
    import pose_gpu as PG
    K.check_conditions(CONDITIONED[case](), "dpose_ray", PG.COLUMNS)


def test_the_conditioned_rule_rejects_a_one_percent_error():
    """all_three: one ray puts err32 at 4 % of the scale, and the rule over all rays accepts a pose gradient that is 1 % off
    in every column of every ray. Over the well-conditioned rays it does not."""
    import camgrad_gpu as K
    import pose_gpu as PG
    import test_gpu_pose as TP
    for f16 in (False, True):
        _, ref, ref32 = TP.grad_case("all_three", f16)
        keep = PG.keep(ref, ref32)
        good = PG.well_conditioned(ref, ref32, keep)
        assert good.sum() < (keep & (ref["n"] > 1)).sum()   # there are ill-conditioned rays to leave out
        K.mutation_check(PG.pose_rule, ref["dpose_ray"], ref32["dpose_ray"], ref, ref32, keep, good)


def test_a_view_that_misses_the_box_has_a_zero_reference():
    """look_at = 2 look_from: no ray meets the box, the reference marches nothing and every gradient is 0."""
    inp = dict(_scene(), **PANNED)
    inp["look_at"] = tuple(2.0 * np.asarray(PANNED["look_from"]))
    for dtype in (torch.float64, torch.float32):
        res = PR.run_case(inp, dtype=dtype)
        assert (res["n"] == 0).all() and (res["steps"] == 0).all() and (res["rgba"] == 0).all()
        assert (res["dpose_ray"] == 0).all() and (res["dpose"] == 0).all()


def test_fast_path_hard_poses_see_enough_of_the_box():
    """The premise of test_gpu_pose.py::test_fast_path_serves_a_posed_camera for its hard poses: more than a quarter of the
    pixels of the two cameras have n > 1."""
    import test_gpu_pose as TP
    W, H = TP.FAST_SIZE
    T = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))
    for name, (look_at, up, fovs) in sorted(TP.FAST_HARD_POSES.items()):
        hit = []
        for v in range(2):
            fov = math.radians((fovs or (PR.FOV_DEG,) * 2)[v])
            n = PR.ray_setup(T(TP.CAMS[v]), T(look_at or PR.ORIGIN), T(up or PR.UP_Y), fov, W, H, (40, 24, 36), 1.0)[3]
            hit.append(float((n > 1).double().mean()))
        print("fast path pose", name, "share of n > 1 rays %.2f / %.2f" % tuple(hit))
        assert min(hit) > 0.25, (name, hit)


def test_new_symbols_and_abi_version(hiplib):
    from differender_amd import _native as N
    assert N.ABI_VERSION == 9 and hiplib.dr_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    for name in POSE_ENTRIES:
        assert name in N.SIGNATURES and hasattr(hiplib, name) and name + "(" in header, name
    # the pose entries are the old ones plus (pose, fov_v) -- and d_pose / d_pose_ray in d_cam's place
    for old, new in (("dr_ray_setup_rows", "dr_ray_setup_pose_rows"), ("dr_march_fwd_rows", "dr_march_fwd_rows_pose"),
                     ("dr_march_bwd_rows", "dr_march_bwd_rows_pose"), ("dr_march_bwd_cam", "dr_march_bwd_pose"),
                     ("dr_project_bwd_cam", "dr_project_bwd_pose")):
        assert len(N.SIGNATURES[new][1]) == len(N.SIGNATURES[old][1]) + 2, new


def test_pose_entries_validate_before_any_gpu_call(hiplib):
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(cam=p, V=1, W=4, H=4, img_W=4, row0=0, pose=p, fov_v=None)

    def setup(**kw):
        a = dict(ok, **kw)
        return hiplib.dr_ray_setup_pose_rows(a["cam"], a["V"], a["W"], a["H"], a["img_W"], a["row0"], 8, 8, 8, 0.5, 0.1, 1.0, 0, 0,
                                             p, p, p, p, a["pose"], a["fov_v"], None)

    assert setup(cam=None, pose=None) == -1          # neither a camera nor a pose
    assert setup(pose=None, fov_v=p) == -1           # a per-view fov needs a pose
    assert setup(W=0) == -1 and setup(row0=2) == -1  # the old checks hold
    vol = (p, 0, 8, 8, 8, 64, 8, 1, 0)
    tfa = (p, 4, 0)
    rays = (p, p, p, p, p, 1, 4, 4)
    # dr_march_bwd_pose without a pose; dr_march_fwd_rows_pose with fov_v alone
    assert hiplib.dr_march_bwd_pose(*vol, *tfa, *rays, 64, 1.0, 0.5, 0.1, 0, 0, 4, 0, p, p, p, None, None, p, None, None) == -1
    assert hiplib.dr_march_fwd_rows_pose(*vol, *tfa, *rays, 64, 1.0, 0.5, 0.1, 0, 0, p, None, None, 0, 4, 0, None, p, None) == -1
    assert hiplib.dr_project_bwd_pose(*vol, *rays, 64, 0, 0.5, 0.1, 0, 0, p, None, None, None, p, None, None) == -1


def test_pose_rule_batches_the_pose_with_the_other_inputs():
    from differender_amd import _layout as L
    lf, vol = torch.zeros(3), torch.zeros(1, 4, 4, 4)
    # nothing batched: one view, the pose as single rows
    batched, bs, cam, (la, up, fov) = L.pose_rule(lf, (torch.ones(3), None, 20.0), (vol, 5))
    assert not batched and bs == 0 and cam.shape == (1, 3) and la.shape == (1, 3) and up is None and fov.shape == (1,)
    # a batched look_at alone sets the batch; the others are shared, not copied
    batched, bs, cam, (la, up, fov) = L.pose_rule(lf, (torch.ones(4, 3), torch.ones(3), torch.tensor(20.0)), (vol, 5))
    assert batched and bs == 4 and cam.shape == (4, 3) and la.shape == (4, 3) and up.shape == (4, 3) and fov.shape == (4,)
    assert cam.stride(0) == 0 and up.stride(0) == 0 and fov.stride(0) == 0
    batched, bs, _, (_, _, fov) = L.pose_rule(lf, (None, None, torch.full((3,), 25.0)), (vol, 5))
    assert batched and bs == 3 and fov.shape == (3,)
    with pytest.raises(ValueError, match="disagree"):
        L.pose_rule(torch.zeros(2, 3), (torch.ones(4, 3), None, None), (vol, 5))
    with pytest.raises(ValueError, match="disagree"):
        L.pose_rule(lf, (None, None, torch.ones(3)), (torch.zeros(2, 1, 4, 4, 4), 5))
    with pytest.raises(ValueError, match="look_at"):
        L.pose_rule(lf, (torch.ones(4), None, None), (vol, 5))
    # batch_rule itself is what it was
    assert len(L.batch_rule(lf, (vol, 5))) == 3


def test_all_none_pose_takes_the_old_path(hiplib, monkeypatch):
    """Every renderer with look_at = up = fov = None runs the fixed camera's code: ray_setup, never ray_setup_pose, and no
    pose argument reaches the march. (No GPU here: the first functional call is intercepted.)"""
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    from differender_amd.rgba import RaycasterRGBA
    from differender_amd.tf2d import Raycaster2D
    from differender_amd.volume_raycaster import Raycaster

    class Reached(Exception):
        pass

    def old(*a, **k):
        raise Reached()

    def new(*a, **k):
        raise AssertionError("the pose path ran without a pose")

    monkeypatch.setattr(F, "ray_setup", old)
    monkeypatch.setattr(F, "ray_setup_pose", new)
    vol, vol4, lf = torch.zeros(1, 8, 8, 8), torch.zeros(4, 8, 8, 8), torch.tensor([2.0, 0.5, 1.0])
    rc, r2 = Raycaster((8, 8, 8), (6, 6), 4, jitter=False), Raycaster2D((8, 8, 8), (6, 6), (4, 2), 1.0, jitter=False)
    pj, r4 = Projector((8, 8, 8), (6, 6), jitter=False), RaycasterRGBA((8, 8, 8), (6, 6), jitter=False)
    calls = [lambda: rc(vol, torch.zeros(4, 4), lf), lambda: rc.raycast_nondiff(vol, torch.zeros(4, 4), lf),
             lambda: r2(vol, torch.zeros(4, 4, 2), lf), lambda: r2.raycast_nondiff(vol, torch.zeros(4, 4, 2), lf),
             lambda: pj(vol, lf), lambda: r4(vol4, lf), lambda: r4.raycast_nondiff(vol4, lf),
             lambda: rc(vol, torch.zeros(4, 4), lf, look_at=None, up=None, fov=None)]
    for call in calls:
        with pytest.raises(Reached):
            call()
    # ... and with any one of them the pose path
    monkeypatch.setattr(F, "ray_setup_pose", old)
    monkeypatch.setattr(F, "ray_setup", new)
    posed = [lambda: rc(vol, torch.zeros(4, 4), lf, up=torch.tensor([0.1, 1.0, 0.0])), lambda: pj(vol, lf, fov=25.0),
             lambda: r2(vol, torch.zeros(4, 4, 2), lf, look_at=torch.zeros(3)), lambda: r4.raycast_nondiff(vol4, lf, fov=20.0)]
    for call in posed:
        with pytest.raises(Reached):
            call()


def test_renderers_without_camera_gradients_refuse_a_pose_that_requires_grad(hiplib):
    from differender_amd.rgba import RaycasterRGBA
    from differender_amd.tf2d import Raycaster2D
    lf = torch.tensor([2.0, 0.5, 1.0])
    la = torch.zeros(3, requires_grad=True)
    with pytest.raises(ValueError, match="look_at"):
        RaycasterRGBA((8, 8, 8), (6, 6))(torch.zeros(4, 8, 8, 8), lf, look_at=la)
    with pytest.raises(ValueError, match="fov"):
        Raycaster2D((8, 8, 8), (6, 6), (4, 2), 1.0)(torch.zeros(1, 8, 8, 8), torch.zeros(4, 4, 2), lf,
                                                    fov=torch.tensor(20.0, requires_grad=True))
