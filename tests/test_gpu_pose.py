"""The free camera on the GPU: the pose ray setup, the brick-centric fast path under a pose, the pose gradient
of the march and of the projections against the float64 autograd reference (tests/pose_reference.py), and the four renderers."""
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

import pose_gpu as PG  # noqa: E402
import pose_reference as PR  # noqa: E402
from test_setup_nondiff_golden import RAY_TOL, T_TOL  # noqa: E402
from test_gpu_parity import FWD_TOL, grad_close  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = lambda: torch.device("cuda")
CAMS = [(-1.3, 0.9, 2.0), (2.3, 0.5, -0.9), (0.8, -1.1, -2.1)]   # outside the box, off every axis and coordinate plane
SETUP_CAMS = [(1.73, -1.64, -1.85), (-1.6, 1.91, 1.92), (-1.8, -1.9, -1.58)]   # off all three slabs of the box (see the ray-setup test)
# look_at, up, fov (degrees): panned, rolled, zoomed, and all three
POSES = {"panned": ((0.25, -0.15, 0.2), None, None), "rolled": (None, (0.35, 1.0, -0.2), None), "zoomed": (None, None, 21.0),
         "all": ((-0.2, 0.1, 0.15), (-0.3, 0.9, 0.25), 36.0)}


def _pose(cams, look_at=None, up=None):
    from differender_amd import functional as F
    lf = torch.tensor(cams, dtype=torch.float32, device=DEV()).reshape(-1, 3)
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=DEV())
    return F.pack_pose(lf, t(look_at), t(up))


# ---- ray setup ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 4711])
def test_default_pose_gives_the_fixed_cameras_buffers_bitwise(hiplib, seed):
    from differender_amd import functional as F
    cam = torch.tensor(CAMS, device=DEV())
    WH, vshape = (21, 13), (20, 16, 24)
    pose = F.pack_pose(cam)
    for rows, Wb in ((None, WH[0]), ((0, WH[0]), 8), ((8, WH[0]), 13)):
        want = F.ray_setup(cam, (Wb, WH[1]), vshape, 1.5, jitter_seed=seed, view_base=3, rows=rows)
        got = F.ray_setup_pose(pose, (Wb, WH[1]), vshape, 1.5, jitter_seed=seed, view_base=3, rows=rows)
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), rows
    assert (want[3] > 1).float().mean() > 0.2


def test_default_pose_gives_the_old_image_bitwise(hiplib):
    from differender_amd.volume_raycaster import Raycaster
    g = torch.Generator().manual_seed(2)
    vol = (0.3 + 0.4 * torch.rand((1, 24, 26, 28), generator=g)).to(DEV())
    tf = torch.rand((4, 16), generator=g).to(DEV())
    tf[3] = torch.linspace(0.02, 0.2, 16, device=DEV())
    lf = torch.tensor(CAMS[:2], device=DEV())
    rc = Raycaster(vol.shape[-3:], (20, 16), 16, jitter=False, max_samples=4096)
    with torch.no_grad():
        old = rc(vol, tf, lf)
        new = rc(vol, tf, lf, look_at=torch.zeros(3, device=DEV()), up=torch.tensor([0.0, 1.0, 0.0], device=DEV()))
        assert torch.equal(old, new) and float(old.abs().max()) > 0
        assert torch.equal(rc.raycast_nondiff(vol, tf, lf), rc.raycast_nondiff(vol, tf, lf, look_at=torch.zeros(3, device=DEV())))


@pytest.mark.parametrize("seed", [0, 31337])
@pytest.mark.parametrize("name", sorted(POSES))
def test_pose_ray_buffers_match_the_f64_reference(hiplib, name, seed):
    """The rule of tests/test_setup_nondiff_golden.py. Three views per launch: view 0 has the pose under test, the others the
    other cameras with a pose of their own, so that a view reading its neighbour's rows cannot pass.
    The rule's T_TOL presumes well-conditioned rays: a slab distance t = (c - o_a) / vd_a carries the direction's float32 error
    (~1.5e-6 absolute after three normalisations from a 0.1-unit near plane) divided by |vd_a|, and a ray that meets its face
    at a grazing angle (|vd_a| = 0.03 for a camera inside a slab of the box, looking along it) is 3e-5 off in ANY float32
    evaluation. That is a condition on the cases, not a measurement: SETUP_CAMS stand off all three slabs (|vd_a| >= 0.12 on
    every picked face), and the float32 run of the reference itself is held to the rule here before the kernel is."""
    from differender_amd import functional as F
    look_at, up, fov = POSES[name]
    CAMS = SETUP_CAMS
    W, H, vshape, sr, view_base = 18, 14, (20, 24, 16), 1.3, 2
    las = [look_at or PR.ORIGIN, (0.1, 0.2, -0.1), (-0.15, 0.0, 0.1)]
    ups = [up or PR.UP_Y, (0.1, 1.0, 0.0), (-0.2, 1.0, 0.3)]
    fovs = [fov or PR.FOV_DEG, 27.0, 33.0]
    lf = torch.tensor(CAMS, device=DEV())
    pose = F.pack_pose(lf, torch.tensor(las, device=DEV()), torch.tensor(ups, device=DEV()))
    per_view = fov is not None
    fov_v = torch.deg2rad(torch.tensor(fovs, device=DEV())) if per_view else None
    e, x, r, n = (t.cpu().numpy() for t in F.ray_setup_pose(pose, (W, H), vshape, sr, jitter_seed=seed, view_base=view_base, fov_v=fov_v))
    for v in range(3):
        T64 = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))
        fr = float(fov_v[v].cpu()) if per_view else math.radians(PR.FOV_DEG)
        e0, x0, r0, n0 = (t.numpy() for t in PR.ray_setup(T64(CAMS[v]), T64(las[v]), T64(ups[v]), fr, W, H, vshape, sr,
                                                           jitter_seed=seed, view=view_base + v))
        e0, x0, r0, n0 = e0.reshape(W, H), x0.reshape(W, H), r0.reshape(W, H, 3), n0.reshape(W, H)
        hit = n0 > 0
        assert hit.mean() > 0.2, (name, v)
        T32 = lambda a: torch.tensor(np.asarray(a, np.float32))
        e32, x32 = (t.double().numpy().reshape(W, H) for t in PR.ray_setup(T32(CAMS[v]), T32(las[v]), T32(ups[v]), fr, W, H, vshape, sr,
                                                                             jitter_seed=seed, view=view_base + v)[:2])
        for a32, a0 in ((e32, e0), (x32, x0)):   # the condition on the case
            assert (np.abs(a32 - a0)[hit] <= T_TOL * np.maximum(np.abs(a0[hit]), 1.0)).all(), "ill-conditioned case: move the camera"
        assert np.abs(n[v].astype(np.int64) - n0).max() <= 1 and (n[v] == n0).mean() >= 0.97 and (n[v] == n0)[~hit].all()
        assert np.abs(r[v] - r0).max() <= RAY_TOL
        assert (np.abs(e[v] - e0)[hit] <= T_TOL * np.maximum(np.abs(e0[hit]), 1.0)).all()
        assert (np.abs(x[v] - x0)[hit] <= T_TOL * np.maximum(np.abs(x0[hit]), 1.0)).all()
    # a band of the image is the rows of the whole image, bit for bit
    band = F.ray_setup_pose(pose, (7, H), vshape, sr, jitter_seed=seed, view_base=view_base, fov_v=fov_v, rows=(5, W))
    for a, b in zip(band, (e, x, r, n)):
        assert np.array_equal(a.cpu().numpy(), b[:, 5:12])


# ---- the fast path under a pose --------------------------------------------------------------------------------------------------

def _fast_scene(oracle, R=64):
    vol = torch.from_numpy(oracle.synth_volume((40, 24, 36))).to(DEV())
    tf = torch.from_numpy(oracle.bench_tf(R, 0.03)).to(DEV())
    return vol, tf


def _fast_and_baseline(vol, tf, pose, fov_v, WH, sr=1.0, seed=0, rows=None, S=1 << 20):
    """Forward and backward of the brick-centric path under the pose and of the plain kernels on the same buffers.
    -> dict of both sides' out, steps, d_vol, d_tf, the forward's workspace header, n."""
    from differender_amd import _native as N
    from differender_amd import functional as F
    V = pose.shape[0]
    Wb = WH[0] if rows is None else rows[2]
    rr = None if rows is None else rows[:2]
    e, x, r, n = F.ray_setup_pose(pose, (Wb, WH[1]), vol.shape, sr, jitter_seed=seed, fov_v=fov_v, rows=rr)
    cam = pose[:, :3].contiguous()
    ws = F.alloc_workspace(V, (Wb, WH[1]), vol.shape, tf.shape[0], vol.device)
    assert ws is not None
    out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, workspace=ws, rows=rr, pose=pose, fov_v=fov_v)
    stats = F.workspace_stats(ws).numpy().copy()
    # (a band's upstream gradient is the band of the whole image's)
    g = torch.randn((V, *WH, 4), generator=torch.Generator().manual_seed(11)).to(vol.device)
    g = g if rows is None else g[:, rr[0]:rr[0] + Wb].contiguous()
    dv, dt = F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out, workspace=ws, rows=rr, pose=pose, fov_v=fov_v)
    stale = int(F.workspace_stats(ws)[9])
    outb, stepsb = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, variant=N.DR_VARIANT_BASELINE, workspace=None, rows=rr)
    dvb, dtb = F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, outb, variant=N.DR_VARIANT_BASELINE, rows=rr)
    torch.cuda.synchronize()
    return dict(out=out, steps=steps, dv=dv, dt=dt, outb=outb, stepsb=stepsb, dvb=dvb, dtb=dtb, stats=stats, n=n, stale=stale)


def _check_fast(res, what, heavy=None):
    st, n = res["stats"], res["n"]
    irregular = int((n <= 1).sum())
    print("pose fast path", what, "repaired", st[0], "per-ray", st[2], "irregular", irregular, "exact", st[15], "items", st[5])
    assert st[0] == 0, (what, "rays fell off the fast path", int(st[0]))
    assert st[2] <= irregular + st[15], (what, int(st[2]), irregular, int(st[15]))
    assert res["stale"] == 0, what                       # the backward found its forward's records
    if heavy is not None:
        assert (st[5] > 0) == heavy, (what, int(st[5]))
    # fast against baseline by tests/test_gpu_parity.py's rules: the same live samples, images to FWD_TOL, gradients by grad_close
    assert torch.equal(res["steps"], res["stepsb"]), what
    assert float((res["out"] - res["outb"]).abs().max()) <= FWD_TOL, what
    assert float(res["outb"].abs().max()) > 0.05
    for k in ("dv", "dt"):
        ok, err = grad_close(res[k].cpu().numpy(), res[k + "b"].cpu().numpy())
        assert ok, (what, k, err)


# look_at, up, fov of the two views (degrees): the hard poses of the fast path. The share of n > 1 rays of the two cameras was
# checked on the CPU (pose_reference.ray_setup): 0.68 / 0.80, 0.69 / 0.80, 1.0 / 1.0, 0.53 / 0.60.
FAST_HARD_POSES = {"upside_down": (None, (0.0, -1.0, 0.0), None), "roll_90": (None, (1.0, 0.05, 0.0), None),
                   "narrow": (None, None, (8.0, 6.0)), "half_off": ((0.9, 0.6, -0.4), None, None)}
FAST_SIZE = (48, 40)


@pytest.mark.parametrize("name", ["panned", "rolled", "all"] + sorted(FAST_HARD_POSES))
def test_fast_path_serves_a_posed_camera(hiplib, oracle, name):
    """The test that fails if only the ray setup learns the pose: with the fixed camera's brick rectangles the rays of a panned
    or rolled camera fail the sample-count check (workspace_stats[0]) and are marched one by one."""
    if name in FAST_HARD_POSES:
        look_at, up, fovs = FAST_HARD_POSES[name]
    else:
        look_at, up, fov = POSES[name]
        fovs = None if fov is None else (fov, fov - 8.0)
    vol, tf = _fast_scene(oracle)
    pose = _pose(CAMS[:2], look_at, up)
    fov_v = None if fovs is None else torch.deg2rad(torch.tensor(fovs, device=DEV()))
    res = _fast_and_baseline(vol, tf, pose, fov_v, FAST_SIZE, seed=77 if name == "all" else 0)
    assert (res["n"] > 1).float().mean() > 0.25
    _check_fast(res, name)


def test_fast_path_with_the_camera_inside_the_box(hiplib, oracle):
    """64 x 48 from inside: bricks next to the eye cover more than 1024 candidate pixels, their overflow items go through the
    line pre-test that make_cam_basis feeds (workspace_stats[5] > 0)."""
    vol, tf = _fast_scene(oracle)
    pose = _pose([(0.3, 0.2, -0.4)], (-0.4, 0.1, 0.5), (0.4, 1.0, 0.2))
    res = _fast_and_baseline(vol, tf, pose, torch.deg2rad(torch.tensor([38.0], device=DEV())), (64, 48))
    _check_fast(res, "inside", heavy=True)


def test_fast_path_row_bands_add_up_under_a_pose(hiplib, oracle):
    vol, tf = _fast_scene(oracle)
    pose = _pose(CAMS[1:2], *POSES["all"][:2])
    fov_v = torch.deg2rad(torch.tensor([POSES["all"][2]], device=DEV()))
    WH = (48, 40)
    whole = _fast_and_baseline(vol, tf, pose, fov_v, WH, seed=5)
    _check_fast(whole, "whole")
    bands = [_fast_and_baseline(vol, tf, pose, fov_v, WH, seed=5, rows=(r0, WH[0], wb)) for r0, wb in ((0, 17), (17, 16), (33, 15))]
    for k, b in enumerate(bands):
        _check_fast(b, ("band", k))
    assert torch.equal(torch.cat([b["steps"] for b in bands], 1), whole["steps"])
    assert float((torch.cat([b["out"] for b in bands], 1) - whole["out"]).abs().max()) <= FWD_TOL
    for k in ("dv", "dt"):
        ok, err = grad_close(sum(b[k] for b in bands).cpu().numpy(), whole[k].cpu().numpy())
        assert ok, (k, err)


# ---- the pose gradient against the float64 reference -----------------------------------------------------------------------------

# scene (a case of make_camgrad_golden.CASES), then what is laid over it. The cameras were checked on the CPU (the float32 run of
# the reference against the float64 one): at least 80 % of the n > 1 rays keep their sample count and live samples.
GRAD_CASES = {
    "look_at_off_centre": ("a_orbit_sr1", dict(look_at=(0.25, -0.15, 0.2))),
    "roll": ("e_nonsquare", dict(up=(0.35, 1.0, -0.2))),
    "per_view_fov": ("a_orbit_sr1", dict(fov_rad=math.radians(23.0))),
    # (34 degrees: at 36 only 75 of the 92 n > 1 rays were well-conditioned, one ray from the cap, and 72 with the float32
    # reference of another CPU; here 104 of 112, and one ray still puts err32 at 4 % of the scale)
    "all_three": ("l_anisotropic", dict(look_at=(-0.2, 0.1, 0.15), up=(-0.3, 0.9, 0.25), fov_rad=math.radians(34.0))),
    "inside": ("j_inside", dict(look_at=(-0.3, 0.05, 0.4), up=(0.3, 1.0, 0.1), fov_rad=math.radians(34.0))),
    "jitter": ("d_jitter", dict(look_at=(0.1, 0.2, -0.15), up=(0.2, 1.0, 0.1))),
    "early_termination_sr2": ("b_sr2_ert", dict(look_at=(0.15, -0.1, 0.1), up=(-0.25, 1.0, 0.15), fov_rad=math.radians(27.0))),
    "max_samples_clip": ("c_clip", dict(look_at=(-0.1, 0.15, 0.1), up=(0.15, 1.0, -0.3))),
    # hard poses: the camera upside down, rolled by a quarter and by three eighths of a turn (right and up' swap roles and
    # signs in pose_ray_grad), a 5 degree zoom (near_h, and with it d fov, 1/7 of the default's), a wide angle on a 24 x 24
    # image (the box fills a third of it), the box half off the image and in one corner of it (26 rays). Each keeps its share
    # of well-conditioned rays (tests/test_pose.py).
    "upside_down": ("e_nonsquare", dict(up=(0.0, -1.0, 0.0))),
    "roll_90": ("e_nonsquare", dict(up=(1.0, 0.05, 0.0))),
    "roll_135": ("a_orbit_sr1", dict(up=(0.7, -0.7, 0.1))),
    "narrow_5deg": ("a_orbit_sr1", dict(fov_rad=math.radians(5.0))),
    "wide_45deg": ("a_orbit_sr1", dict(fov_rad=math.radians(45.0), WH=(24, 24))),
    "half_off": ("e_nonsquare", dict(look_at=(0.9, 0.6, -0.4))),
    "corner_only": ("a_orbit_sr1", dict(look_at=(1.6, 1.2, 0.3), fov_rad=math.radians(25.0))),
}


# every case with a float32 volume, two of them with a float16 one as well
GRAD_RUNS = [(name, torch.float32) for name in sorted(GRAD_CASES)] + [("all_three", torch.float16), ("early_termination_sr2", torch.float16)]


@functools.lru_cache(maxsize=None)
def grad_case(name, f16):
    """(inputs, float64 reference, float32 reference) of a case, computed once and shared (read only)."""
    scene, over = GRAD_CASES[name]
    inp = PG.inputs(scene, **over)
    if f16:   # the reference on the f16-rounded volume the kernel reads
        inp["vol"] = PG.F16(inp["vol"])
    return (inp,) + PG.refs(inp)


@pytest.mark.parametrize("name,vol_dtype", GRAD_RUNS, ids=lambda v: v if isinstance(v, str) else str(v)[6:])
def test_march_bwd_pose_matches_the_f64_reference(hiplib, name, vol_dtype):
    inp, ref, ref32 = grad_case(name, vol_dtype == torch.float16)
    if name == "early_termination_sr2":
        assert ((ref["steps"] < ref["n"]) & (ref["n"] > 1)).sum() > 20
    if name == "max_samples_clip":
        assert (ref["n"] > int(inp["max_samples"])).sum() > 20
    if name == "inside":
        assert (ref["entry"] < 0).all() and (ref["n"] > 1).all()
    ray, total, mask = PG.both_passes(inp, ref, ref32, vol_dtype, (name, str(vol_dtype)))
    for _, sl in PG.COLUMNS:   # every tensor has a gradient in every case (d up and d fov are there under the default pose too)
        assert np.abs(ray[..., sl]).max() > 0


def test_look_from_columns_under_the_default_pose_are_march_bwd_cams(hiplib):
    """With look_at = 0 and up = +y the look_from columns are the fixed camera's gradient. The two kernels share the per-sample
    sums bit for bit but not the tail: march_bwd_cam carries the 3x3 Jacobian forward (ray_dir_jacobian), the pose kernel runs
    the same chain in reverse (pose_ray_grad), so the columns agree to float32 rounding of the tail, not bitwise. The bound is
    D8's own per-ray slack, 1e-4 of the largest component, without the reference's 3 err32: both sides are float32."""
    import camgrad_gpu as K
    import make_camgrad_golden as CG
    inp = PG.inputs("d_jitter")
    ref, ref32 = PG.refs(inp)
    keep = PG.keep(ref, ref32)
    ray, total, mask = PG.hip_per_ray(inp, ref, torch.float32, keep)
    cinp = dict(inp, cam=inp["look_from"])
    cref = dict(ref, dcam_ray=ref["dpose_ray"][..., :3])
    cray, ctotal, cmask = K.hip_per_ray(cinp, cref, torch.float32, keep)
    assert np.array_equal(mask, cmask) and mask.sum() > 0.8 * (ref["n"] > 1).sum()
    scale = np.abs(cray).max()
    assert np.abs(ray[..., :3] - cray).max() <= 1e-4 * scale
    assert np.abs(total[:3] - ctotal).max() <= 1e-5 * np.abs(cray).sum()
    assert np.abs(ray[..., 3:]).max() > 0


# ---- the projections ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 2024])
@pytest.mark.parametrize("mode", ["sum", "max"])
def test_project_bwd_pose_matches_the_f64_reference(hiplib, mode, seed):
    from differender_amd import functional as F
    inp = PG.inputs("l_anisotropic", look_at=(-0.2, 0.1, 0.15), up=(-0.3, 0.9, 0.25), fov_rad=math.radians(33.0),
                    jitter_seed=np.int64(seed))
    inp["grad_out"] = inp["grad_out"][..., 0]
    inp["max_samples"] = None
    ref = PR.run_projection(inp, mode)
    W, H = ref["n"].shape
    poses, fov = PG.pose_rows([inp])
    pose, fov_v = PG.dev(poses), PG.dev(fov)
    vol = PG.dev(inp["vol"])
    rays = [PG.dev(ref[k][None], torch.int32 if k == "n" else torch.float32) for k in ("entry", "exit", "rays", "n")]
    out, arg = F.project_fwd(vol, pose[:, :3].contiguous(), *rays, None, mode)
    keep = ref["n"] > 1
    if mode == "max":   # the gradient goes through the kernel's own frozen argmax: the reference takes it from there
        a = arg[0].cpu().numpy()
        ref = PR.run_projection(inp, mode, arg_max=a)
        ref32 = PR.run_projection(inp, mode, dtype=torch.float32, arg_max=a)
    else:
        ref32 = PR.run_projection(inp, mode, dtype=torch.float32)
    keep &= ref32["n"] == ref["n"]
    g = PG.dev((inp["grad_out"] * keep)[None])
    d, d_ray = F.project_bwd_pose(vol, pose, *rays, g, None, mode, arg, jitter_seed=seed, view_base=int(inp["view"]), per_ray=True,
                                  fov_v=fov_v)
    torch.cuda.synchronize()
    PG.pose_rule(d_ray[0].double().cpu().numpy(), d[0].double().cpu().numpy(), ref, ref32, keep, ("project", mode, seed))


# ---- the modules ----------------------------------------------------------------------------------------------------------------------

def _module_scene(batched_vol, R=16, N=22):
    g = torch.Generator().manual_seed(7)
    vol = (0.3 + 0.4 * torch.rand((2 if batched_vol else 1, 1, N, N + 2, N + 4), generator=g)).to(DEV())
    tf = torch.rand((4, R), generator=g).to(DEV())
    tf[3] = torch.linspace(0.02, 0.12, R, device=DEV())
    return (vol if batched_vol else vol[0]), tf


@pytest.mark.parametrize("kind", ["single", "batched", "shared_pose_batched_vol"])
def test_raycaster_pose_grads_have_the_inputs_shapes_and_sums(hiplib, kind):
    from differender_amd import functional as F
    from differender_amd.volume_raycaster import Raycaster
    vol0, tf0 = _module_scene(kind == "shared_pose_batched_vol")
    WH = (20, 16)
    rc = Raycaster(vol0.shape[-3:], WH, tf0.shape[-1], jitter=False, max_samples=4096)
    t = lambda a: torch.tensor(a, device=DEV())
    if kind == "batched":   # look_from and fov per view, look_at and up shared
        lf0, fov0 = t([CAMS[0], CAMS[1]]), t([26.0, 33.0])
    else:
        lf0, fov0 = t(CAMS[0]), t(28.0)
    la0, up0 = t([0.2, -0.1, 0.15]), t([0.3, 1.0, -0.2])
    bs = 2 if kind != "single" else 0
    w = torch.randn(((bs,) if bs else ()) + (4, WH[1], WH[0]), generator=torch.Generator().manual_seed(3)).to(DEV())
    leaves = [x.clone().requires_grad_(True) for x in (lf0, la0, up0, fov0)]
    vol, tf = vol0.clone().requires_grad_(True), tf0.clone().requires_grad_(True)
    (rc(vol, tf, leaves[0], look_at=leaves[1], up=leaves[2], fov=leaves[3]) * w).sum().backward()
    for leaf, x0 in zip(leaves, (lf0, la0, up0, fov0)):
        assert leaf.grad is not None and leaf.grad.shape == x0.shape and leaf.grad.dtype == x0.dtype
        assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert vol.grad is not None and tf.grad is not None

    # the same through the functional API: grad_out is w mapped back through Raycaster's flip / permute
    batched, _, vol_in, tf_in, lf_in, (la, up, fov) = rc._determine_batch(vol0, tf0, lf0, (la0, up0, fov0))
    pose = F.pack_pose(lf_in.reshape(-1, 3).expand(max(bs, 1), 3), la, up)
    fov_v = torch.deg2rad(fov).contiguous()
    g = (w.flip(-2).permute(0, 3, 2, 1) if batched else w.flip(-2).permute(2, 1, 0)[None]).contiguous()
    e, x, r, n = F.ray_setup_pose(pose, WH, vol_in.shape[-3:], 1.0, fov_v=fov_v)
    tfc = tf_in.float().contiguous()
    out, steps = F.march_fwd(vol_in, tfc, pose[:, :3].contiguous(), e, x, r, n, 4096, 1.0, pose=pose, fov_v=fov_v)
    d = F.march_bwd_pose(vol_in, tfc, pose, e, x, r, n, steps, 4096, 1.0, g, out, fov_v=fov_v)
    per_degree = math.pi / 180.0
    want = [d[:, 0:3], d[:, 3:6].sum(0), d[:, 6:9].sum(0), d[:, 9] * per_degree]   # shared look_at and up: the sum over the views
    if kind != "batched":
        want[0], want[3] = want[0].sum(0), want[3].sum(0)
    for leaf, ww in zip(leaves, want):
        assert torch.allclose(leaf.grad, ww.reshape(leaf.shape), rtol=1e-5, atol=1e-6 * float(ww.abs().max())), kind


def test_projector_pose_grads(hiplib):
    from differender_amd import functional as F
    from differender_amd.projection import Projector
    vol0, _ = _module_scene(False)
    WH = (18, 14)
    pj = Projector(vol0.shape[-3:], WH, mode="sum", jitter=False)
    t = lambda a: torch.tensor(a, device=DEV())
    lf0, la0, up0, fov0 = t([CAMS[0], CAMS[2]]), t([0.2, -0.1, 0.15]), t([[0.3, 1.0, -0.2], [-0.1, 1.0, 0.2]]), t(29.0)
    leaves = [x.clone().requires_grad_(True) for x in (lf0, la0, up0, fov0)]
    w = torch.randn((2, 1, WH[1], WH[0]), generator=torch.Generator().manual_seed(4)).to(DEV())
    (pj(vol0, leaves[0], look_at=leaves[1], up=leaves[2], fov=leaves[3]) * w).sum().backward()
    batched, vol_in, lf_in, (la, up, fov) = pj._determine_batch(vol0, lf0, (la0, up0, fov0))
    pose, fov_v = F.pack_pose(lf_in, la, up), torch.deg2rad(fov).contiguous()
    rays = F.ray_setup_pose(pose, WH, vol_in.shape[-3:], 1.0, fov_v=fov_v)
    g = w[:, 0].flip(-2).permute(0, 2, 1).contiguous()
    d = F.project_bwd_pose(vol_in, pose, *rays, g, None, "sum", None, fov_v=fov_v)
    want = [d[:, 0:3], d[:, 3:6].sum(0), d[:, 6:9], (d[:, 9] * (math.pi / 180.0)).sum(0)]
    for leaf, ww in zip(leaves, want):
        assert leaf.grad.shape == leaf.shape
        assert torch.allclose(leaf.grad, ww.reshape(leaf.shape), rtol=1e-5, atol=1e-6 * float(ww.abs().max()))


def test_tf2d_and_rgba_render_a_posed_camera(hiplib):
    """Raycaster2D and RaycasterRGBA under a panned, rolled, zoomed pose: the image of their march on the pose's ray buffers, the
    volume gradient flowing, and a pose that requires grad refused."""
    from differender_amd import _native as N
    from differender_amd import functional as F
    from differender_amd import _layout as L
    from differender_amd.rgba import RaycasterRGBA
    from differender_amd.tf2d import Raycaster2D
    vol0, _ = _module_scene(False)
    WH = (18, 14)
    t = lambda a: torch.tensor(a, device=DEV())
    lf, la, up, fov = t(CAMS[1]), t([0.2, -0.1, 0.15]), t([0.3, 1.0, -0.2]), t(24.0)
    pose, fov_v = F.pack_pose(lf, la, up), torch.deg2rad(fov).reshape(1)
    g = torch.Generator().manual_seed(9)
    tf2 = torch.rand((4, 8, 3), generator=g).to(DEV())
    tf2[3] *= 0.2
    r2 = Raycaster2D(vol0.shape[-3:], WH, (8, 3), 40.0, jitter=False, max_samples=4096)
    vol = vol0.clone().requires_grad_(True)
    img = r2(vol, tf2, lf, look_at=la, up=up, fov=fov)
    rays = F.ray_setup_pose(pose, WH, L.field_view(vol0).shape, 1.0, fov_v=fov_v)
    want, _ = F.march_tf2d_fwd(L.field_view(vol0), tf2.movedim(0, -1).contiguous(), pose[:, :3].contiguous(), *rays, 4096, 1.0, 40.0)
    assert torch.equal(img, L.image(want[0])) and float(img.detach().abs().max()) > 0
    assert not torch.equal(img, r2(vol0, tf2, lf))
    img.sum().backward()
    assert vol.grad is not None and float(vol.grad.abs().max()) > 0
    assert torch.equal(r2.raycast_nondiff(vol0, tf2, lf, 1.0, look_at=la, up=up, fov=fov),
                       L.image(F.march_tf2d_fwd(L.field_view(vol0), tf2.movedim(0, -1).contiguous(), pose[:, :3].contiguous(), *rays,
                                                4096, 1.0, 40.0, N.DR_MODE_NONDIFF)[0][0]))
    with pytest.raises(ValueError, match="up"):
        r2(vol0, tf2, lf, up=up.clone().requires_grad_(True))

    vol4 = torch.rand((4, *vol0.shape[-3:]), generator=g).to(DEV())
    vol4[3] *= 0.1
    r4 = RaycasterRGBA(vol0.shape[-3:], WH, jitter=False, max_samples=4096)
    v4 = vol4.clone().requires_grad_(True)
    img4 = r4(v4, lf, look_at=la, up=up, fov=fov)
    want4, _ = F.march_rgba_fwd(L.field_view_rgba(vol4), pose[:, :3].contiguous(), *rays, 4096, 1.0)
    assert torch.equal(img4, L.image(want4[0])) and float(img4.detach().abs().max()) > 0
    img4.sum().backward()
    assert float(v4.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="fov"):
        r4(vol4, lf, fov=fov.clone().requires_grad_(True))


def test_pose_recovery_example(hiplib):
    """examples/pose_opt_synthetic.py at a small size, from a start that is off in position, pan, roll and zoom at once: the
    reprojection error of the box's corners, the rotation between the camera frames, the fov error and the loss all end below
    where they started. The position error alone is printed, not asserted: from one image the distance along the viewing
    direction trades against the fov (a dolly zoom), so it is not identified on its own; the reprojection error holds the two
    together."""
    sys.path.insert(0, ROOT)
    from examples.pose_opt_synthetic import main
    res = main(["--vol", "48", "--img", "48", "--tf-res", "32", "--iterations", "60", "--quiet"])
    first, last, losses = res["errors"][0], res["errors"][-1], res["losses"]
    print("pose recovery (reprojection, position, rotation, fov)", first, "->", last, "loss", losses[0], "->", losses[-1])
    for k in (0, 2, 3):
        assert last[k] < first[k], (k, first, last)
    assert losses[-1] < losses[0]
