"""Which C entries the plain-kernel renderers call, and in which order (tests/entry_log.py records them): the host path between
the modules and the kernels, held to lists written out here. Every module runs with the fixed camera and with a pose, with nothing,
with its volume / table / light and with its camera requiring grad; each gradient comes back in its input's shape and dtype.

The shapes are the smallest that exercise the layout: a volume (D, H, W) = (6, 7, 8), output_shape (5, 9) (ragged, two 8-wide
tiles along one axis), R = 4 and a (4, 3) 2-D table, two views of one un-batched volume (so the shared-input sum runs), no jitter.
With a pose look_from is un-batched too -- the views differ in look_at -- and receives the (3,) sum of the views' gradients."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import entry_log  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, OUT, R, TABLE, BS = (6, 7, 8), (5, 9), 4, (4, 3), 2
DEVICE = "cuda"
CAMERA_ENTRIES = {"dr_march_bwd_cam", "dr_march_bwd_pose", "dr_march_rgba_bwd_cam", "dr_march_rgba_bwd_pose",
                  "dr_march_depth_bwd_cam", "dr_march_depth_bwd_pose", "dr_project_bwd_cam", "dr_project_bwd_pose"}
SETUP = {"fixed": "dr_ray_setup_rows", "posed": "dr_ray_setup_pose_rows"}

# family -> (camera, what requires grad) -> the entries of forward + backward after ray setup. "none": under no_grad; "inputs":
# the volume and the table or light; "camera": look_from as well, and with a pose look_at, up and fov (absent: the module refuses)
EXPECTED = {
    "tf2d": {("fixed", "none"): ["dr_march_tf2d_fwd"],
             ("fixed", "inputs"): ["dr_march_tf2d_fwd", "dr_march_tf2d_bwd"],
             ("posed", "none"): ["dr_march_tf2d_fwd"],
             ("posed", "inputs"): ["dr_march_tf2d_fwd", "dr_march_tf2d_bwd"]},
    "lit": {("fixed", "none"): ["dr_march_lit_fwd"],
            ("fixed", "inputs"): ["dr_march_lit_fwd", "dr_march_lit_bwd"],
            ("posed", "none"): ["dr_march_lit_fwd"],
            ("posed", "inputs"): ["dr_march_lit_fwd", "dr_march_lit_bwd"]},
    "rgba": {("fixed", "none"): ["dr_march_rgba_fwd"],
             ("fixed", "inputs"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd"],
             ("posed", "none"): ["dr_march_rgba_fwd"],
             ("posed", "inputs"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd"]},
    "rgba_camera_grad": {("fixed", "none"): ["dr_march_rgba_fwd"],
                         ("fixed", "inputs"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd"],
                         ("fixed", "camera"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd", "dr_march_rgba_bwd_cam"],
                         ("posed", "none"): ["dr_march_rgba_fwd"],
                         ("posed", "inputs"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd"],
                         ("posed", "camera"): ["dr_march_rgba_fwd", "dr_march_rgba_bwd", "dr_march_rgba_bwd_pose"]},
    "depth": {("fixed", "none"): ["dr_march_depth_fwd"],
              ("fixed", "inputs"): ["dr_march_depth_fwd", "dr_march_depth_bwd"],
              ("posed", "none"): ["dr_march_depth_fwd"],
              ("posed", "inputs"): ["dr_march_depth_fwd", "dr_march_depth_bwd"]},
    "depth_camera_grad": {("fixed", "none"): ["dr_march_depth_fwd"],
                          ("fixed", "inputs"): ["dr_march_depth_fwd", "dr_march_depth_bwd"],
                          ("fixed", "camera"): ["dr_march_depth_fwd", "dr_march_depth_bwd", "dr_march_depth_bwd_cam"],
                          ("posed", "none"): ["dr_march_depth_fwd"],
                          ("posed", "inputs"): ["dr_march_depth_fwd", "dr_march_depth_bwd"],
                          ("posed", "camera"): ["dr_march_depth_fwd", "dr_march_depth_bwd", "dr_march_depth_bwd_pose"]},
    "project_sum": {("fixed", "none"): ["dr_project_fwd"],
                    ("fixed", "inputs"): ["dr_project_fwd", "dr_project_bwd"],
                    ("fixed", "camera"): ["dr_project_fwd", "dr_project_bwd", "dr_project_bwd_cam"],
                    ("posed", "none"): ["dr_project_fwd"],
                    ("posed", "inputs"): ["dr_project_fwd", "dr_project_bwd"],
                    ("posed", "camera"): ["dr_project_fwd", "dr_project_bwd", "dr_project_bwd_pose"]},
    "project_max": {("fixed", "none"): ["dr_project_fwd"],
                    ("fixed", "inputs"): ["dr_project_fwd", "dr_project_bwd"],
                    ("fixed", "camera"): ["dr_project_fwd", "dr_project_bwd", "dr_project_bwd_cam"],
                    ("posed", "none"): ["dr_project_fwd"],
                    ("posed", "inputs"): ["dr_project_fwd", "dr_project_bwd"],
                    ("posed", "camera"): ["dr_project_fwd", "dr_project_bwd", "dr_project_bwd_pose"]},
}
# rc._steps after a forward: the views' (W, H) sample counts in the kernels' layout; the projections keep none
STEPS_SHAPE = {family: None if family.startswith("project") else (BS, *OUT) for family in EXPECTED}
NONDIFF = {"tf2d": "dr_march_tf2d_fwd", "lit": "dr_march_lit_fwd", "rgba": "dr_march_rgba_fwd"}
CASES = [(family, camera, grads) for family, lists in EXPECTED.items() for camera, grads in lists]


def module(family, jitter=False):
    from differender_amd.depth import DepthRaycaster
    from differender_amd.lighting import RaycasterLit
    from differender_amd.projection import Projector
    from differender_amd.rgba import RaycasterRGBA
    from differender_amd.tf2d import Raycaster2D
    return {"tf2d": lambda: Raycaster2D(SHAPE, OUT, TABLE, 1.0, jitter=jitter),
            "lit": lambda: RaycasterLit(SHAPE, OUT, R, jitter=jitter),
            "rgba": lambda: RaycasterRGBA(SHAPE, OUT, jitter=jitter),
            "rgba_camera_grad": lambda: RaycasterRGBA(SHAPE, OUT, jitter=jitter, camera_grad=True),
            "depth": lambda: DepthRaycaster(SHAPE, OUT, R, jitter=jitter),
            "depth_camera_grad": lambda: DepthRaycaster(SHAPE, OUT, R, jitter=jitter, camera_grad=True),
            "project_sum": lambda: Projector(SHAPE, OUT, mode="sum", jitter=jitter),
            "project_max": lambda: Projector(SHAPE, OUT, mode="max", jitter=jitter)}[family]()


def inputs(family, camera, grads):
    """-> (positional inputs before look_from, camera tensors by name, further keyword inputs, {name: tensor that requires grad})."""
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.rand(*shape, generator=gen)
    dev = torch.device(DEVICE)
    channels = 4 if family.startswith("rgba") else 1
    named = {"volume": rand(channels, *SHAPE).to(dev)}
    if family == "tf2d":
        named["table"] = rand(4, *TABLE).to(dev)
    elif family in ("lit", "depth", "depth_camera_grad"):
        named["table"] = (0.1 + 0.5 * rand(4, R)).to(dev)
    extra = {"light_pos": torch.tensor([0.3, 1.0, 0.2], device=dev)} if family == "lit" else {}
    # look_from is float64 where it requires grad: its gradient comes back in that dtype
    lf_dtype = torch.float64 if grads == "camera" else torch.float32
    if camera == "fixed":
        cam = {"look_from": torch.tensor([[2.0, 0.5, 1.0], [-1.5, 1.0, 2.0]], dtype=lf_dtype, device=dev)}
    else:
        cam = {"look_from": torch.tensor([2.0, 0.5, 1.0], dtype=lf_dtype, device=dev),
               "look_at": torch.tensor([[0.1, 0.0, -0.1], [-0.1, 0.05, 0.0]], device=dev),
               "up": torch.tensor([0.1, 1.0, 0.0], device=dev), "fov": torch.tensor(28.0, device=dev)}
    leaves = {}
    if grads != "none":
        leaves.update(named, **extra)
    if grads == "camera":
        leaves.update(cam)
    for t in leaves.values():
        t.requires_grad_(True)
    return list(named.values()), cam, extra, leaves


def run_case(family, camera, grads, log, jitter=False):
    """One forward (+ backward) of the case through `log` -> (the entries' names, rc, image, the leaves that require grad)."""
    rc = module(family, jitter)
    positional, cam, extra, leaves = inputs(family, camera, grads)
    log.take()
    look_from = cam.pop("look_from")
    if grads == "none":
        with torch.no_grad():
            img = rc(*positional, look_from, **extra, **cam)
    else:
        img = rc(*positional, look_from, **extra, **cam)
        weight = torch.rand(img.shape, generator=torch.Generator().manual_seed(6)).to(img.device)
        (img * weight).sum().backward()
    torch.cuda.synchronize()
    return log.take(), rc, img.detach(), leaves


@pytest.mark.parametrize("family,camera,grads", CASES, ids=lambda v: v)
def test_entries_gradient_shapes_and_steps(hiplib, monkeypatch, family, camera, grads):
    log = entry_log.record(monkeypatch)
    names, rc, img, leaves = run_case(family, camera, grads, log)
    assert names == [SETUP[camera]] + EXPECTED[family][(camera, grads)]
    if grads != "camera":
        assert not CAMERA_ENTRIES.intersection(names)
    assert img.shape[0] == BS and torch.isfinite(img).all()
    for name, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, name
    if camera == "posed" and grads == "camera":
        assert leaves["look_from"].grad.shape == (3,)   # un-batched: the sum over the views
    if STEPS_SHAPE[family] is None:
        assert rc._steps is None
    else:
        assert rc._steps.shape == STEPS_SHAPE[family] and rc._steps.dtype == torch.int32


@pytest.mark.parametrize("camera", ["fixed", "posed"])
@pytest.mark.parametrize("family", sorted(NONDIFF))
def test_raycast_nondiff_is_ray_setup_and_one_forward(hiplib, monkeypatch, family, camera):
    log = entry_log.record(monkeypatch)
    rc = module(family)
    positional, cam, extra, _ = inputs(family, camera, "none")
    log.take()
    img = rc.raycast_nondiff(*positional, cam.pop("look_from"), **extra, **cam)
    torch.cuda.synchronize()
    assert log.take() == [SETUP[camera], NONDIFF[family]]
    assert img.shape[0] == BS and rc._steps.shape == (BS, *OUT)
