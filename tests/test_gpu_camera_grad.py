"""Camera-position gradient on the GPU (camera_grad_kernel) against the float64 autograd reference
(tests/golden/camgrad_*.npz, make_camgrad_golden.py), through the functional API, Raycaster, row bands, a user-sized scene
and the pose-recovery example."""
import functools
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "camgrad_*.npz")))

import camgrad_gpu as K  # noqa: E402
from camgrad_gpu import hip_per_ray as _hip_per_ray  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture_case(path, f16):
    """(inputs, float64 reference, float32 reference, keep mask) of a fixture, computed once and shared (read only)."""
    import make_camgrad_golden as CG
    d = np.load(path)
    inp = {k: d[k] for k in ("vol", "tf", "cam", "grad_out", "sr", "max_samples", "jitter_seed", "view")}
    if f16:   # the reference on the f16-rounded volume the kernel reads
        inp["vol"] = inp["vol"].astype(np.float16).astype(np.float64)
        ref = CG.run_case(inp)
    else:
        ref = {k: d[k] for k in ("entry", "exit", "rays", "n", "steps", "dcam_ray")}
    ref32 = CG.run_case(inp, dtype=torch.float32)
    return inp, K.with_kinks(inp, ref), ref32, ref32["steps"] == ref["steps"]


@pytest.mark.parametrize("vol_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_march_bwd_cam_matches_the_f64_reference(hiplib, path, vol_dtype):
    """D8's rule (camgrad_gpu.d8_rule: per ray err <= 3 err32 + 1e-4 scale, the workgroup sums and the one atomic per workgroup
    adding up to the rays' own contributions, the total against the float64 sum), over all compared rays and then again over
    the rays on which the two references agree (camgrad_gpu.well_conditioned), where err32 no longer hides anything."""
    inp, ref, ref32, keep = fixture_case(path, vol_dtype == torch.float16)
    what = (os.path.basename(path)[8:-4], str(vol_dtype))
    ray, total, mask = K.hip_per_ray(inp, ref, vol_dtype, keep)
    K.d8_rule(ray, total, ref, ref32, mask, what)
    good = K.well_conditioned(ref, ref32, keep, what=what)
    ray, total, mask = K.hip_per_ray(inp, ref, vol_dtype, keep & good)
    K.d8_rule(ray, total, ref, ref32, mask, what + ("conditioned",))


def _scene(batched_vol, R=16, N=24):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(7)
    vol = (0.3 + 0.4 * torch.rand((2 if batched_vol else 1, 1, N, N + 2, N + 4), generator=g)).to(dev)
    if not batched_vol:
        vol = vol[0]
    tf = torch.rand((4, R), generator=g).to(dev)
    tf[3] = torch.linspace(0.02, 0.12, R, device=dev)
    return vol, tf


@pytest.mark.parametrize("kind", ["single", "batched", "shared_cam_batched_vol"])
def test_raycaster_look_from_grad(hiplib, kind):
    from differender_amd import functional as F
    from differender_amd.volume_raycaster import Raycaster
    dev = torch.device("cuda")
    vol0, tf0 = _scene(kind == "shared_cam_batched_vol")
    WH = (20, 16)
    rc = Raycaster(vol0.shape[-3:], WH, tf0.shape[-1], jitter=False, max_samples=4096)
    if kind == "batched":
        lf0 = torch.stack([torch.tensor([2.2, 0.6, 1.1]), torch.tensor([-1.5, 0.9, 1.9])]).to(dev)
    else:
        lf0 = torch.tensor([2.2, 0.6, 1.1], device=dev)
    bs = 2 if kind != "single" else 0
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(((bs,) if bs else ()) + (4, WH[1], WH[0]), generator=gen).to(dev)

    def run(cam_grad):
        vol, tf, lf = vol0.clone().requires_grad_(True), tf0.clone().requires_grad_(True), lf0.clone().requires_grad_(cam_grad)
        (rc(vol, tf, lf) * w).sum().backward()
        return vol.grad, tf.grad, lf.grad

    dv1, dt1, dl1 = run(True)
    dv0, dt0, dl0 = run(False)
    assert dl0 is None and dl1 is not None and dl1.shape == lf0.shape
    for a, b in ((dv1, dv0), (dt1, dt0)):   # unchanged by the camera gradient (float atomics: order only)
        assert (a - b).abs().max() <= 1e-6 * b.abs().max()

    # the same through the functional API: grad_out is w mapped back through Raycaster's flip / permute
    batched, _, vol_in, tf_in, lf_in = rc._determine_batch(vol0, tf0, lf0)
    cam = lf_in.reshape(-1, 3).float().contiguous()
    g = (w.flip(-2).permute(0, 3, 2, 1) if batched else w.flip(-2).permute(2, 1, 0)[None]).contiguous()
    e, x, r, n = F.ray_setup(cam, WH, vol_in.shape[-3:], 1.0)
    tfc = tf_in.float().contiguous()
    out, steps = F.march_fwd(vol_in, tfc, cam, e, x, r, n, 4096, 1.0)
    d = F.march_bwd_cam(vol_in, tfc, cam, e, x, r, n, steps, 4096, 1.0, g, out)
    if kind == "single":
        d = d[0]
    elif kind == "shared_cam_batched_vol":
        d = d.sum(0)
    assert torch.allclose(dl1, d, rtol=1e-5, atol=1e-6 * float(d.abs().max()))


def test_row_bands_add_up(hiplib):
    from differender_amd import functional as F
    dev = torch.device("cuda")
    vol, tf = _scene(False, N=32)
    vol = vol[0].permute(2, 0, 1)
    tf = tf.t().contiguous()
    cam = torch.tensor([[1.9, 0.7, 1.7]], device=dev)
    Wimg, H, seed = 30, 22, 987
    g = torch.randn((1, Wimg, H, 4), generator=torch.Generator().manual_seed(5)).to(dev)

    def part(row0, Wb):
        rows = (row0, Wimg)
        e, x, r, n = F.ray_setup(cam, (Wb, H), vol.shape, 1.0, jitter_seed=seed, rows=rows)
        out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, 4096, 1.0, rows=rows)
        return F.march_bwd_cam(vol, tf, cam, e, x, r, n, steps, 4096, 1.0, g[:, row0:row0 + Wb].contiguous(), out,
                               jitter_seed=seed, rows=rows, per_ray=True)

    whole, whole_ray = part(0, Wimg)
    bands = [part(r0, wb) for r0, wb in ((0, 11), (11, 9), (20, 10))]
    total = sum(b[0] for b in bands)
    assert (total - whole).abs().max() <= 1e-5 * whole_ray.abs().sum()
    # same rays; the forward images of a band and of the whole image may differ in their last bits (brick partials)
    assert (torch.cat([b[1] for b in bands], 1) - whole_ray).abs().max() <= 1e-5 * whole_ray.abs().max()


def test_user_sized_scene_matches_the_f64_reference(hiplib):
    """256^3, 256^2, in_circles camera, the bench TF, rate 1: 512 random rays against the float64 autograd reference."""
    import make_camgrad_golden as CG
    from oracle import oracle as O
    N, WH, R = 256, (256, 256), 256
    alpha = 3.0 / (2.0 * math.sqrt(3.0) * math.sqrt(3.0) * (N - 1))
    inp = dict(vol=O.synth_volume(N, dtype=np.float64), tf=O.bench_tf(R, alpha, np.float64),
               cam=O.in_circles(0.9).astype(np.float64), sr=np.float64(1.0), max_samples=np.int32(1 << 20),
               jitter_seed=np.int64(0), view=np.int32(0))
    inp["grad_out"] = np.random.RandomState(9).standard_normal((*WH, 4))
    pixels = np.random.RandomState(10).choice(WH[0] * WH[1], 512, replace=False)
    ref = CG.run_case(inp, pixels=pixels)
    ref32 = CG.run_case(inp, dtype=torch.float32, pixels=pixels)
    sel = np.zeros(WH[0] * WH[1], bool); sel[pixels] = True
    sel = sel.reshape(WH) & (ref["n"] > 1)
    ray, _, mask = _hip_per_ray(inp, ref, torch.float32, sel & (ref32["steps"] == ref["steps"]))
    assert mask.sum() > 400
    scale = np.abs(ref["dcam_ray"][mask]).max()
    err = np.abs(ray - ref["dcam_ray"])[mask].max()
    err32 = np.abs(ref32["dcam_ray"] - ref["dcam_ray"])[mask].max()
    assert err <= 3.0 * err32 + 1e-4 * scale, (err / scale, err32 / scale)


def test_camera_recovery_example(hiplib):
    sys.path.insert(0, ROOT)
    from examples.camera_opt_synthetic import main
    res = main(["--vol", "64", "--img", "64", "--tf-res", "64", "--iterations", "40", "--quiet"])
    e, losses = res["errors"], res["losses"]
    assert e[-1] * 5.0 <= e[0], e
    assert losses[-1] < losses[0]
