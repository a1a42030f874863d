"""The fused MS-SSIM + MSE image loss on the GPU (msssim.hip) against ms_dssim_mse_loss in float64 on the CPU,
with the D8 tolerance rule (3x what torch's own float32 evaluation is off by); through the C ABI on a march buffer, the
autograd loss, the renderer and the TF optimisation example."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from differender_amd import _native as N
from differender_amd import functional as F
from differender_amd.utils import MS_SSIM_WEIGHTS, fused_dssim_mse_loss, fused_ms_dssim_mse_loss, ms_dssim_mse_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _torch_ref(X, Y, dtype, win_size=11, weights=MS_SSIM_WEIGHTS, up=(1.0, 0.0, 0.0)):
    """(loss, dms, mse, dX, dY) of the torch definition on the CPU in `dtype`."""
    X = X.detach().cpu().to(dtype).requires_grad_(True)
    Y = Y.detach().cpu().to(dtype).requires_grad_(True)
    loss, dms, mse = ms_dssim_mse_loss(X, Y, win_size=win_size, weights=weights)
    (up[0] * loss + up[1] * dms + up[2] * mse).backward()
    return [t.detach().double() for t in (loss, dms, mse, X.grad, Y.grad)]


def _check(got, X, Y, win_size=11, weights=MS_SSIM_WEIGHTS, up=(1.0, 0.0, 0.0)):
    """got = (loss, dms, mse, dX[, dY]) from the kernels; the D8 rule against the float64 reference."""
    r64 = _torch_ref(X, Y, torch.float64, win_size, weights, up)
    r32 = _torch_ref(X, Y, torch.float32, win_size, weights, up)
    for name, g, a, b in zip(("loss", "dms", "mse"), got[:3], r64[:3], r32[:3]):
        g = float(g)
        tol = max(3 * abs(float(b) - float(a)), 1e-6)
        assert abs(g - float(a)) <= tol, (name, g, float(a), tol)
    for name, g, a, b in zip(("dX", "dY"), got[3:], r64[3:], r32[3:]):
        g = g.detach().cpu().double()
        finite = torch.isfinite(a)
        tol = max(3 * float((b - a)[finite].abs().max()), 1e-5 * float(a[finite].abs().max()))
        err = float((g - a)[finite].abs().max())
        assert err <= tol, (name, err, tol)


def _images(shape, case="random", seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=g)
    if case == "random":
        Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)
    elif case == "identical":
        Y = X.clone()
    elif case == "anti":
        Y = 1.0 - X
    elif case == "constant":
        X, Y = torch.full(shape, 0.25), torch.full(shape, 0.6)
    elif case == "nan":
        Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)
        X[0, 1, shape[2] // 2, shape[3] // 3] = float("nan")
    return X.to(DEV), Y.to(DEV)


def _kernel(X, Y, win_size=11, weights=MS_SSIM_WEIGHTS):
    stats = F.msssim_mse_fwd(X, Y, win_size=win_size, weights=weights)
    gx, gy = F.msssim_mse_bwd(X, Y, stats, want_ref_grad=True, win_size=win_size, weights=weights)
    s = stats.cpu()
    return s[-3], s[-2], s[-1], gx, gy


SHAPES = [(8, 4, 256, 256), (1, 4, 512, 512), (2, 3, 161, 161), (1, 4, 241, 333)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_matches_torch(shape):
    X, Y = _images(shape)
    _check(_kernel(X, Y), X, Y)


@pytest.mark.parametrize("k,shape", [(7, (2, 4, 97, 130)), (31, (1, 2, 481, 481))])
def test_window_sizes(k, shape):
    X, Y = _images(shape, seed=k)
    _check(_kernel(X, Y, win_size=k), X, Y, win_size=k)


LEVELS = [(1.0,), (0.4, 0.6), (0.2, 0.5, 0.3), (0.1, 0.2, 0.3, 0.4), (0.3, 0.1, 0.2, 0.25, 0.15)]


@pytest.mark.parametrize("weights", LEVELS, ids=[f"L{len(w)}" for w in LEVELS])
def test_levels_and_weights(weights):
    X, Y = _images((2, 3, 170, 181), seed=len(weights))
    got = _kernel(X, Y, weights=weights)
    _check(got, X, Y, weights=weights)
    stats = F.msssim_mse_fwd(X, Y, weights=weights)
    assert stats.numel() == (len(weights) + 1) * 6 + 3
    if len(weights) == 1:   # one level is single-scale SSIM with relu: the DSSIM of D9
        _, dssim, _ = fused_dssim_mse_loss(X, Y)
        assert abs(float(got[1]) - float(dssim)) <= 1e-6


@pytest.mark.parametrize("case", ["identical", "anti", "constant"])
def test_cases(case):
    X, Y = _images((2, 4, 170, 200), case)
    got = _kernel(X, Y)
    _check(got, X, Y)
    if case == "identical":
        assert abs(float(got[1])) <= 1e-6
    if case == "anti":   # CS < 0 at level 0: ms = 0 for every plane, dms = 1 and only the mse gradient is left
        assert float(got[1]) == 1.0
        assert torch.equal(got[3], (X - Y) * (2.0 / X.numel()))


def test_nan_in_x():
    X, Y = _images((2, 4, 170, 200), "nan")
    loss, dms, mse, gx, gy = _kernel(X, Y)
    assert torch.isnan(loss) and torch.isnan(dms) and torch.isnan(mse)
    # no MS gradient: the mse term alone, NaN exactly where X is
    e = (X - Y) * (2.0 / X.numel())
    assert torch.equal(torch.isnan(gx), torch.isnan(X))
    ok = ~torch.isnan(X)
    assert torch.allclose(gx[ok], e[ok], rtol=1e-6, atol=0) and torch.allclose(gy[ok], -e[ok], rtol=1e-6, atol=0)
    ref = _torch_ref(X, Y, torch.float64)[3]
    finite = torch.isfinite(ref)
    assert torch.allclose(gx.cpu().double()[finite], ref[finite], rtol=1e-5, atol=1e-12)


def test_gradient_is_bitwise_deterministic():
    X, Y = _images((8, 4, 256, 256), seed=11)
    a = F.msssim_mse_bwd(X, Y, F.msssim_mse_fwd(X, Y), want_ref_grad=True)
    b = F.msssim_mse_bwd(X, Y, F.msssim_mse_fwd(X, Y), want_ref_grad=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], F.msssim_mse_loss_grad(X, Y)[3])


def _march_buffer(V=2, W=176, H=168):
    """A real [view][W][H][4] march output per TF (the image Raycaster returns, flipped along H)."""
    from differender.utils import get_tf, in_circles
    from examples.render_nondiff_synthetic import synthetic_volume
    vol = synthetic_volume(32, DEV)[0].permute(2, 0, 1)
    cam = torch.stack([in_circles(0.3), in_circles(1.9)]).float().to(DEV)[:V]
    outs = []
    for name in ("tf1", "gray"):
        tf = get_tf(name, 64).t().contiguous().float().to(DEV)
        e, x, r, n = F.ray_setup(cam, (W, H), vol.shape, 1.0)
        out, _ = F.march_fwd(vol, tf, cam, e, x, r, n, 1 << 16, 1.0)
        outs.append(out.clone())
    return outs


def test_strided_march_buffer_equals_contiguous_image():
    out, ref = _march_buffer()
    V, W, H, C = out.shape
    img = torch.flip(out, (2,)).permute(0, 3, 2, 1).contiguous()   # what Raycaster returns
    gt = torch.flip(ref, (2,)).permute(0, 3, 2, 1).contiguous()
    # logical (n, c, h, w) -> buffer [n][w][H-1-h][c]: a negative stride along H from the last row, straight through the ABI
    lib, L = N.lib(), len(MS_SSIM_WEIGHTS)
    s = (ctypes.c_int64 * 4)(W * H * C, 1, -C, H * C)
    wts = (ctypes.c_double * L)(*MS_SSIM_WEIGHTS)
    off = 4 * (H - 1) * C
    stats = torch.empty((L + 1) * V * C + 3, dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.dr_msssim_workspace_bytes(V, C, H, W, L, 0), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = (out.data_ptr() + off, ref.data_ptr() + off, V, C, H, W, s, 1.0, 11, 1.5, 0.01, 0.03, wts, L)
    N.check(lib.dr_msssim_mse_fwd(*args, ws.data_ptr(), stats.data_ptr(), st), "fwd")
    gx = torch.empty_like(out)
    N.check(lib.dr_msssim_mse_bwd(*args, stats.data_ptr(), None, gx.data_ptr() + off, None, ws.data_ptr(), st), "bwd")
    loss, dms, mse, g_img = F.msssim_mse_loss_grad(img, gt)
    _check((stats[-3], stats[-2], stats[-1], torch.flip(gx, (2,)).permute(0, 3, 2, 1)), img, gt)
    for a, b in ((stats[-3], loss), (stats[-2], dms), (stats[-1], mse)):
        assert abs(float(a) - float(b)) <= 1e-6
    g_buf = torch.flip(g_img.permute(0, 3, 2, 1), (2,))
    assert float((gx - g_buf).abs().max()) <= 1e-5 * float(g_buf.abs().max())
    # the functional API on the permuted view (no copy): the image flipped along H. Unlike SSIM, MS-SSIM sees the flip: at an
    # odd level side (168 -> 84 -> 42 -> 21) the 2x2 pooling pairs other rows, so the reference is the flipped image's own loss
    xb, yb = out.permute(0, 3, 2, 1), ref.permute(0, 3, 2, 1)
    _check(F.msssim_mse_loss_grad(xb, yb), xb, yb)


def test_autograd_gives_the_target_its_gradient():
    X, Y = _images((2, 4, 170, 200), seed=3)
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss, dms, mse = fused_ms_dssim_mse_loss(x, y)
    assert loss.dtype == torch.float32 and loss.ndim == 0
    loss.backward()
    _check((loss, dms, mse, x.grad, y.grad), X, Y)


@pytest.mark.parametrize("which,up", [("loss", (1.0, 0.0, 0.0)), ("dms", (0.0, 1.0, 0.0)), ("mse", (0.0, 0.0, 1.0)),
                                      ("mix", (0.5, -2.0, 3.0))])
def test_autograd_through_each_output(which, up):
    X, Y = _images((2, 4, 170, 200), seed=4)
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss, dms, mse = fused_ms_dssim_mse_loss(x, y)
    (up[0] * loss + up[1] * dms + up[2] * mse).backward()
    _check((loss, dms, mse, x.grad, y.grad), X, Y, up=up)


def test_through_the_renderer():
    from differender_amd.volume_raycaster import Raycaster
    from differender.utils import get_tf, in_circles
    from examples.render_nondiff_synthetic import synthetic_volume
    vol = synthetic_volume(48, DEV).float()
    rc = Raycaster(vol.shape[-3:], (176, 176), 64, jitter=False, max_samples=2048)
    cams = torch.stack([in_circles(0.4), in_circles(2.1)]).float().to(DEV)
    with torch.no_grad():
        gt = rc(vol, get_tf("tf1", 64).to(DEV).float(), cams).detach()
    grads = []
    for loss_fn in (ms_dssim_mse_loss, fused_ms_dssim_mse_loss):
        tf = get_tf("gray", 64).to(DEV).float().requires_grad_(True)
        loss = loss_fn(rc(vol, tf, cams), gt)[0]
        loss.backward()
        grads.append((float(loss), tf.grad.clone()))
    (l0, t0), (l1, t1) = grads
    assert abs(l0 - l1) <= 1e-5
    assert float((t1 - t0).abs().max()) <= 1e-4 * float(t0.abs().max())


def test_tf_opt_example_with_msssim():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tf_opt_synthetic.py"), "--loss", "msssim", "--vol", "48",
                        "--img", "176", "--iterations", "40"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "->" in r.stdout
