"""The fused DSSIM + MSE image loss on the GPU (image_loss.hip) against dssim_mse_loss / ssim2d in float64 on the
CPU, with the D8 tolerance rule (3x what torch's own float32 evaluation is off by); through the C ABI on a march buffer, the
autograd loss, the renderer and the TF optimisation example."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from differender_amd import _native as N
from differender_amd import functional as F
from differender_amd.utils import dssim_mse_loss, fused_dssim_mse_loss, ssim2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _torch_loss(X, Y, win_size=11, nonneg=True):
    if win_size == 11 and nonneg:
        return dssim_mse_loss(X, Y)
    dssim = 1.0 - ssim2d(X, Y, data_range=1.0, win_size=win_size, nonnegative_ssim=nonneg)
    mse = TF.mse_loss(X, Y)
    return torch.nan_to_num(dssim) + mse, dssim, mse


def _torch_ref(X, Y, dtype, win_size=11, nonneg=True, up=(1.0, 0.0, 0.0)):
    """(loss, dssim, mse, dX, dY) of the torch definition on the CPU in `dtype`."""
    X = X.detach().cpu().to(dtype).requires_grad_(True)
    Y = Y.detach().cpu().to(dtype).requires_grad_(True)
    loss, dssim, mse = _torch_loss(X, Y, win_size, nonneg)
    (up[0] * loss + up[1] * dssim + up[2] * mse).backward()
    return [t.detach().double() for t in (loss, dssim, mse, X.grad, Y.grad)]


def _check(got, X, Y, win_size=11, nonneg=True, up=(1.0, 0.0, 0.0)):
    """got = (loss, dssim, mse, dX[, dY]) from the kernels; the D8 rule against the float64 reference."""
    r64 = _torch_ref(X, Y, torch.float64, win_size, nonneg, up)
    r32 = _torch_ref(X, Y, torch.float32, win_size, nonneg, up)
    for name, g, a, b in zip(("loss", "dssim", "mse"), got[:3], r64[:3], r32[:3]):
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
        Y = torch.rand(shape, generator=g)
        X[0, 1, shape[2] // 2, shape[3] // 3] = float("nan")
    return X.to(DEV), Y.to(DEV)


def _kernel(X, Y, win_size=11, nonneg=True):
    stats = F.dssim_mse_fwd(X, Y, win_size=win_size, nonnegative_ssim=nonneg)
    gx, gy = F.dssim_mse_bwd(X, Y, stats, want_ref_grad=True, win_size=win_size, nonnegative_ssim=nonneg)
    s = stats.cpu()
    return s[-3], s[-2], s[-1], gx, gy


SHAPES = [(8, 4, 256, 256), (1, 4, 512, 512), (2, 4, 64, 200), (1, 4, 8, 300), (1, 4, 10, 10), (3, 3, 11, 11)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_matches_torch(shape):
    X, Y = _images(shape)
    _check(_kernel(X, Y), X, Y)


@pytest.mark.parametrize("k", [7, 31])
def test_window_sizes(k):
    X, Y = _images((2, 4, 64, 200), seed=k)
    _check(_kernel(X, Y, win_size=k), X, Y, win_size=k)


@pytest.mark.parametrize("case", ["identical", "anti", "constant"])
def test_cases(case):
    X, Y = _images((2, 4, 64, 200), case)
    got = _kernel(X, Y)
    _check(got, X, Y)
    if case == "anti":   # relu active: dssim = 1 and only the mse gradient is left
        assert float(got[1]) == 1.0
        assert torch.equal(got[3], (X - Y) * (2.0 / X.numel()))


def test_signed_ssim():
    for case in ("random", "anti"):
        X, Y = _images((2, 4, 64, 200), case, seed=7)
        _check(_kernel(X, Y, nonneg=False), X, Y, nonneg=False)


def test_nan_in_x():
    X, Y = _images((2, 4, 64, 200), "nan")
    loss, dssim, mse, gx, gy = _kernel(X, Y)
    assert torch.isnan(loss) and torch.isnan(dssim) and torch.isnan(mse)
    # no dssim gradient: the mse term alone, NaN exactly where X is
    e = (X - Y) * (2.0 / X.numel())
    assert torch.equal(torch.isnan(gx), torch.isnan(X))
    ok = ~torch.isnan(X)
    assert torch.allclose(gx[ok], e[ok], rtol=1e-6, atol=0) and torch.allclose(gy[ok], -e[ok], rtol=1e-6, atol=0)
    ref = _torch_ref(X, Y, torch.float64)[3]
    finite = torch.isfinite(ref)
    assert torch.allclose(gx.cpu().double()[finite], ref[finite], rtol=1e-5, atol=1e-12)


def test_gradient_is_bitwise_deterministic():
    X, Y = _images((8, 4, 256, 256), seed=11)
    stats = F.dssim_mse_fwd(X, Y)
    a = F.dssim_mse_bwd(X, Y, stats, want_ref_grad=True)
    stats2 = F.dssim_mse_fwd(X, Y)
    b = F.dssim_mse_bwd(X, Y, stats2, want_ref_grad=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g = F.dssim_mse_loss_grad(X, Y)[3]
    assert torch.equal(a[0], g)


def _march_buffer(V=2, W=48, H=40):
    """A real [view][W][H][4] march output and the same image as Raycaster returns it (flipped along H, (V, 4, H, W))."""
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


def _abi(buf, ref, strides, offset):
    """dr_dssim_mse_fwd / _bwd straight on raw buffers: element strides (may be negative) from element `offset`."""
    lib, V, C = N.lib(), buf.shape[0], buf.shape[3]
    H, W = buf.shape[2], buf.shape[1]
    s = (ctypes.c_int64 * 4)(*strides)
    stats = torch.empty(V * C + 3, dtype=torch.float64, device=DEV)
    px, py = buf.data_ptr() + 4 * offset, ref.data_ptr() + 4 * offset
    st = torch.cuda.current_stream().cuda_stream
    N.check(lib.dr_dssim_mse_fwd(px, py, V, C, H, W, s, 1.0, 11, 1.5, 0.01, 0.03, 1, stats.data_ptr(), st), "fwd")
    gx = torch.empty_like(buf)
    N.check(lib.dr_dssim_mse_bwd(px, py, V, C, H, W, s, 1.0, 11, 1.5, 0.01, 0.03, 1, stats.data_ptr(), None,
                                 gx.data_ptr() + 4 * offset, None, st), "bwd")
    return stats, gx


def test_strided_march_buffer_equals_contiguous_image():
    out, ref = _march_buffer()
    V, W, H, C = out.shape
    img = torch.flip(out, (2,)).permute(0, 3, 2, 1).contiguous()   # what Raycaster returns
    gt = torch.flip(ref, (2,)).permute(0, 3, 2, 1).contiguous()
    # logical (n, c, h, w) -> buffer [n][w][H-1-h][c]: a negative stride along H from the last row
    stats, gx = _abi(out, ref, (W * H * C, 1, -C, H * C), (H - 1) * C)
    loss, dssim, mse, g_img = F.dssim_mse_loss_grad(img, gt)
    _check((stats[-3], stats[-2], stats[-1], torch.flip(gx, (2,)).permute(0, 3, 2, 1)), img, gt)
    for a, b in ((stats[-3], loss), (stats[-2], dssim), (stats[-1], mse)):
        assert abs(float(a) - float(b)) <= 1e-6
    g_buf = torch.flip(g_img.permute(0, 3, 2, 1), (2,))
    assert float((gx - g_buf).abs().max()) <= 1e-5 * float(g_buf.abs().max())
    # the functional API on the permuted view (no copy; the image flipped along H, which the loss does not see)
    # (the same image flipped along H: other tiles, other roundings; held to the same D8 rule)
    l2, d2, m2, g2 = F.dssim_mse_loss_grad(out.permute(0, 3, 2, 1), ref.permute(0, 3, 2, 1))
    _check((l2, d2, m2, torch.flip(g2, (2,))), img, gt)


def test_autograd_gives_the_target_its_gradient():
    X, Y = _images((2, 4, 64, 200), seed=3)
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss, dssim, mse = fused_dssim_mse_loss(x, y)
    assert loss.dtype == torch.float32 and loss.ndim == 0
    loss.backward()
    _check((loss, dssim, mse, x.grad, y.grad), X, Y)


@pytest.mark.parametrize("which,up", [("dssim", (0.0, 1.0, 0.0)), ("mse", (0.0, 0.0, 1.0)), ("mix", (0.5, -2.0, 3.0))])
def test_autograd_through_each_output(which, up):
    X, Y = _images((2, 4, 64, 200), seed=4)
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss, dssim, mse = fused_dssim_mse_loss(x, y)
    (up[0] * loss + up[1] * dssim + up[2] * mse).backward()
    _check((loss, dssim, mse, x.grad, y.grad), X, Y, up=up)


def test_through_the_renderer():
    from differender_amd.volume_raycaster import Raycaster
    from differender.utils import get_tf, in_circles
    from examples.render_nondiff_synthetic import synthetic_volume
    vol0 = synthetic_volume(48, DEV)
    rc = Raycaster(vol0.shape[-3:], (64, 64), 64, jitter=False, max_samples=2048)
    cams = torch.stack([in_circles(0.4), in_circles(2.1)]).float().to(DEV)
    with torch.no_grad():
        gt = rc(vol0, get_tf("tf1", 64).to(DEV).float(), cams).detach()
    grads = []
    for fused in (False, True):
        vol = vol0.clone().float().requires_grad_(True)
        tf = get_tf("gray", 64).to(DEV).float().requires_grad_(True)
        res = rc(vol, tf, cams)
        loss = (fused_dssim_mse_loss if fused else dssim_mse_loss)(res, gt)[0]
        loss.backward()
        grads.append((float(loss), vol.grad.clone(), tf.grad.clone()))
    (l0, v0, t0), (l1, v1, t1) = grads
    assert abs(l0 - l1) <= 1e-5
    assert float((v1 - v0).abs().max()) <= 1e-4 * float(v0.abs().max())
    assert float((t1 - t0).abs().max()) <= 1e-4 * float(t0.abs().max())


def test_tf_opt_example_with_dssim():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tf_opt_synthetic.py"), "--loss", "dssim", "--vol", "48",
                        "--img", "96", "--iterations", "40"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "->" in r.stdout
