"""The fused MS-SSIM + MSE image loss without a GPU: the C ABI declares, exports and signs its entry points and
rejects bad arguments before any HIP call; ms_ssim2d's definition (single level, pyramid, minimum side); and a float64 torch
restatement of the closed-form backward the kernels implement (CS / SSIM adjoints per level, the pooling's transpose) matches
torch.autograd of ms_dssim_mse_loss."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as TF

from differender_amd.utils.losses import MS_SSIM_WEIGHTS, _gauss_window, ms_dssim_mse_loss, ms_ssim2d, ssim2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dr_msssim_workspace_bytes", "dr_msssim_mse_fwd", "dr_msssim_mse_bwd")


def test_header_declares_the_msssim_entry_points():
    text = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bsize_t dr_msssim_workspace_bytes\s*\(", text)
    for name in ENTRIES[1:]:
        assert re.search(rf"\bint {name}\s*\(", text), name
    assert "DR_MSSSIM_MAX_LEVELS" in text


def test_library_exports_and_native_signs_the_msssim_entry_points(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES, name
    assert len(N.SIGNATURES["dr_msssim_workspace_bytes"][1]) == 6
    assert len(N.SIGNATURES["dr_msssim_mse_fwd"][1]) == 17 and len(N.SIGNATURES["dr_msssim_mse_bwd"][1]) == 20
    assert N.SIGNATURES["dr_msssim_workspace_bytes"][0] is ctypes.c_size_t
    assert hiplib.dr_abi_version() == 9


def _sides(h, levels):
    out = [h]
    for _ in range(levels - 1):
        out.append((out[-1] + 1) // 2)
    return out


@pytest.mark.parametrize("shape,levels,gy", [((1, 4, 161, 161), 5, 0), ((2, 3, 241, 333), 5, 1), ((8, 4, 256, 256), 3, 0),
                                              ((1, 1, 200, 200), 1, 1)])
def test_workspace_bytes(hiplib, shape, levels, gy):
    n, c, h, w = shape
    got = hiplib.dr_msssim_workspace_bytes(n, c, h, w, levels, gy)
    hs, ws = _sides(h, levels), _sides(w, levels)
    need = sum(math.ceil(4 * n * c * hs[l] * ws[l] / 256) * 256 * (4 if gy else 3) for l in range(1, levels))
    assert got == need
    for bad in ((0, c, h, w, levels), (n, c, h, -1, levels), (n, c, h, w, 0), (n, c, h, w, 6)):
        assert hiplib.dr_msssim_workspace_bytes(*bad, gy) == 0


def _call(lib, bwd, **kw):
    strides = (ctypes.c_int64 * 4)(4 * 200 * 200, 200 * 200, 200, 1)
    weights = (ctypes.c_double * 5)(*MS_SSIM_WEIGHTS)
    a = dict(x=16, y=16, N=1, C=4, H=200, W=200, strides=strides, data_range=1.0, win_size=11, win_sigma=1.5, K1=0.01,
             K2=0.03, weights=weights, levels=5, ws=16, stats=16, gx=16)
    a.update(kw)
    head = (a["x"], a["y"], a["N"], a["C"], a["H"], a["W"], a["strides"], a["data_range"], a["win_size"], a["win_sigma"],
            a["K1"], a["K2"], a["weights"], a["levels"])
    if bwd:
        return lib.dr_msssim_mse_bwd(*head, a["stats"], None, a["gx"], None, a["ws"], None)
    return lib.dr_msssim_mse_fwd(*head, a["ws"], a["stats"], None)


BAD = [dict(x=None), dict(y=None), dict(strides=None), dict(stats=None), dict(weights=None), dict(ws=None), dict(N=0),
       dict(C=-1), dict(H=0), dict(W=0), dict(H=160), dict(W=160), dict(win_size=7, H=96), dict(win_size=10),
       dict(win_size=33), dict(win_size=0), dict(levels=0), dict(levels=6), dict(data_range=0.0), dict(data_range=-1.0),
       dict(data_range=float("nan")), dict(data_range=float("inf")), dict(win_sigma=0.0),
       dict(weights=(ctypes.c_double * 5)(0.1, 0.2, float("nan"), 0.2, 0.1)),
       dict(weights=(ctypes.c_double * 5)(0.1, 0.2, 0.0, 0.2, 0.1)),
       dict(weights=(ctypes.c_double * 5)(0.1, -0.2, 0.3, 0.2, 0.1))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v if not isinstance(v, ctypes.Array) else list(v)}"
                                                   for k, v in b.items()) for b in BAD])
def test_argument_validation_needs_no_gpu(hiplib, bad):
    # (the pointers are never dereferenced: every argument is checked before the first HIP call)
    assert _call(hiplib, False, **bad) == -1
    assert _call(hiplib, True, **bad) == -1


def test_backward_requires_grad_x(hiplib):
    assert _call(hiplib, True, gx=None) == -1


def test_window_31_minimum_side_is_481(hiplib):
    assert _call(hiplib, False, win_size=31, H=480, W=481) == -1
    assert _call(hiplib, False, win_size=31, H=481, W=480) == -1


# ---- the definition ---------------------------------------------------------------------------------------------------

def _images(case, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=g, dtype=torch.float64)
    if case == "random":
        Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    elif case == "identical":
        Y = X.clone()
    elif case == "anti":
        Y = 1.0 - X
    elif case == "constant":
        X, Y = torch.full(shape, 0.25, dtype=torch.float64), torch.full(shape, 0.6, dtype=torch.float64)
    return X, Y


@pytest.mark.parametrize("shape", [(2, 3, 170, 181), (1, 2, 161, 200)])
def test_single_level_is_nonnegative_ssim(shape):
    X, Y = _images("random", shape)
    a = ms_ssim2d(X, Y, data_range=1.0, weights=(1.0,))
    b = ssim2d(X, Y, data_range=1.0, nonnegative_ssim=True)
    assert torch.allclose(a, b, rtol=1e-14, atol=0)
    a = ms_ssim2d(X, Y, data_range=1.0, weights=(1.0,), size_average=False)
    b = ssim2d(X, Y, data_range=1.0, nonnegative_ssim=True, size_average=False)
    assert a.shape == (shape[0],) and torch.allclose(a, b, rtol=1e-14, atol=0)


def pool(x):
    """2x2 average with padding (H % 2, W % 2) on both sides, padded zeros counted, by index arithmetic."""
    ph, pw = x.shape[2] % 2, x.shape[3] % 2
    Hn, Wn = (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2
    xp = TF.pad(x, (pw, pw, ph, ph))[:, :, :2 * Hn, :2 * Wn]
    return (xp[:, :, 0::2, 0::2] + xp[:, :, 0::2, 1::2] + xp[:, :, 1::2, 0::2] + xp[:, :, 1::2, 1::2]) / 4


def pool_T(d, H, W):
    """The transpose of pool onto an H x W plane: each fine pixel takes 1/4 of its one parent (y + H % 2) // 2."""
    ry = (torch.arange(H) + H % 2) // 2
    rx = (torch.arange(W) + W % 2) // 2
    return 0.25 * d[:, :, ry][:, :, :, rx]


@pytest.mark.parametrize("hw", [(17, 17), (16, 16), (17, 30), (30, 17), (161, 161), (241, 333)])
def test_pyramid_is_avg_pool2d(hw):
    X, _ = _images("random", (2, 3) + hw, seed=1)
    for _ in range(4):
        ref = TF.avg_pool2d(X, kernel_size=2, padding=[X.shape[2] % 2, X.shape[3] % 2])
        got = pool(X)
        assert got.shape == ref.shape == (2, 3, (X.shape[2] + 1) // 2, (X.shape[3] + 1) // 2)
        assert torch.allclose(got, ref, rtol=1e-15, atol=0)
        X = got


def test_pool_transpose_is_avg_pool2d_backward():
    X = torch.rand(1, 2, 23, 18, dtype=torch.float64, requires_grad=True)
    d = torch.rand(1, 2, 12, 9, dtype=torch.float64)
    TF.avg_pool2d(X, kernel_size=2, padding=[1, 0]).backward(d)
    assert torch.allclose(pool_T(d, 23, 18), X.grad, rtol=1e-15, atol=0)


@pytest.mark.parametrize("hw,k", [((160, 200), 11), ((200, 160), 11), ((96, 100), 7), ((480, 500), 31)])
def test_raises_below_the_minimum_side(hw, k):
    X = torch.rand((1, 1) + hw, dtype=torch.float64)
    with pytest.raises(ValueError):
        ms_ssim2d(X, X, data_range=1.0, win_size=k)
    with pytest.raises(ValueError):
        ms_ssim2d(X, X, data_range=1.0, win_size=k, weights=(0.5, 0.5))


def test_identical_images_give_one():
    X, Y = _images("identical", (1, 2, 170, 170))
    assert torch.allclose(ms_ssim2d(X, Y, data_range=1.0), torch.tensor(1.0, dtype=torch.float64), atol=1e-12)


# ---- the closed form of the backward (what msssim.hip computes), in float64 torch -----------------------------------------

def closed_form(X, Y, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03), weights=MS_SSIM_WEIGHTS,
                up=(1.0, 0.0, 0.0), shift=(0.0, 0.0)):
    """(loss, dms, mse, dX, dY) from the closed-form backward of DESIGN.md D10. shift = (cx, cy): the moments of every level
    taken of (X_l - cx, Y_l - cy) and the means put back, as the kernels do per tile."""
    N, C = X.shape[:2]
    k, L = win_size, len(weights)
    win = _gauss_window(k, win_sigma, X.dtype, X.device)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2

    def G(x):
        c = x.shape[1]
        x = TF.conv2d(x, win.view(1, 1, k, 1).expand(c, 1, k, 1), groups=c)
        return TF.conv2d(x, win.view(1, 1, 1, k).expand(c, 1, 1, k), groups=c)

    def GT(d):
        c = d.shape[1]
        d = TF.conv_transpose2d(d, win.view(1, 1, 1, k).expand(c, 1, 1, k), groups=c)
        return TF.conv_transpose2d(d, win.view(1, 1, k, 1).expand(c, 1, k, 1), groups=c)

    Xs, Ys = [X], [Y]
    for _ in range(L - 1):
        Xs.append(pool(Xs[-1]))
        Ys.append(pool(Ys[-1]))
    terms, v = [], []
    for l in range(L):
        xs, ys = Xs[l] - shift[0], Ys[l] - shift[1]
        n1, n2, m3, m4, m5 = G(xs), G(ys), G(xs * xs), G(ys * ys), G(xs * ys)
        sw = G(torch.ones_like(X[:1, :1, :Xs[l].shape[2], :Xs[l].shape[3]]))
        mu1, mu2 = n1 + shift[0] * sw, n2 + shift[1] * sw
        a1, a2 = 2 * mu1 * mu2 + C1, mu1 * mu1 + mu2 * mu2 + C1
        b1, b2 = 2 * (m5 - n1 * n2) + C2, (m3 - n1 * n1) + (m4 - n2 * n2) + C2
        A, B = a1 / a2, b1 / b2
        v.append(torch.relu((B if l < L - 1 else A * B).flatten(2).mean(-1)))
        terms.append((xs, ys, n1, n2, mu1, mu2, a2, b2, A, B))
    v = torch.stack(v)                                               # (L, N, C)
    w = torch.tensor(weights, dtype=X.dtype).view(-1, 1, 1)
    ms = torch.prod(v ** w, dim=0)
    dms = 1.0 - ms.mean()
    mse = ((X - Y) ** 2).mean()
    loss = torch.nan_to_num(dms) + mse
    u0, u1, u2 = up
    ok = (v > 0).all(0)                                              # (N, C): the plane has an MS gradient at all
    g_ms = -(u0 * float(torch.isfinite(dms)) + u1) / (N * C)
    dX = dY = None
    for l in reversed(range(L)):
        xs, ys, n1, n2, mu1, mu2, a2, b2, A, B = terms[l]
        g = torch.where(ok, g_ms * w[l] * ms / v[l], torch.zeros_like(ms)) / (n1.shape[2] * n1.shape[3])
        mask = ok[:, :, None, None]
        s = g[:, :, None, None]
        if l == L - 1:   # SSIM = A B
            d_mu1 = s * (2 * B * (mu2 - mu1 * A) / a2 + 2 * A * (n1 * B - n2) / b2)
            d_mu2 = s * (2 * B * (mu1 - mu2 * A) / a2 + 2 * A * (n2 * B - n1) / b2)
            d_m34, d_m5 = s * (-A * B / b2), s * (2 * A / b2)
        else:            # CS = B: dB/dm3 = -B/b2, dB/dm5 = 2/b2, dB/dmu1 = 2(mu1 B - mu2)/b2
            d_mu1, d_mu2 = s * (2 * (n1 * B - n2) / b2), s * (2 * (n2 * B - n1) / b2)
            d_m34, d_m5 = s * (-B / b2), s * (2 / b2)
        zero = torch.zeros((), dtype=X.dtype)
        gx = torch.where(mask, GT(d_mu1) + 2 * xs * GT(d_m34) + ys * GT(d_m5), zero)
        gy = torch.where(mask, GT(d_mu2) + 2 * ys * GT(d_m34) + xs * GT(d_m5), zero)
        if dX is not None:
            H, W = xs.shape[2:]
            gx, gy = gx + pool_T(dX, H, W), gy + pool_T(dY, H, W)
        dX, dY = gx, gy
    e = (u0 + u2) * 2 * (X - Y) / X.numel()
    return loss, dms, mse, dX + e, dY - e


def autograd_ref(X, Y, win_size=11, weights=MS_SSIM_WEIGHTS, up=(1.0, 0.0, 0.0)):
    X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    loss, dms, mse = ms_dssim_mse_loss(X, Y, win_size=win_size, weights=weights)
    (up[0] * loss + up[1] * dms + up[2] * mse).backward()
    return loss.detach(), dms.detach(), mse.detach(), X.grad, Y.grad


def _close(got, ref):
    for a, b in zip(got[:3], ref[:3]):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-14), (float(a), float(b))
    for a, b in zip(got[3:], ref[3:]):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-15 + 1e-9 * float(b.abs().max())), float((a - b).abs().max())


CASES = [("random", (2, 3, 161, 161), 11, MS_SSIM_WEIGHTS), ("random", (1, 2, 171, 190), 11, MS_SSIM_WEIGHTS),
         ("random", (1, 2, 175, 163), 11, (0.3, 0.7)), ("random", (1, 2, 165, 170), 11, (0.1, 0.2, 0.3, 0.4)),
         ("random", (1, 2, 170, 163), 11, (1.0,)), ("random", (1, 2, 101, 98), 7, (0.2, 0.3, 0.5)),
         ("identical", (1, 2, 162, 177), 11, MS_SSIM_WEIGHTS), ("constant", (1, 1, 161, 164), 11, MS_SSIM_WEIGHTS)]


@pytest.mark.parametrize("case,shape,k,weights", CASES,
                         ids=[f"{c}-{'x'.join(map(str, s))}-k{k}-L{len(w)}" for c, s, k, w in CASES])
def test_closed_form_backward_matches_autograd(case, shape, k, weights):
    X, Y = _images(case, shape)
    _close(closed_form(X, Y, win_size=k, weights=weights), autograd_ref(X, Y, win_size=k, weights=weights))


def test_shifted_moments_are_the_same_maths():
    X, Y = _images("random", (1, 2, 165, 171), seed=2)
    got = closed_form(X, Y, shift=(float(X[0, 0, 3, 4]), float(Y[0, 1, 5, 6])))
    _close(got, autograd_ref(X, Y))


@pytest.mark.parametrize("up", [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, -2.0, 3.0)])
def test_closed_form_upstream_weights(up):
    X, Y = _images("random", (1, 2, 163, 170), seed=3)
    _close(closed_form(X, Y, up=up), autograd_ref(X, Y, up=up))


def test_negative_cs_plane_gets_no_ms_gradient():
    X, Y = _images("random", (1, 3, 161, 166), seed=4)
    Y[0, 1] = 1.0 - X[0, 1]      # anti-correlated plane: CS < 0 at level 0, relu -> 0, ms = 0
    got, ref = closed_form(X, Y), autograd_ref(X, Y)
    _close(got, ref)
    e = 2 * (X - Y) / X.numel()
    assert torch.equal(got[3][0, 1], e[0, 1]) and torch.allclose(ref[3][0, 1], e[0, 1], rtol=1e-12, atol=0)
    assert not torch.allclose(ref[3][0, 0], e[0, 0], rtol=1e-6, atol=0)   # the other planes keep theirs


def test_closed_form_nan_gives_no_ms_gradient():
    X, Y = _images("random", (1, 2, 161, 161), seed=5)
    X[0, 1, 70, 90] = float("nan")
    loss, dms, mse, dX, dY = closed_form(X, Y)
    assert torch.isnan(loss) and torch.isnan(dms) and torch.isnan(mse)
    # no MS gradient for any plane (dms is not finite): the mse term alone, NaN exactly at the NaN pixel
    e = 2 * (X - Y) / X.numel()
    assert torch.equal(torch.isnan(dX), torch.isnan(X)) and torch.equal(dX[~torch.isnan(X)], e[~torch.isnan(X)])
    ref = autograd_ref(X, Y)[3]
    finite = torch.isfinite(ref)
    assert finite[0, 0].all() and torch.allclose(dX[finite], ref[finite], rtol=1e-12, atol=0)


def test_fused_loss_rejects_what_it_cannot_serve():
    from differender_amd.utils import fused_ms_dssim_mse_loss
    x = torch.rand(1, 2, 170, 170)
    with pytest.raises(ValueError):
        fused_ms_dssim_mse_loss(x[0], x[0])
    with pytest.raises(ValueError):
        fused_ms_dssim_mse_loss(x, x[:, :1])
    with pytest.raises(TypeError):
        fused_ms_dssim_mse_loss(x.double(), x.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_ms_dssim_mse_loss(x, x)
