"""Image losses of the reference's demo loop that are not part of the raycasting path.

`ssim2d` restates `pytorch_msssim.ssim` as examples/test_opt_tf.py:14,70 calls it
(`ssim2d(res, gt, data_range=1.0, size_average=True, nonnegative_ssim=True)`): pytorch_msssim is not installed here and is
not vendored by the reference, so its semantics are taken from memory of the package [mem: parity unpinned] -- 11-tap
gaussian window (sigma 1.5), separable, VALID convolution per channel, K = (0.01, 0.03), the per-channel mean of the SSIM map,
`relu` on it when nonnegative_ssim, mean over channels and batch when size_average. Plain torch ops (differentiable through
autograd); used by the synthetic counterparts of the demo (examples/test_opt_synthetic.py, bench.py --workload opt).

`fused_dssim_mse_loss` is the same loss on the HIP kernels: one forward and one backward over the images, with
ssim2d / dssim_mse_loss as its definition.

`ms_ssim2d` restates `pytorch_msssim.ms_ssim`, the package's multi-scale SSIM, from the same memory [mem: parity unpinned]:
per level the SSIM and contrast-structure (CS) maps of ssim2d and their per-plane means, relu'd; 2x2 average pooling between
levels; the weighted product over the levels. `fused_ms_dssim_mse_loss` is ms_dssim_mse_loss on the HIP kernels (DESIGN.md
D10).

`tv3d` is the 3-D total-variation prior on a volume, the regulariser of a volume reconstruction such as the
demo's (salt noise in `vol`, examples/vol_denoise_tv_synthetic.py); `fused_tv3d_loss` is tv3d on the HIP kernels. With
differender_amd.distributed.all_reduce_gradients, add the term on one rank only (or after the reduce): otherwise it is counted
once per rank."""
import torch
import torch.nn.functional as F

__all__ = ["ssim2d", "dssim_mse_loss", "fused_dssim_mse_loss", "MS_SSIM_WEIGHTS", "ms_ssim2d", "ms_dssim_mse_loss",
           "fused_ms_dssim_mse_loss", "tv3d", "fused_tv3d_loss"]


def _gauss_window(size, sigma, dtype, device):
    x = torch.arange(size, dtype=dtype, device=device) - size // 2
    g = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def _filter(x, win):
    c = x.shape[1]
    k = win.numel()
    x = F.conv2d(x, win.view(1, 1, k, 1).expand(c, 1, k, 1), groups=c) if x.shape[2] >= k else x
    x = F.conv2d(x, win.view(1, 1, 1, k).expand(c, 1, 1, k), groups=c) if x.shape[3] >= k else x
    return x


def ssim2d(X, Y, data_range=255.0, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """SSIM of two (N, C, H, W) image batches; see the module docstring for what is restated and from where."""
    if X.shape != Y.shape or X.ndim != 4:
        raise ValueError("ssim2d expects two (N, C, H, W) tensors of the same shape")
    win = _gauss_window(win_size, win_sigma, X.dtype, X.device)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    c = X.shape[1]
    # the five windowed moments in ONE pair of grouped convolutions (channels stacked): two launches forward, two backward
    m = _filter(torch.cat([X, Y, X * X, Y * Y, X * Y], dim=1), win)
    mu1, mu2 = m[:, :c], m[:, c:2 * c]
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = m[:, 2 * c:3 * c] - mu1_sq
    s2 = m[:, 3 * c:4 * c] - mu2_sq
    s12 = m[:, 4 * c:] - mu12
    cs = (2.0 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2.0 * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs
    per_channel = ssim_map.flatten(2).mean(-1)
    if nonnegative_ssim:
        per_channel = torch.relu(per_channel)
    return per_channel.mean() if size_average else per_channel.mean(1)


def dssim_mse_loss(res, gt):
    """The loss of examples/test_opt_tf.py:70-72: nan_to_num(1 - ssim(res, gt, data_range=1, nonnegative)) + mse."""
    dssim = 1.0 - ssim2d(res, gt, data_range=1.0, size_average=True, nonnegative_ssim=True)
    mse = F.mse_loss(res, gt)
    return torch.nan_to_num(dssim) + mse, dssim, mse


class _FusedImageLoss(torch.autograd.Function):
    """(loss, dssim or dms, mse) of one of the fused image losses (`fwd`, `bwd`: its pair of differender_amd.functional) as one
    3-element float32 tensor; the caller unbinds it, so autograd hands backward the three upstream gradients stacked on the
    device and the kernel reads them there (no host read)."""

    @staticmethod
    def forward(ctx, res, gt, fwd, bwd, cfg):
        stats = fwd(res, gt, **cfg)
        ctx.save_for_backward(res, gt, stats)
        ctx.bwd, ctx.cfg = bwd, cfg
        return stats[-3:].float()

    @staticmethod
    def backward(ctx, g3):
        res, gt, stats = ctx.saved_tensors
        gx, gy = ctx.bwd(res, gt, stats, upstream=g3, want_ref_grad=ctx.needs_input_grad[1], **ctx.cfg)
        return (gx if ctx.needs_input_grad[0] else None), gy, None, None, None


def _fused_image_loss(name, res, gt, fwd, bwd, cfg):
    """The input check of both fused_*_loss front-ends (`name`: the one in the messages), then the loss as (loss, d, mse)."""
    if res.ndim != 4 or gt.shape != res.shape:
        raise ValueError(f"{name} expects two (N, C, H, W) tensors of the same shape")
    if res.dtype != torch.float32 or gt.dtype != torch.float32:
        raise TypeError(f"{name} expects float32 tensors")
    if not (res.is_cuda and gt.is_cuda):
        raise RuntimeError(f"{name} runs on a ROCm GPU only: there is no CPU path")
    return _FusedImageLoss.apply(res, gt, fwd, bwd, cfg).unbind(0)


def fused_dssim_mse_loss(res, gt, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=True):
    """dssim_mse_loss on the HIP kernels: returns (loss, dssim, mse), 0-d float32 tensors, with
    loss = nan_to_num(1 - ssim2d(res, gt, data_range, ..., nonnegative_ssim)) + mse_loss(res, gt). Differentiable w.r.t. res
    and, when it requires a gradient, gt. res and gt: (N, C, H, W) float32 on a ROCm GPU (there is no CPU path)."""
    from differender_amd import functional as DF
    cfg = dict(data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=tuple(K), nonnegative_ssim=nonnegative_ssim)
    return _fused_image_loss("fused_dssim_mse_loss", res, gt, DF.dssim_mse_fwd, DF.dssim_mse_bwd, cfg)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _ssim_cs(X, Y, win, data_range, K):
    """Per-plane means (N, C) of the SSIM map and of the CS map, formed exactly as ssim2d forms them."""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    c = X.shape[1]
    m = _filter(torch.cat([X, Y, X * X, Y * Y, X * Y], dim=1), win)
    mu1, mu2 = m[:, :c], m[:, c:2 * c]
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = m[:, 2 * c:3 * c] - mu1_sq
    s2 = m[:, 3 * c:4 * c] - mu2_sq
    s12 = m[:, 4 * c:] - mu12
    cs_map = (2.0 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2.0 * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim2d(X, Y, data_range=255.0, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """Multi-scale SSIM of two (N, C, H, W) image batches (pytorch_msssim.ms_ssim; see the module docstring).
    Level l < L-1 contributes relu(CS_nc), the last level relu(SSIM_nc); between levels X and Y are 2x2 average pooled with a
    padding of (H % 2, W % 2), the padded zeros counted. ms_nc = prod_l v_l ** w_l, averaged over (N, C), or over C when not
    size_average. With weights=(1.0,) it is ssim2d(..., nonnegative_ssim=True)."""
    if X.shape != Y.shape or X.ndim != 4:
        raise ValueError("ms_ssim2d expects two (N, C, H, W) tensors of the same shape")
    if min(X.shape[-2:]) <= (win_size - 1) * 2 ** 4:
        raise ValueError(f"ms_ssim2d needs both sides longer than {(win_size - 1) * 2 ** 4} (the window at the 5th scale)")
    weights = torch.tensor(MS_SSIM_WEIGHTS if weights is None else weights, dtype=X.dtype, device=X.device)
    win = _gauss_window(win_size, win_sigma, X.dtype, X.device)
    levels = weights.numel()
    vals = []
    for i in range(levels):
        ssim_nc, cs_nc = _ssim_cs(X, Y, win, data_range, K)
        if i < levels - 1:
            vals.append(torch.relu(cs_nc))
            padding = [X.shape[2] % 2, X.shape[3] % 2]
            X = F.avg_pool2d(X, kernel_size=2, padding=padding)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=padding)
    vals.append(torch.relu(ssim_nc))
    ms_nc = torch.prod(torch.stack(vals, dim=0) ** weights.view(-1, 1, 1), dim=0)
    return ms_nc.mean() if size_average else ms_nc.mean(1)


def ms_dssim_mse_loss(res, gt, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """nan_to_num(1 - ms_ssim2d(res, gt, data_range=1)) + mse, the multi-scale counterpart of dssim_mse_loss.
    Returns (loss, dms, mse)."""
    dms = 1.0 - ms_ssim2d(res, gt, data_range=1.0, size_average=True, win_size=win_size, win_sigma=win_sigma,
                          weights=weights, K=K)
    mse = F.mse_loss(res, gt)
    return torch.nan_to_num(dms) + mse, dms, mse


def fused_ms_dssim_mse_loss(res, gt, data_range=1.0, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """ms_dssim_mse_loss on the HIP kernels: returns (loss, dms, mse), 0-d float32 tensors, with
    loss = nan_to_num(1 - ms_ssim2d(res, gt, data_range, ...)) + mse_loss(res, gt). Differentiable w.r.t. res and, when it
    requires a gradient, gt. res and gt: (N, C, H, W) float32 on a ROCm GPU (there is no CPU path)."""
    from differender_amd import functional as DF
    cfg = dict(data_range=data_range, win_size=win_size, win_sigma=win_sigma,
               weights=tuple(float(w) for w in (MS_SSIM_WEIGHTS if weights is None else weights)), K=tuple(K))
    return _fused_image_loss("fused_ms_dssim_mse_loss", res, gt, DF.msssim_mse_fwd, DF.msssim_mse_bwd, cfg)


TV_NORMS = ("l1", "iso", "sq")


def tv3d(vol, norm="l1", eps=1e-3, reduction="mean"):
    """3-D total variation of vol (..., D, H, W); the leading axes are separate volumes. Forward differences along each of the
    last three axes with the last slice repeated (0 at the far edge), per voxel |dD| + |dH| + |dW| ("l1", anisotropic),
    sqrt(dD^2 + dH^2 + dW^2 + eps^2) ("iso", Charbonnier, eps > 0) or dD^2 + dH^2 + dW^2 ("sq", Tikhonov); summed
    (reduction="sum") or divided by vol.numel() ("mean"). Plain torch: any device, any float dtype; autograd gives the
    gradient (sign(0) = 0 for "l1"). This is the definition fused_tv3d_loss and dr_tv3d_fwd / _bwd implement."""
    if vol.ndim < 3:
        raise ValueError(f"tv3d expects a volume (..., D, H, W), got {vol.ndim} dimensions")
    if norm not in TV_NORMS:
        raise ValueError(f"norm must be one of {TV_NORMS}, got {norm!r}")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    d = [torch.diff(vol, dim=a, append=vol.narrow(a, vol.shape[a] - 1, 1)) for a in (-3, -2, -1)]
    if norm == "l1":
        t = d[0].abs() + d[1].abs() + d[2].abs()
    elif norm == "sq":
        t = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    else:
        if not eps > 0:
            raise ValueError(f"norm='iso' needs eps > 0, got {eps}")
        t = torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + eps * eps)
    s = t.sum()
    return s / vol.numel() if reduction == "mean" else s


class _FusedTV3D(torch.autograd.Function):
    """The TV sum from dr_tv3d_fwd, times `scale`, as a 0-d float32; backward hands the upstream gradient to dr_tv3d_bwd on the
    device (no host read)."""

    @staticmethod
    def forward(ctx, vol, norm, eps, scale):
        from differender_amd import functional as DF
        total = DF.tv3d_fwd(vol, norm, eps)
        ctx.save_for_backward(vol)
        ctx.cfg = (norm, eps, scale)
        return (total * scale).float()

    @staticmethod
    def backward(ctx, g):
        from differender_amd import functional as DF
        (vol,) = ctx.saved_tensors
        norm, eps, scale = ctx.cfg
        grad = DF.tv3d_bwd(vol, upstream=g, scale=scale, norm=norm, eps=eps)
        return grad.to(vol.dtype), None, None, None


def fused_tv3d_loss(vol, norm="l1", eps=1e-3, reduction="mean"):
    """tv3d on the HIP kernels: a 0-d float32 tensor, differentiable w.r.t. vol (the gradient comes back in vol's dtype and
    shape). vol: (..., D, H, W) float32 or float16 on a ROCm GPU (there is no CPU path), any strides -- Raycaster's user
    layouts (1, D, H, W) and (BS, 1, D, H, W) and its permuted views included. norm="iso" needs an eps whose square float32
    holds (eps >= 3e-23; the kernels add eps^2 in float32): a smaller one raises ValueError where tv3d in float32 gives NaN."""
    if vol.ndim < 3:
        raise ValueError(f"fused_tv3d_loss expects a volume (..., D, H, W), got {vol.ndim} dimensions")
    if vol.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"fused_tv3d_loss expects a float32 or float16 volume, got {vol.dtype}")
    if not vol.is_cuda:
        raise RuntimeError("fused_tv3d_loss runs on a ROCm GPU only: there is no CPU path")
    if norm not in TV_NORMS:
        raise ValueError(f"norm must be one of {TV_NORMS}, got {norm!r}")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    scale = 1.0 / vol.numel() if reduction == "mean" else 1.0
    return _FusedTV3D.apply(vol, norm, float(eps), scale)
