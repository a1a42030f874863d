"""Differentiable X-ray line-integral and maximum intensity projections of a scalar volume.

The two standard views of a volume beside compositing: the line integral int mu ds along each ray (the forward model of
tomography, a digitally reconstructed radiograph) and the maximum intensity projection (angiography). The samples are those of
Raycaster at the same sampling rate, camera and jitter; there is no transfer function and no shading.

    proj = Projector(volume.shape[-3:], (H, W), mode="sum")
    line_integral = proj(mu, look_from)          # mu ([BS,]1,D,H,W), look_from ([BS,]3) -> ([BS,]1,H,W)
    radiograph = torch.exp(-line_integral)       # Beer-Lambert: transmitted intensity of a monochromatic beam

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster. Gradients flow to the volume (a
back-projection) and to look_from (when it requires grad). Lengths are in world units of the renderer's [-1, 1]^3 box: a
constant volume c gives c times the chord of the ray through the box.
"""
import torch

from . import _native as N
from . import functional as F

__all__ = ["Projector", "ProjectFunction"]

_MODES = ("sum", "max")


class ProjectFunction(torch.autograd.Function):
    """Autograd boundary of the projections: `apply(pj, volume, look_from, batched, jitter)`. volume (W,D,H) or (BS,W,D,H),
    any strides; look_from (BS,3). Returns (W,H) or (BS,W,H)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pj, volume, look_from, batched, jitter=True):
        cam = look_from.reshape(-1, 3)
        volume = F.as_volume(volume)
        seed = F.new_jitter_seed() if jitter else 0
        e, x, r, n = F.ray_setup(cam, pj.output_shape, volume.shape[-3:], pj.sampling_rate, pj.fov, pj.near, seed)
        out, arg = F.project_fwd(volume, cam, e, x, r, n, pj.max_samples, pj.mode)
        ctx.save_for_backward(volume, cam, e, x, r, n, *((arg,) if arg is not None else ()))
        ctx.pj, ctx.batched, ctx.seed = pj, batched, seed
        ctx.lf_shape, ctx.lf_dtype = look_from.shape, look_from.dtype
        return out if batched else out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, cam, e, x, r, n = ctx.saved_tensors[:6]
        arg = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        pj = ctx.pj
        g = grad_output if ctx.batched else grad_output[None]
        dv = d_cam = None
        if ctx.needs_input_grad[1]:
            dv = torch.nan_to_num(F.project_bwd(volume, cam, e, x, r, n, g, pj.max_samples, pj.mode, arg))
        if ctx.needs_input_grad[2]:
            d_cam = F.project_bwd_cam(volume, cam, e, x, r, n, g, pj.max_samples, pj.mode, arg, fov_deg=pj.fov, near=pj.near,
                                      jitter_seed=ctx.seed)
            d_cam = d_cam.reshape(ctx.lf_shape).to(ctx.lf_dtype)
        return None, dv, d_cam, None, None


class Projector(torch.nn.Module):
    """Line-integral (mode "sum") or maximum intensity ("max") projection of a volume.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster; sampling_rate, jitter, fov, near and far as for Raycaster.
    max_samples None: every sample of every ray; an integer truncates the rays (and the integral) after that many samples.
    forward(volume ([BS,]1,D,H,W), look_from ([BS,]3)) -> ([BS,]1,H,W). For "sum" the result is D * sum of the samples,
    D = (exit - entry) / n the sample spacing in world units; torch.exp(-proj) is the Beer-Lambert transmission."""

    def __init__(self, volume_shape, output_shape, mode="sum", sampling_rate=1.0, jitter=True, max_samples=None, fov=30.0,
                 near=0.1, far=100.0):
        super().__init__()
        if len(tuple(volume_shape)) != 3 or len(tuple(output_shape)) != 2:
            raise ValueError("expected volume_shape (D, H, W) and output_shape (H, W)")
        if min(volume_shape) < 2 or min(output_shape) < 1:
            raise ValueError(f"volume_shape needs >= 2 voxels per axis and output_shape >= 1 pixel, got {tuple(volume_shape)}, "
                             f"{tuple(output_shape)}")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'sum' or 'max', got {mode!r}")
        if not (sampling_rate > 0):
            raise ValueError(f"sampling_rate must be > 0, got {sampling_rate}")
        if max_samples is not None and int(max_samples) < 1:
            raise ValueError(f"max_samples must be None or >= 1, got {max_samples}")
        self.volume_shape = (volume_shape[2], volume_shape[0], volume_shape[1])  # (W, D, H), as Raycaster
        self.output_shape = tuple(output_shape)
        self.mode = mode
        self.sampling_rate = float(sampling_rate)
        self.jitter = jitter
        self.max_samples = max_samples
        self.fov, self.near, self.far = fov, near, far
        N.lib()  # fail loudly at construction time if the HIP library is missing

    def _determine_batch(self, volume, look_from):
        """-> (batched, vol ([BS,] W, D, H) view, look_from (BS, 3)); an un-batched volume is shared by all views."""
        if volume.ndim not in (4, 5) or look_from.ndim not in (1, 2):
            raise ValueError("expected volume ([BS,]1,D,H,W) and look_from ([BS,]3)")
        if volume.shape[-4] != 1 or look_from.shape[-1] != 3:
            raise ValueError(f"expected volume ([BS,]1,D,H,W) and look_from ([BS,]3); got {tuple(volume.shape)}, "
                             f"{tuple(look_from.shape)}")
        vshape = (volume.shape[-1], volume.shape[-3], volume.shape[-2])
        if vshape != self.volume_shape:
            raise ValueError(f"volume (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for "
                             f"{(self.volume_shape[1], self.volume_shape[2], self.volume_shape[0])}")
        flags = (volume.ndim == 5, look_from.ndim == 2)
        if any(flags):
            sizes = {t.shape[0] for t, f in zip((volume, look_from), flags) if f}
            if len(sizes) != 1:
                raise ValueError(f"batched inputs disagree on the batch size: {sorted(sizes)}")
            bs = sizes.pop()
            vol = volume.squeeze(1).permute(0, 3, 1, 2) if flags[0] else volume.squeeze(0).permute(2, 0, 1)
            lf = look_from if flags[1] else look_from.reshape(1, 3).expand(bs, 3)
            return True, vol, lf
        return False, volume.squeeze(0).permute(2, 0, 1), look_from.reshape(1, 3)

    @staticmethod
    def _image(out, batched):
        if batched:  # (BS,W,H) -> flip H -> (BS,1,H,W), as Raycaster
            return torch.flip(out, (2,)).permute(0, 2, 1).unsqueeze(1).contiguous()
        return torch.flip(out, (1,)).t().unsqueeze(0).contiguous()

    def forward(self, volume, look_from):
        """volume ([BS,]1,D,H,W), look_from ([BS,]3) -> ([BS,]1,H,W)."""
        batched, vol, lf = self._determine_batch(volume, look_from)
        res = ProjectFunction.apply(self, vol, lf, batched, self.jitter)
        return self._image(res, batched)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output ({self.output_shape}), mode = {self.mode}, "
                f"Max Samples = {self.max_samples}")
