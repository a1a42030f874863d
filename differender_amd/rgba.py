"""Differentiable rendering of pre-classified ("pre-shaded") RGBA volumes.

The third classical optical model beside the transfer-function marches (emission-absorption through a TF) and the projections
(absorption only): the volume carries its own colour and opacity per voxel and is composited directly, with a gradient to all
four channels. No transfer function has to be known or guessed to recover a volume from images; baked or segmented colour
volumes and per-voxel radiance grids render as they are.

    rc = RaycasterRGBA(volume.shape[-3:], (H, W))
    img = rc(volume, look_from)              # volume ([BS,]4,D,H,W), look_from ([BS,]3) -> ([BS,]4,H,W)

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster. There is no shading and no gradient
w.r.t. look_from. `interleaved(volume)` stores the four channels of a voxel next to each other, which lets the kernels fetch a
voxel with one load; the rendered bits are the same.
"""
import torch

from . import _native as N
from . import functional as F

__all__ = ["RaycasterRGBA", "RgbaRaycastFunction", "interleaved"]


def interleaved(volume):
    """The same logical tensor ([BS,]4,D,H,W) (values, shape, dtype) with the channel axis at stride 1 in memory: a copy unless
    the volume is laid out that way already. A leaf to optimise: interleaved(v).detach().requires_grad_()."""
    if volume.ndim not in (4, 5) or volume.shape[-4] != 4:
        raise ValueError(f"expected an RGBA volume ([BS,]4,D,H,W), got {tuple(volume.shape)}")
    return volume.movedim(-4, -1).contiguous().movedim(-1, -4)


class RgbaRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the RGBA march: `apply(rc, volume, look_from, sampling_rate, batched, jitter)`.
    volume (4,W,D,H) or (BS,4,W,D,H), any strides; look_from (BS,3). Returns (W,H,4) or (BS,W,H,4). d look_from is not
    defined."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter=True):
        cam = look_from.reshape(-1, 3)
        volume = F.as_volume(volume)
        seed = F.new_jitter_seed() if jitter else 0
        e, x, r, n = F.ray_setup(cam, rc.output_shape, volume.shape[-3:], sampling_rate, rc.fov, rc.near, seed)
        out, steps = F.march_rgba_fwd(volume, cam, e, x, r, n, rc.max_samples, sampling_rate, N.DR_MODE_DIFF)
        ctx.save_for_backward(volume, cam, e, x, r, n, out)
        ctx.rc, ctx.sampling_rate, ctx.batched = rc, sampling_rate, batched
        rc._steps = steps if batched else steps[0]
        return out if batched else out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, cam, e, x, r, n, out = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        g = grad_output if ctx.batched else grad_output[None]
        dv = F.march_rgba_bwd(volume, cam, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, g, out)
        # the plain kernels propagate NaN like the reference: nan_to_num, as Tf2dRaycastFunction does
        return None, torch.nan_to_num(dv), None, None, None, None


class RaycasterRGBA(torch.nn.Module):
    """Raycaster of pre-classified RGBA volumes.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster.
    forward(volume ([BS,]4,D,H,W), look_from ([BS,]3)) -> ([BS,]4,H,W)."""

    def __init__(self, volume_shape, output_shape, sampling_rate=1.0, jitter=True, max_samples=512, fov=30.0, near=0.1,
                 far=100.0):
        super().__init__()
        if len(tuple(volume_shape)) != 3 or len(tuple(output_shape)) != 2:
            raise ValueError("expected volume_shape (D, H, W) and output_shape (H, W)")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples must be >= 1, got {max_samples}")
        self.user_shape = tuple(int(v) for v in volume_shape)
        self.volume_shape = (self.user_shape[2], self.user_shape[0], self.user_shape[1])  # (W, D, H), as Raycaster
        self.output_shape = tuple(output_shape)
        self.sampling_rate = sampling_rate
        self.jitter = jitter
        self.max_samples = max_samples
        self.fov, self.near, self.far = fov, near, far
        self._steps = None
        N.lib()  # fail loudly at construction time if the HIP library is missing

    def _determine_batch(self, volume, look_from):
        """-> (batched, vol ([BS,] 4, W, D, H) view, look_from (BS, 3)); an un-batched volume is shared by all views."""
        if volume.ndim not in (4, 5) or look_from.ndim not in (1, 2):
            raise ValueError("expected volume ([BS,]4,D,H,W), look_from ([BS,]3)")
        if volume.shape[-4] != 4 or look_from.shape[-1] != 3:
            raise ValueError(f"expected volume ([BS,]4,D,H,W), look_from ([BS,]3); got {tuple(volume.shape)}, "
                             f"{tuple(look_from.shape)}")
        if tuple(volume.shape[-3:]) != self.user_shape:
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {self.user_shape}")
        flags = (volume.ndim == 5, look_from.ndim == 2)
        if any(flags):
            sizes = {t.shape[0] for t, f in zip((volume, look_from), flags) if f}
            if len(sizes) != 1:
                raise ValueError(f"batched inputs disagree on the batch size: {sorted(sizes)}")
            bs = sizes.pop()
            vol = volume.permute(0, 1, 4, 2, 3) if flags[0] else volume.permute(0, 3, 1, 2)
            lf = look_from if flags[1] else look_from.reshape(1, 3).expand(bs, 3)
            return True, vol, lf
        return False, volume.permute(0, 3, 1, 2), look_from.reshape(1, 3)

    @staticmethod
    def _image(out, batched):
        if batched:  # (BS,W,H,4) -> flip H -> (BS,4,H,W), as Raycaster
            return torch.flip(out, (2,)).permute(0, 3, 2, 1).contiguous()
        return torch.flip(out, (1,)).permute(2, 1, 0).contiguous()

    def forward(self, volume, look_from):
        """volume ([BS,]4,D,H,W), look_from ([BS,]3) -> ([BS,]4,H,W)."""
        if torch.is_grad_enabled() and look_from.requires_grad:
            raise ValueError("RaycasterRGBA has no gradient w.r.t. look_from: use volume_raycaster.Raycaster (scalar volume and "
                             "transfer function) for camera gradients, or pass look_from.detach()")
        batched, vol, lf = self._determine_batch(volume, look_from)
        res = RgbaRaycastFunction.apply(self, vol, lf, self.sampling_rate, batched, self.jitter)
        return self._image(res, batched)

    def raycast_nondiff(self, volume, look_from, sampling_rate=None):
        """Non-differentiable render (never jittered); default rate 4x the module's, as Raycaster.raycast_nondiff."""
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            batched, vol, lf = self._determine_batch(volume, look_from)
            sr = sampling_rate if sampling_rate is not None else 4.0 * self.sampling_rate
            vol = F.as_volume(vol)
            cam = lf.reshape(-1, 3).float()
            e, x, r, n = F.ray_setup(cam, self.output_shape, vol.shape[-3:], sr, self.fov, self.near, 0)
            out, steps = F.march_rgba_fwd(vol, cam, e, x, r, n, self.max_samples, sr, N.DR_MODE_NONDIFF)
            self._steps = steps if batched else steps[0]
            return self._image(out if batched else out[0], batched)

    def extra_repr(self):
        return f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), Max Samples = {self.max_samples}"
