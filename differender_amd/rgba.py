"""Differentiable rendering of pre-classified ("pre-shaded") RGBA volumes.

The third classical optical model beside the transfer-function marches (emission-absorption through a TF) and the projections
(absorption only): the volume carries its own colour and opacity per voxel and is composited directly, with a gradient to all
four channels. No transfer function has to be known or guessed to recover a volume from images; baked or segmented colour
volumes and per-voxel radiance grids render as they are.

    rc = RaycasterRGBA(volume.shape[-3:], (H, W))
    img = rc(volume, look_from)              # volume ([BS,]4,D,H,W), look_from ([BS,]3) -> ([BS,]4,H,W)

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster. There is no shading. The camera is
differentiable on request: a module built with camera_grad=True gives look_from, look_at, up and fov their
gradients, as Raycaster and Projector do (pose.py); the default module refuses a camera tensor that requires grad.

    rc = RaycasterRGBA(volume.shape[-3:], (H, W), camera_grad=True)
    loss(rc(volume, look_from, look_at=look_at, up=up, fov=fov)).backward()    # look_from.grad ... fov.grad (per degree)

`interleaved(volume)` stores the four channels of a voxel next to each other, which lets the kernels fetch a voxel with one
load; the rendered bits are the same.
"""
import functools

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["RaycasterRGBA", "RgbaRaycastFunction", "RgbaCameraFunction", "interleaved"]


def interleaved(volume):
    """The same logical tensor ([BS,]4,D,H,W) (values, shape, dtype) with the channel axis at stride 1 in memory: a copy unless
    the volume is laid out that way already. A leaf to optimise: interleaved(v).detach().requires_grad_()."""
    if volume.ndim not in (4, 5) or volume.shape[-4] != 4:
        raise ValueError(f"expected an RGBA volume ([BS,]4,D,H,W), got {tuple(volume.shape)}")
    return volume.movedim(-4, -1).contiguous().movedim(-1, -4)


def _forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter, pose, camera=None, needs=()):
    march = lambda volume, cam, rays: F.march_rgba_fwd(volume, cam, *rays, rc.max_samples, sampling_rate, N.DR_MODE_DIFF)
    return L.march_forward(ctx, rc, march, volume, (), look_from, sampling_rate, batched, jitter, pose, camera, needs)


def _backward(ctx, grad_output, need_vol, need_camera=()):
    """-> (d_vol, [d look_from, d look_at, d up, d fov]): the volume backward first, the camera backward behind it on the same
    stream; neither is called where its gradient is not needed."""
    (volume, e, x, r, n, out), cam, steps, pose9, fov_v = L.saved_rays(ctx)
    g = grad_output if ctx.batched else grad_output[None]
    dv = None
    if need_vol:
        dv = L.sanitised(F.march_rgba_bwd(volume, cam, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, g, out))
    march = (e, x, r, n, steps, ctx.rc.max_samples, ctx.sampling_rate, g, out)
    return dv, L.camera_grads(ctx, need_camera, functools.partial(F.march_rgba_bwd_cam, volume, cam, *march),
                              functools.partial(F.march_rgba_bwd_pose, volume, pose9, *march, fov_v=fov_v))


class RgbaRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the RGBA march: `apply(rc, volume, look_from, sampling_rate, batched, jitter)`.
    volume (4,W,D,H) or (BS,4,W,D,H), any strides; look_from (BS,3). Returns (W,H,4) or (BS,W,H,4). No camera gradient: that
    is RgbaCameraFunction."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter=True, pose=None):
        return _forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter, pose)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        return None, _backward(ctx, grad_output, ctx.needs_input_grad[1])[0], None, None, None, None, None


class RgbaCameraFunction(torch.autograd.Function):
    """`apply(rc, volume, look_from, look_at, up, fov, sampling_rate, batched, jitter)`: RgbaRaycastFunction with gradients for
    the camera as well. look_from (BS,3); look_at, up (BS,3) and fov (BS,) degrees as _layout.pose_rule expanded
    them, or all three None: the fixed camera, whose ray buffers, image and d_vol are RgbaRaycastFunction's, with d look_from
    from march_rgba_bwd_cam. Otherwise the free camera (D15) and march_rgba_bwd_pose."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, look_from, look_at, up, fov, sampling_rate, batched, jitter=True):
        return _forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter, L.pose_or_none(look_at, up, fov),
                        (look_from, look_at, up, fov), ctx.needs_input_grad[2:6])

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        dv, camera = _backward(ctx, grad_output, ctx.needs_input_grad[1], ctx.needs_input_grad[2:6])
        return (None, dv, *camera, None, None, None)


class RaycasterRGBA(L.RayModule):
    """Raycaster of pre-classified RGBA volumes.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster.
    forward(volume ([BS,]4,D,H,W), look_from ([BS,]3)) -> ([BS,]4,H,W).
    camera_grad=True: look_from, look_at, up and fov may require grad and receive their gradients; the images
    and the volume gradient are the default module's."""

    def __init__(self, volume_shape, output_shape, sampling_rate=1.0, jitter=True, max_samples=512, fov=30.0, near=0.1,
                 far=100.0, camera_grad=False):
        self._check_built(volume_shape, output_shape, max_samples=max_samples)
        super().__init__(tuple(int(v) for v in volume_shape), output_shape, sampling_rate, jitter, max_samples, fov, near, far)
        self.camera_grad = bool(camera_grad)

    def _batch(self, volume, look_from, pose=None):
        """-> (batched, vol ([BS,] 4, W, D, H) view, look_from (BS, 3), pose); an un-batched volume is shared by all views.
        pose = (look_at, up, fov): they join the batch rule and come back as rows per view; else None."""
        L.check_inputs("volume ([BS,]4,D,H,W), look_from ([BS,]3)", (volume, 5, -4, 4), (look_from, 2, -1, 3))
        self._check_built_for(volume)
        batched, lf, pose = L.views(look_from, pose, (volume, 5))
        return batched, L.field_view_rgba(volume), lf, pose

    def forward(self, volume, look_from, look_at=None, up=None, fov=None):
        """volume ([BS,]4,D,H,W), look_from ([BS,]3) -> ([BS,]4,H,W).
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera for the image and the volume gradient. All
        None: the fixed camera. The four camera tensors may require grad in a module built with camera_grad=True only."""
        pose = L.pose_or_none(look_at, up, fov)
        if self.camera_grad and L.wants_grad(look_from, look_at, up, fov):
            batched, vol, lf, pose = self._batch(volume, look_from, pose)
            res = RgbaCameraFunction.apply(self, vol, lf, *(pose or (None, None, None)), self.sampling_rate, batched, self.jitter)
            return self._image(res, batched)
        hint = "construct RaycasterRGBA(..., camera_grad=True) for camera gradients"
        L.refuse_pose_grad("RaycasterRGBA", hint, look_from=look_from, look_at=look_at, up=up, fov=fov)
        batched, vol, lf, pose = self._batch(volume, look_from, pose)
        res = RgbaRaycastFunction.apply(self, vol, lf, self.sampling_rate, batched, self.jitter, pose)
        return self._image(res, batched)

    def raycast_nondiff(self, volume, look_from, sampling_rate=None, look_at=None, up=None, fov=None):
        """Non-differentiable render (never jittered); default rate 4x the module's, as Raycaster.raycast_nondiff."""
        batched, vol, lf, pose = self._batch(volume, look_from, L.pose_or_none(look_at, up, fov))
        march = lambda vol, cam, rays, sr: F.march_rgba_fwd(vol, cam, *rays, self.max_samples, sr, N.DR_MODE_NONDIFF)
        return self._raycast_nondiff(vol, lf, sampling_rate, pose, batched, march)

    def extra_repr(self):
        return f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), Max Samples = {self.max_samples}"
