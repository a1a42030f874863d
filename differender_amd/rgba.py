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
import torch

from . import _layout as L
from . import _native as N
from . import functional as F
from .pose import _pose_grads, _shapes

__all__ = ["RaycasterRGBA", "RgbaRaycastFunction", "RgbaCameraFunction", "interleaved"]


def interleaved(volume):
    """The same logical tensor ([BS,]4,D,H,W) (values, shape, dtype) with the channel axis at stride 1 in memory: a copy unless
    the volume is laid out that way already. A leaf to optimise: interleaved(v).detach().requires_grad_()."""
    if volume.ndim not in (4, 5) or volume.shape[-4] != 4:
        raise ValueError(f"expected an RGBA volume ([BS,]4,D,H,W), got {tuple(volume.shape)}")
    return volume.movedim(-4, -1).contiguous().movedim(-1, -4)


class RgbaRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the RGBA march: `apply(rc, volume, look_from, sampling_rate, batched, jitter)`.
    volume (4,W,D,H) or (BS,4,W,D,H), any strides; look_from (BS,3). Returns (W,H,4) or (BS,W,H,4). No camera gradient: that
    is RgbaCameraFunction."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, look_from, sampling_rate, batched, jitter=True, pose=None):
        volume, cam, _, rays = L.diff_rays(volume, look_from, jitter, rc.output_shape, sampling_rate, rc.fov, rc.near, pose)[:4]
        out, steps = F.march_rgba_fwd(volume, cam, *rays, rc.max_samples, sampling_rate, N.DR_MODE_DIFF)
        ctx.save_for_backward(volume, cam, *rays, out)
        ctx.rc, ctx.sampling_rate, ctx.batched = rc, sampling_rate, batched
        rc._steps = L.unbatch(steps, batched)
        return L.unbatch(out, batched)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, cam, e, x, r, n, out = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None
        g = grad_output if ctx.batched else grad_output[None]
        dv = F.march_rgba_bwd(volume, cam, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, g, out)
        # the plain kernels propagate NaN like the reference: nan_to_num, as Tf2dRaycastFunction does
        return None, torch.nan_to_num(dv), None, None, None, None, None


class RgbaCameraFunction(torch.autograd.Function):
    """`apply(rc, volume, look_from, look_at, up, fov, sampling_rate, batched, jitter)`: RgbaRaycastFunction with gradients for
    the camera as well. look_from (BS,3); look_at, up (BS,3) and fov (BS,) degrees as _layout.pose_rule expanded
    them, or all three None: the fixed camera, whose ray buffers, image and d_vol are RgbaRaycastFunction's, with d look_from
    from march_rgba_bwd_cam. Otherwise the free camera (D15) and march_rgba_bwd_pose."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, look_from, look_at, up, fov, sampling_rate, batched, jitter=True):
        pose = (look_at, up, fov) if L.has_pose(look_at, up, fov) else None
        volume, cam, seed, rays, *posed = L.diff_rays(volume, look_from, jitter, rc.output_shape, sampling_rate, rc.fov, rc.near,
                                                      pose)
        pose9, fov_v = posed if posed else (None, None)
        out, steps = F.march_rgba_fwd(volume, cam, *rays, rc.max_samples, sampling_rate, N.DR_MODE_DIFF)
        ctx.want_cam = any(ctx.needs_input_grad[2:6])
        extra = [t for t in (steps if ctx.want_cam else None, pose9, fov_v) if t is not None]
        ctx.save_for_backward(volume, cam, *rays, out, *extra)
        ctx.has_pose, ctx.has_fov = pose9 is not None, fov_v is not None
        ctx.shapes = _shapes(look_from, look_at, up, fov)
        ctx.rc, ctx.sampling_rate, ctx.batched, ctx.seed = rc, sampling_rate, batched, seed
        rc._steps = L.unbatch(steps, batched)
        return L.unbatch(out, batched)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, cam, e, x, r, n, out, *extra = ctx.saved_tensors
        rc = ctx.rc
        g = grad_output if ctx.batched else grad_output[None]
        dv = None
        grads = [None] * 4
        if ctx.needs_input_grad[1]:
            dv = torch.nan_to_num(F.march_rgba_bwd(volume, cam, e, x, r, n, rc.max_samples, ctx.sampling_rate, g, out))
        if ctx.want_cam:
            steps = extra[0]
            opts = dict(fov_deg=rc.fov, near=rc.near, jitter_seed=ctx.seed)
            if ctx.has_pose:
                d_pose = F.march_rgba_bwd_pose(volume, extra[1], e, x, r, n, steps, rc.max_samples, ctx.sampling_rate, g, out,
                                               fov_v=extra[2] if ctx.has_fov else None, **opts)
            else:   # the fixed camera: look_from's three columns, nothing else came in
                d_cam = F.march_rgba_bwd_cam(volume, cam, e, x, r, n, steps, rc.max_samples, ctx.sampling_rate, g, out, **opts)
                d_pose = torch.cat([d_cam, d_cam.new_zeros(d_cam.shape[0], 7)], 1)
            grads = _pose_grads(d_pose, ctx.shapes, ctx.needs_input_grad[2:6])
        return (None, dv, *grads, None, None, None)


class RaycasterRGBA(L.RayModule):
    """Raycaster of pre-classified RGBA volumes.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster.
    forward(volume ([BS,]4,D,H,W), look_from ([BS,]3)) -> ([BS,]4,H,W).
    camera_grad=True: look_from, look_at, up and fov may require grad and receive their gradients; the images
    and the volume gradient are the default module's."""

    def __init__(self, volume_shape, output_shape, sampling_rate=1.0, jitter=True, max_samples=512, fov=30.0, near=0.1,
                 far=100.0, camera_grad=False):
        if len(tuple(volume_shape)) != 3 or len(tuple(output_shape)) != 2:
            raise ValueError("expected volume_shape (D, H, W) and output_shape (H, W)")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples must be >= 1, got {max_samples}")
        super().__init__(tuple(int(v) for v in volume_shape), output_shape, sampling_rate, jitter, max_samples, fov, near, far)
        self.camera_grad = bool(camera_grad)

    def _determine_batch(self, volume, look_from, pose=None):
        """-> (batched, vol ([BS,] 4, W, D, H) view, look_from (BS, 3)); an un-batched volume is shared by all views.
        pose = (look_at, up, fov): they join the batch rule, and a fourth result holds them as rows per view."""
        if volume.ndim not in (4, 5) or look_from.ndim not in (1, 2):
            raise ValueError("expected volume ([BS,]4,D,H,W), look_from ([BS,]3)")
        if volume.shape[-4] != 4 or look_from.shape[-1] != 3:
            raise ValueError(f"expected volume ([BS,]4,D,H,W), look_from ([BS,]3); got {tuple(volume.shape)}, "
                             f"{tuple(look_from.shape)}")
        self._check_built_for(volume)
        batched, _, lf, *posed = L.batch_rule(look_from, (volume, 5)) if pose is None else L.pose_rule(look_from, pose, (volume, 5))
        return (batched, L.field_view_rgba(volume), lf, *posed)

    def forward(self, volume, look_from, look_at=None, up=None, fov=None):
        """volume ([BS,]4,D,H,W), look_from ([BS,]3) -> ([BS,]4,H,W).
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera for the image and the volume gradient. All
        None: the fixed camera. The four camera tensors may require grad in a module built with camera_grad=True only."""
        posed = L.has_pose(look_at, up, fov)
        if self.camera_grad and L.wants_grad(look_from, look_at, up, fov):
            if posed:
                batched, vol, lf, pose = self._determine_batch(volume, look_from, (look_at, up, fov))
            else:
                (batched, vol, lf), pose = self._determine_batch(volume, look_from), (None, None, None)
            return self._image(RgbaCameraFunction.apply(self, vol, lf, *pose, self.sampling_rate, batched, self.jitter), batched)
        hint = "construct RaycasterRGBA(..., camera_grad=True) for camera gradients"
        L.refuse_pose_grad("RaycasterRGBA", hint, look_from=look_from)
        if posed:
            L.refuse_pose_grad("RaycasterRGBA", hint, look_at=look_at, up=up, fov=fov)
            batched, vol, lf, pose = self._determine_batch(volume, look_from, (look_at, up, fov))
            return self._image(RgbaRaycastFunction.apply(self, vol, lf, self.sampling_rate, batched, self.jitter, pose), batched)
        batched, vol, lf = self._determine_batch(volume, look_from)
        res = RgbaRaycastFunction.apply(self, vol, lf, self.sampling_rate, batched, self.jitter)
        return self._image(res, batched)

    def raycast_nondiff(self, volume, look_from, sampling_rate=None, look_at=None, up=None, fov=None):
        """Non-differentiable render (never jittered); default rate 4x the module's, as Raycaster.raycast_nondiff."""
        pose = None
        if L.has_pose(look_at, up, fov):
            batched, vol, lf, pose = self._determine_batch(volume, look_from, (look_at, up, fov))
        else:
            batched, vol, lf = self._determine_batch(volume, look_from)
        with self._nondiff_rays(vol, lf, sampling_rate, pose) as (sr, vol, cam, rays, *_):
            out, steps = F.march_rgba_fwd(vol, cam, *rays, self.max_samples, sr, N.DR_MODE_NONDIFF)
            self._steps = L.unbatch(steps, batched)
            return L.image(L.unbatch(out, batched))

    def extra_repr(self):
        return f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), Max Samples = {self.max_samples}"
