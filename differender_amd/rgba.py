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

RayBundleRaycasterRGBA marches the same volumes along rays that are inputs, as bundle.RayBundleRaycaster does
for the TF raycaster: random minibatches of rays across views, parallel and cone beams, distorted lenses, per-ray masks.

    rc = RayBundleRaycasterRGBA(volume.shape[-3:], ray_grad=True)
    rgba = rc(volume, origins, directions)             # (4,D,H,W), (..., 3), (..., 3) -> (..., 4)
"""
import functools
import math

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["RaycasterRGBA", "RgbaRaycastFunction", "RgbaCameraFunction", "interleaved", "RayBundleRaycasterRGBA",
           "RgbaRayBundleFunction"]


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


class RgbaRayBundleFunction(torch.autograd.Function):
    """Autograd boundary of the RGBA bundle march: `apply(rc, volume, origins, dirs, sampling_rate, jitter)`. volume (4,W,D,H),
    float32 or float16, any strides; origins, dirs (N,3), the directions of unit length. Returns (N,4). origins and dirs receive
    gradients where they require them (RayBundleRaycasterRGBA refuses that unless built with ray_grad=True)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, origins, dirs, sampling_rate, jitter=True):
        volume = F.as_volume(volume)
        origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
        seed = F.new_jitter_seed() if jitter else 0
        e, x, n = F.bundle_setup(origins, dirs, volume.shape[-3:], sampling_rate, rc.t_near, seed)
        out, steps = F.march_rgba_bundle_fwd(volume, origins, dirs, e, x, n, rc.max_samples, sampling_rate)
        ctx.save_for_backward(volume, origins, dirs, e, x, n, steps, out)
        ctx.rc, ctx.sampling_rate, ctx.seed = rc, sampling_rate, seed
        rc._steps = steps
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, origins, dirs, e, x, n, steps, out = ctx.saved_tensors
        rc, sr = ctx.rc, ctx.sampling_rate
        dv = d_o = d_d = None
        if ctx.needs_input_grad[1]:
            dv = L.sanitised(F.march_rgba_bundle_bwd(volume, origins, dirs, e, x, n, rc.max_samples, sr, grad_output, out))
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            d_o, d_d = F.march_rgba_bundle_bwd_rays(volume, origins, dirs, e, x, n, steps, rc.max_samples, sr, grad_output, out,
                                                    rc.t_near, ctx.seed)
        return (None, dv, d_o if ctx.needs_input_grad[2] else None, d_d if ctx.needs_input_grad[3] else None, None, None)


class RayBundleRaycasterRGBA(torch.nn.Module):
    """The RGBA raycaster over a bundle of rays.

    volume_shape (D, H, W) as for RaycasterRGBA.
    forward(volume (4,D,H,W), origins (...,3), directions (...,3)) -> (...,4) RGBA; one volume per call, float32 or float16, any
    strides (`interleaved(volume)`: a voxel is one load).
    t_near: None marches the reference's line through the box, which also shows what lies behind an origin inside it (so a
    pinhole camera's rays give RaycasterRGBA's image); 0.0 makes every ray start at its origin.
    ray_grad=True: origins and directions may require grad and receive their gradients."""

    def __init__(self, volume_shape, sampling_rate=1.0, jitter=True, max_samples=512, t_near=None, ray_grad=False):
        super().__init__()
        if len(tuple(volume_shape)) != 3:
            raise ValueError("expected volume_shape (D, H, W)")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples must be >= 1, got {max_samples}")
        if t_near is not None and math.isnan(float(t_near)):
            raise ValueError("t_near must be a number or None")
        self.volume_shape = (int(volume_shape[2]), int(volume_shape[0]), int(volume_shape[1]))  # (W, D, H), as RaycasterRGBA
        self.sampling_rate, self.jitter, self.max_samples = sampling_rate, jitter, int(max_samples)
        self.t_near = None if t_near is None else float(t_near)
        self.ray_grad = bool(ray_grad)
        self._steps = None
        N.lib()  # fail loudly at construction time if the HIP library is missing

    def _check(self, volume, origins, directions):
        expected = "volume (4,D,H,W), origins (...,3), directions (...,3) of one shape"
        if volume.ndim != 4 or volume.shape[0] != 4:
            raise ValueError(f"expected {expected}; got volume {tuple(volume.shape)}")
        w, d, h = self.volume_shape
        if tuple(volume.shape[-3:]) != (d, h, w):
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {(d, h, w)}")
        if origins.ndim < 1 or origins.shape[-1] != 3 or origins.shape != directions.shape or origins.numel() == 0:
            raise ValueError(f"expected {expected}; got origins {tuple(origins.shape)}, directions {tuple(directions.shape)}")

    @staticmethod
    def _check_devices(volume, origins, directions):
        for name, t in (("volume", volume), ("origins", origins), ("directions", directions)):
            F._require_gpu(t, name)
            if t.device != volume.device:
                raise ValueError(f"{name} lives on {t.device}, the volume on {volume.device}")

    def forward(self, volume, origins, directions):
        """volume (4,D,H,W), origins, directions (...,3) -> (...,4). The directions are normalised here, in torch (a zero-length
        one raises), so their gradient is that of the direction handed in."""
        self._check(volume, origins, directions)
        if not self.ray_grad:
            L.refuse_pose_grad("RayBundleRaycasterRGBA", "construct RayBundleRaycasterRGBA(..., ray_grad=True) for ray gradients",
                               origins=origins, directions=directions)
        length = torch.sqrt((directions * directions).sum(-1, keepdim=True))
        if bool((length == 0).any()):
            raise ValueError("a direction has zero length")
        self._check_devices(volume, origins, directions)
        dirs = (directions / length).reshape(-1, 3)
        out = RgbaRayBundleFunction.apply(self, L.field_view_rgba(volume), origins.reshape(-1, 3), dirs, self.sampling_rate,
                                          self.jitter)
        steps = self._steps
        self._steps = None if steps is None else steps.reshape(origins.shape[:-1])
        return out.reshape(*origins.shape[:-1], 4)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Max Samples = {self.max_samples}, t_near = {self.t_near}, "
                f"ray_grad = {self.ray_grad}")
