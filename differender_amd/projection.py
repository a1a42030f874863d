"""Differentiable X-ray line-integral and maximum intensity projections of a scalar volume.

The two standard views of a volume beside compositing: the line integral int mu ds along each ray (the forward model of
tomography, a digitally reconstructed radiograph) and the maximum intensity projection (angiography). The samples are those of
Raycaster at the same sampling rate, camera and jitter; there is no transfer function and no shading.

    proj = Projector(volume.shape[-3:], (H, W), mode="sum")
    line_integral = proj(mu, look_from)          # mu ([BS,]1,D,H,W), look_from ([BS,]3) -> ([BS,]1,H,W)
    radiograph = torch.exp(-line_integral)       # Beer-Lambert: transmitted intensity of a monochromatic beam

RayBundleProjector projects along rays that are an input -- a parallel beam, a cone beam with a flat detector,
a random minibatch of rays across views -- instead of one pinhole camera's:

    proj = RayBundleProjector(volume.shape[-3:], mode="sum")
    sinogram_row = proj(mu, *orthographic_rays(...))      # origins, directions (..., 3) -> (...)

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster. Gradients flow to the volume (a
back-projection) and to look_from (when it requires grad). Lengths are in world units of the renderer's [-1, 1]^3 box: a
constant volume c gives c times the chord of the ray through the box.
"""
import math

import torch

from . import _layout as L
from . import functional as F

__all__ = ["Projector", "ProjectFunction", "RayBundleProjector", "RayBundleProjectFunction"]

_MODES = ("sum", "max")


def _forward(ctx, pj, volume, look_from, batched, jitter, pose=None):
    """The forward of ProjectFunction and, with pose = (look_at, up, fov), of pose.PoseProjectFunction. Saved: the volume, cam
    (views, 3) -- with a pose the pose (views, 9) in its place --, the ray buffers, arg_max for "max" only, fov_v where given."""
    volume, cam, seed, rays, pose9, fov_v = L.diff_rays(volume, look_from, jitter, pj.output_shape, pj.sampling_rate, pj.fov,
                                                        pj.near, pose)
    out, arg = F.project_fwd(volume, cam, *rays, pj.max_samples, pj.mode)
    ctx.save_for_backward(volume, cam if pose9 is None else pose9, *rays, *((arg,) if arg is not None else ()),
                          *((fov_v,) if fov_v is not None else ()))
    ctx.has_arg, ctx.has_fov = arg is not None, fov_v is not None
    ctx.pj, ctx.batched, ctx.seed = pj, batched, seed
    ctx.shapes = L.camera_shapes(look_from, *(pose or ()))
    return L.unbatch(out, batched)


class ProjectFunction(torch.autograd.Function):
    """Autograd boundary of the projections: `apply(pj, volume, look_from, batched, jitter)`. volume (W,D,H) or (BS,W,D,H),
    any strides; look_from (BS,3). Returns (W,H) or (BS,W,H)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pj, volume, look_from, batched, jitter=True):
        return _forward(ctx, pj, volume, look_from, batched, jitter)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, cam, e, x, r, n, *arg = ctx.saved_tensors
        pj, arg = ctx.pj, arg[0] if arg else None
        g = grad_output if ctx.batched else grad_output[None]
        dv = d_cam = None
        if ctx.needs_input_grad[1]:
            dv = torch.nan_to_num(F.project_bwd(volume, cam, e, x, r, n, g, pj.max_samples, pj.mode, arg))
        if ctx.needs_input_grad[2]:   # after project_bwd, on the same stream
            d_cam = F.project_bwd_cam(volume, cam, e, x, r, n, g, pj.max_samples, pj.mode, arg, fov_deg=pj.fov, near=pj.near,
                                      jitter_seed=ctx.seed)
            d_cam = L.reduce_to(d_cam, *ctx.shapes[0])
        return None, dv, d_cam, None, None


class Projector(L.RayModule):
    """Line-integral (mode "sum") or maximum intensity ("max") projection of a volume.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster; sampling_rate, jitter, fov, near and far as for Raycaster.
    max_samples None: every sample of every ray; an integer truncates the rays (and the integral) after that many samples.
    forward(volume ([BS,]1,D,H,W), look_from ([BS,]3)) -> ([BS,]1,H,W). For "sum" the result is D * sum of the samples,
    D = (exit - entry) / n the sample spacing in world units; torch.exp(-proj) is the Beer-Lambert transmission."""

    def __init__(self, volume_shape, output_shape, mode="sum", sampling_rate=1.0, jitter=True, max_samples=None, fov=30.0,
                 near=0.1, far=100.0):
        self._check_built(volume_shape, output_shape)
        if min(volume_shape) < 2 or min(output_shape) < 1:
            raise ValueError(f"volume_shape needs >= 2 voxels per axis and output_shape >= 1 pixel, got {tuple(volume_shape)}, "
                             f"{tuple(output_shape)}")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'sum' or 'max', got {mode!r}")
        if not (sampling_rate > 0):
            raise ValueError(f"sampling_rate must be > 0, got {sampling_rate}")
        if max_samples is not None and int(max_samples) < 1:
            raise ValueError(f"max_samples must be None or >= 1, got {max_samples}")
        super().__init__(volume_shape, output_shape, float(sampling_rate), jitter, max_samples, fov, near, far)
        self.mode = mode

    def _batch(self, volume, look_from, pose=None):
        """-> (batched, vol ([BS,] W, D, H) view, look_from (BS, 3), pose); an un-batched volume is shared by all views.
        pose = (look_at, up, fov): they join the batch rule and come back as rows per view; else None."""
        L.check_inputs("volume ([BS,]1,D,H,W) and look_from ([BS,]3)", (volume, 5, -4, 1), (look_from, 2, -1, 3))
        self._check_built_for(volume)
        batched, lf, pose = L.views(look_from, pose, (volume, 5))
        return batched, L.field_view(volume), lf, pose

    @staticmethod
    def _image(out, batched):
        """([BS,]W,H) -> ([BS,]1,H,W): the shared orientation at K = 1."""
        return L.image(out.unsqueeze(-1))

    def forward(self, volume, look_from, look_at=None, up=None, fov=None):
        """volume ([BS,]1,D,H,W), look_from ([BS,]3) -> ([BS,]1,H,W).
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera (pose.py) and its gradients, as
        Raycaster.forward; all None: the fixed camera."""
        batched, vol, lf, pose = self._batch(volume, look_from, L.pose_or_none(look_at, up, fov))
        if pose is None:
            return self._image(ProjectFunction.apply(self, vol, lf, batched, self.jitter), batched)
        from .pose import PoseProjectFunction
        return self._image(PoseProjectFunction.apply(self, vol, lf, *pose, batched, self.jitter), batched)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output ({self.output_shape}), mode = {self.mode}, "
                f"Max Samples = {self.max_samples}")


class RayBundleProjectFunction(torch.autograd.Function):
    """Autograd boundary of the bundle projections: `apply(pj, volume, origins, dirs, jitter)`. volume (W,D,H), any strides;
    origins, dirs (N,3), the directions of unit length. Returns (N,). origins and dirs receive gradients where they require them
    (RayBundleProjector refuses that unless built with ray_grad=True)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pj, volume, origins, dirs, jitter=True):
        volume = F.as_volume(volume)
        origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
        seed = F.new_jitter_seed() if jitter else 0
        e, x, n = F.bundle_setup(origins, dirs, volume.shape[-3:], pj.sampling_rate, pj.t_near, seed)
        out, arg = F.project_bundle_fwd(volume, origins, dirs, e, x, n, pj.max_samples, pj.mode)
        ctx.save_for_backward(volume, origins, dirs, e, x, n, *((arg,) if arg is not None else ()))
        ctx.pj, ctx.seed = pj, seed
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, origins, dirs, e, x, n, *arg = ctx.saved_tensors
        pj, arg = ctx.pj, arg[0] if arg else None
        dv = d_o = d_d = None
        if ctx.needs_input_grad[1]:
            dv = torch.nan_to_num(F.project_bundle_bwd(volume, origins, dirs, e, x, n, grad_output, pj.max_samples, pj.mode, arg))
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            d_o, d_d = F.project_bundle_bwd_rays(volume, origins, dirs, e, x, n, grad_output, pj.max_samples, pj.mode, arg,
                                                 pj.t_near, ctx.seed)
        return (None, dv, d_o if ctx.needs_input_grad[2] else None, d_d if ctx.needs_input_grad[3] else None, None)


class RayBundleProjector(torch.nn.Module):
    """Line-integral (mode "sum") or maximum intensity ("max") projection of a volume along a bundle of rays.

    volume_shape (D, H, W), mode, sampling_rate, jitter and max_samples as for Projector.
    forward(volume (1,D,H,W), origins (...,3), directions (...,3)) -> (...); one volume per call. Rays live in look_from's world
    coordinates (the volume fills [-1, 1]^3): bundle.orthographic_rays is a parallel beam, bundle.cone_beam_rays a point source
    and a flat detector, bundle.pinhole_rays Projector's own rays. The volume backward is fastest where 256 consecutive rays
    are neighbours: order an image's rays with bundle.tile_order.
    t_near: None integrates along the reference's whole line through the box, also behind an origin inside it; 0.0 makes every
    ray start at its origin.
    ray_grad=True: origins and directions may require grad and receive their gradients."""

    def __init__(self, volume_shape, mode="sum", sampling_rate=1.0, jitter=True, max_samples=None, t_near=None, ray_grad=False):
        super().__init__()
        if len(tuple(volume_shape)) != 3:
            raise ValueError("expected volume_shape (D, H, W)")
        if min(volume_shape) < 2:
            raise ValueError(f"volume_shape needs >= 2 voxels per axis, got {tuple(volume_shape)}")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'sum' or 'max', got {mode!r}")
        if not (sampling_rate > 0):
            raise ValueError(f"sampling_rate must be > 0, got {sampling_rate}")
        if max_samples is not None and int(max_samples) < 1:
            raise ValueError(f"max_samples must be None or >= 1, got {max_samples}")
        if t_near is not None and math.isnan(float(t_near)):
            raise ValueError("t_near must be a number or None")
        self.volume_shape = (int(volume_shape[2]), int(volume_shape[0]), int(volume_shape[1]))  # (W, D, H), as Raycaster
        self.mode, self.sampling_rate, self.jitter = mode, float(sampling_rate), jitter
        self.max_samples = None if max_samples is None else int(max_samples)
        self.t_near = None if t_near is None else float(t_near)
        self.ray_grad = bool(ray_grad)
        from . import _native
        _native.lib()  # fail loudly at construction time if the HIP library is missing

    def _check(self, volume, origins, directions):
        expected = "volume (1,D,H,W), origins (...,3), directions (...,3) of one shape"
        if volume.ndim != 4 or volume.shape[0] != 1:
            raise ValueError(f"expected {expected}; got volume {tuple(volume.shape)}")
        w, d, h = self.volume_shape
        if tuple(volume.shape[-3:]) != (d, h, w):
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {(d, h, w)}")
        if origins.ndim < 1 or origins.shape[-1] != 3 or origins.shape != directions.shape or origins.numel() == 0:
            raise ValueError(f"expected {expected}; got origins {tuple(origins.shape)}, directions {tuple(directions.shape)}")

    def forward(self, volume, origins, directions):
        """volume (1,D,H,W), origins, directions (...,3) -> (...). The directions are normalised here, in torch (a zero-length
        one raises), so their gradient is that of the direction handed in."""
        self._check(volume, origins, directions)
        if not self.ray_grad:
            L.refuse_pose_grad("RayBundleProjector", "construct RayBundleProjector(..., ray_grad=True) for ray gradients",
                               origins=origins, directions=directions)
        length = torch.sqrt((directions * directions).sum(-1, keepdim=True))
        if bool((length == 0).any()):
            raise ValueError("a direction has zero length")
        for name, t in (("volume", volume), ("origins", origins), ("directions", directions)):
            F._require_gpu(t, name)
            if t.device != volume.device:
                raise ValueError(f"{name} lives on {t.device}, the volume on {volume.device}")
        out = RayBundleProjectFunction.apply(self, L.field_view(volume), origins.reshape(-1, 3), (directions / length).reshape(-1, 3),
                                             self.jitter)
        return out.reshape(origins.shape[:-1])

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), mode = {self.mode}, Max Samples = {self.max_samples}, t_near = {self.t_near}, "
                f"ray_grad = {self.ray_grad}")
