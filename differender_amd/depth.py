"""Differentiable depth maps of the 1-D TF raycaster: ray-depth moments with all gradients.

Raycaster says what colour a ray collects; DepthRaycaster says where along the ray it collects it. With the samples, the
classification and the opacities of Raycaster's differentiable march (no shading: depth needs the table's alpha alone), a ray
composites the distance t of each sample from look_from, in world units along the unit ray direction, and its square:

    rc = DepthRaycaster(volume.shape[-3:], (H, W), R)
    m = rc(volume, tf, look_from)            # ([BS,]3,H,W) = (M1, M2, A): sum w t, sum w t^2, sum w, w = T op
    depth = expected_depth(m)                # M1 / A where A > eps, else `background`
    var = depth_variance(m)                  # max(M2 / A - (M1 / A)^2, 0): small for a sharp surface

Gradients flow to the volume and the TF (its alpha row only: the colour rows receive exact zeros); a module built with
camera_grad=True gives look_from, look_at, up and fov their gradients as well (the free camera of DESIGN.md D15), which is
what registering a camera against a depth image needs (examples/depth_pose_synthetic.py). Batching, image orientation and AMP
casting are those of volume_raycaster.Raycaster; channel A equals the alpha channel of Raycaster's image for the same inputs.

RayBundleDepthRaycaster takes rays as inputs, as bundle.RayBundleRaycaster does for colour: range data is rays
(a LiDAR or time-of-flight scan, sparse depth from structure-from-motion), and depth-supervised fitting mixes rays of many
views in one minibatch (examples/depth_ray_batch_synthetic.py):

    rc = RayBundleDepthRaycaster(volume.shape[-3:], R, t_near=0.0, ray_grad=True)
    m = rc(volume, tf, origins, directions)  # (..., 3), (..., 3) -> (..., 3) = (M1, M2, A), channel LAST
    rng = ray_expected_depth(m)              # (...): M1 / A, the distance from each ray's origin

Jitter: every jittered forward draws its own seed (functional.new_jitter_seed), so a jittered depth render and a jittered colour
render of the same training step sample their rays at DIFFERENT offsets. Render with jitter=False where the two must match
sample for sample.
"""
import functools

import torch

from . import _layout as L
from . import functional as F
from .bundle import RayBundleRaycaster

__all__ = ["DepthRaycaster", "DepthRaycastFunction", "DepthCameraFunction", "expected_depth", "depth_variance",
           "RayBundleDepthRaycaster", "RayBundleDepthFunction", "ray_expected_depth", "ray_depth_variance"]


def _moments(m):
    if not torch.is_tensor(m) or m.ndim < 3 or m.shape[-3] != 3:
        raise ValueError(f"expected the moments ([BS,]3,H,W) = (M1, M2, A) of DepthRaycaster, got "
                         f"{tuple(m.shape) if torch.is_tensor(m) else type(m).__name__}")
    return m[..., 0, :, :], m[..., 1, :, :], m[..., 2, :, :]


def expected_depth(m, background=0.0, eps=1e-6):
    """([BS,]3,H,W) moments -> ([BS,]H,W): the opacity-weighted mean distance M1 / A of a ray's samples where A > eps, and
    `background` (no gradient) where the ray collected nothing. Plain torch: autograd carries it into the moments."""
    m1, _, a = _moments(m)
    hit = a > eps
    return torch.where(hit, m1 / torch.where(hit, a, torch.ones_like(a)), torch.full_like(a, float(background)))


def depth_variance(m, eps=1e-6):
    """([BS,]3,H,W) moments -> ([BS,]H,W): the opacity-weighted variance max(M2 / A - (M1 / A)^2, 0) of the samples' distances
    where A > eps, 0 elsewhere. Small where the ray meets a sharp surface: a prior beside fused_tv3d_loss."""
    m1, m2, a = _moments(m)
    hit = a > eps
    safe = torch.where(hit, a, torch.ones_like(a))
    mean = m1 / safe
    return torch.where(hit, torch.clamp(m2 / safe - mean * mean, min=0.0), torch.zeros_like(a))


def _ray_moments(m):
    if not torch.is_tensor(m) or m.ndim < 1 or m.shape[-1] != 3:
        raise ValueError(f"expected the channel-last moments (...,3) = (M1, M2, A) of RayBundleDepthRaycaster, got "
                         f"{tuple(m.shape) if torch.is_tensor(m) else type(m).__name__}")
    return m[..., 0], m[..., 1], m[..., 2]


def ray_expected_depth(m, background=0.0, eps=1e-6):
    """(...,3) channel-last moments of RayBundleDepthRaycaster -> (...): expected_depth's formula, M1 / A where A > eps and
    `background` (no gradient) elsewhere. Plain torch."""
    m1, _, a = _ray_moments(m)
    hit = a > eps
    return torch.where(hit, m1 / torch.where(hit, a, torch.ones_like(a)), torch.full_like(a, float(background)))


def ray_depth_variance(m, eps=1e-6):
    """(...,3) channel-last moments of RayBundleDepthRaycaster -> (...): depth_variance's formula, max(M2 / A - (M1 / A)^2, 0)
    where A > eps, 0 elsewhere. Plain torch."""
    m1, m2, a = _ray_moments(m)
    hit = a > eps
    safe = torch.where(hit, a, torch.ones_like(a))
    mean = m1 / safe
    return torch.where(hit, torch.clamp(m2 / safe - mean * mean, min=0.0), torch.zeros_like(a))


def _forward(ctx, rc, volume, tf, look_from, sampling_rate, batched, jitter, pose, camera=None, needs=()):
    tf = tf.float().contiguous()
    march = lambda volume, cam, rays: F.march_depth_fwd(volume, tf, cam, *rays, rc.max_samples, sampling_rate)
    return L.march_forward(ctx, rc, march, volume, (tf,), look_from, sampling_rate, batched, jitter, pose, camera, needs)


def _backward(ctx, grad_output, need_camera=()):
    """-> (d_vol, d_tf, [d look_from, d look_at, d up, d fov]): the volume / TF backward first, the camera backward (where
    needed) behind it on the same stream."""
    (volume, tf, e, x, r, n, out), cam, steps, pose9, fov_v = L.saved_rays(ctx)
    g = grad_output if ctx.batched else grad_output[None]
    dv, dt = F.march_depth_bwd(volume, tf, cam, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, g, out,
                               want_vol=ctx.needs_input_grad[1], want_tf=ctx.needs_input_grad[2])
    march = (e, x, r, n, steps, ctx.rc.max_samples, ctx.sampling_rate, g, out)
    camera = L.camera_grads(ctx, need_camera, functools.partial(F.march_depth_bwd_cam, volume, tf, cam, *march),
                            functools.partial(F.march_depth_bwd_pose, volume, tf, pose9, *march, fov_v=fov_v))
    return L.sanitised(dv), L.sanitised(dt), camera


class DepthRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the depth march: `apply(rc, volume, tf, look_from, sampling_rate, batched, jitter, pose)`.
    volume (W,D,H) or (BS,W,D,H), any strides; tf (R,4) or (BS,R,4); look_from (views,3). Returns (W,H,4) or (BS,W,H,4) =
    (M1, M2, 0, A). No camera gradient: that is DepthCameraFunction."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf, look_from, sampling_rate, batched, jitter=True, pose=None):
        return _forward(ctx, rc, volume, tf, look_from, sampling_rate, batched, jitter, pose)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        return (None, *_backward(ctx, grad_output)[:2], None, None, None, None, None)


class DepthCameraFunction(torch.autograd.Function):
    """`apply(rc, volume, tf, look_from, look_at, up, fov, sampling_rate, batched, jitter)`: DepthRaycastFunction with gradients
    for the camera as well. look_from (BS,3); look_at, up (BS,3) and fov (BS,) degrees as _layout.pose_rule expanded them, or
    all three None: the fixed camera, with d look_from from march_depth_bwd_cam. Otherwise the free camera (D15) and
    march_depth_bwd_pose."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf, look_from, look_at, up, fov, sampling_rate, batched, jitter=True):
        return _forward(ctx, rc, volume, tf, look_from, sampling_rate, batched, jitter, L.pose_or_none(look_at, up, fov),
                        (look_from, look_at, up, fov), ctx.needs_input_grad[3:7])

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        dv, dt, camera = _backward(ctx, grad_output, ctx.needs_input_grad[3:7])
        return (None, dv, dt, *camera, None, None, None)


class DepthRaycaster(L.RayModule):
    """Depth moments of the 1-D TF raycaster.

    volume_shape (D, H, W), output_shape (H, W) and tf_shape (R) as for Raycaster.
    forward(volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3)) -> ([BS,]3,H,W) = (M1, M2, A).
    camera_grad=True: look_from, look_at, up and fov may require grad and receive their gradients; the moments and the volume
    and TF gradients are the default module's."""

    def __init__(self, volume_shape, output_shape, tf_shape, sampling_rate=1.0, jitter=True, max_samples=512, fov=30.0,
                 near=0.1, far=100.0, camera_grad=False):
        self._check_built(volume_shape, output_shape, tf_shape, max_samples)
        super().__init__(tuple(int(v) for v in volume_shape), output_shape, sampling_rate, jitter, max_samples, fov, near, far)
        self.tf_shape = int(tf_shape)
        self.camera_grad = bool(camera_grad)

    def _batch(self, volume, tf, look_from, pose=None):
        """-> (batched, vol ([BS,] W, D, H) view, tf ([BS,] R, 4) view, look_from (views, 3), pose); un-batched inputs are shared
        by all views. pose = (look_at, up, fov): they join the batch rule and come back as rows per view; else None."""
        self._check_tf_inputs(volume, tf, look_from)
        batched, lf, pose = L.views(look_from, pose, (volume, 5), (tf, 3))
        return batched, L.field_view(volume), tf.transpose(-1, -2), lf, pose

    @staticmethod
    def _moments_image(out, batched):
        """([BS,]W,H,4) = (M1, M2, 0, A) -> ([BS,]3,H,W) = (M1, M2, A) in Raycaster's image orientation."""
        img = L.image(out)
        return torch.stack((img[..., 0, :, :], img[..., 1, :, :], img[..., 3, :, :]), dim=-3)

    def forward(self, volume, tf, look_from, look_at=None, up=None, fov=None):
        """volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3) -> ([BS,]3,H,W) = (M1, M2, A).
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera. All None: the fixed camera. The four camera
        tensors may require grad in a module built with camera_grad=True only."""
        pose = L.pose_or_none(look_at, up, fov)
        if self.camera_grad and L.wants_grad(look_from, look_at, up, fov):
            batched, vol, tf_in, lf, pose = self._batch(volume, tf, look_from, pose)
            res = DepthCameraFunction.apply(self, vol, tf_in, lf, *(pose or (None, None, None)), self.sampling_rate, batched,
                                            self.jitter)
            return self._moments_image(res, batched)
        hint = "construct DepthRaycaster(..., camera_grad=True) for camera gradients"
        L.refuse_pose_grad("DepthRaycaster", hint, look_from=look_from, look_at=look_at, up=up, fov=fov)
        batched, vol, tf_in, lf, pose = self._batch(volume, tf, look_from, pose)
        res = DepthRaycastFunction.apply(self, vol, tf_in, lf, self.sampling_rate, batched, self.jitter, pose)
        return self._moments_image(res, batched)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), TF ({self.tf_shape}), "
                f"Max Samples = {self.max_samples}, camera_grad = {self.camera_grad}")


class RayBundleDepthFunction(torch.autograd.Function):
    """Autograd boundary of the depth march over a bundle: `apply(rc, volume, tf, origins, dirs, sampling_rate, jitter)`, the
    shape of bundle.RayBundleFunction. volume (W,D,H), any strides; tf (R,4); origins, dirs (N,3), the directions of unit
    length. Returns (N,4) = (M1, M2, 0, A). origins and dirs receive gradients where they require them
    (RayBundleDepthRaycaster refuses that unless built with ray_grad=True)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf, origins, dirs, sampling_rate, jitter=True):
        volume = F.as_volume(volume)
        tf = tf.float().contiguous()
        origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
        seed = F.new_jitter_seed() if jitter else 0
        e, x, n = F.bundle_setup(origins, dirs, volume.shape[-3:], sampling_rate, rc.t_near, seed)
        out, steps = F.march_depth_bundle_fwd(volume, tf, origins, dirs, e, x, n, rc.max_samples, sampling_rate)
        ctx.save_for_backward(volume, tf, origins, dirs, e, x, n, steps, out)
        ctx.rc, ctx.sampling_rate, ctx.seed = rc, sampling_rate, seed
        rc._steps = steps
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, tf, origins, dirs, e, x, n, steps, out = ctx.saved_tensors
        rc, sr = ctx.rc, ctx.sampling_rate
        dv, dt = F.march_depth_bundle_bwd(volume, tf, origins, dirs, e, x, n, rc.max_samples, sr, grad_output, out,
                                          want_vol=ctx.needs_input_grad[1], want_tf=ctx.needs_input_grad[2])
        d_o = d_d = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            d_o, d_d = F.march_depth_bundle_bwd_rays(volume, tf, origins, dirs, e, x, n, steps, rc.max_samples, sr, grad_output,
                                                     out, rc.t_near, ctx.seed)
        return (None, L.sanitised(dv), L.sanitised(dt), d_o if ctx.needs_input_grad[3] else None,
                d_d if ctx.needs_input_grad[4] else None, None, None)


class RayBundleDepthRaycaster(RayBundleRaycaster):
    """Depth moments of the 1-D TF raycaster over a bundle of rays.

    volume_shape (D, H, W) and tf_shape (R) as for Raycaster; the constructor, the argument checks and the AMP casting are
    bundle.RayBundleRaycaster's.
    forward(volume (1,D,H,W), tf (4,R), origins (...,3), directions (...,3)) -> (...,3) = (M1, M2, A), channel last: the
    opacity-weighted sums of each sample's distance from ITS RAY'S ORIGIN along the unit direction, of its square, and of 1. A
    is RayBundleRaycaster's alpha for the same inputs. One volume and one table per call.
    t_near: with None the reference's line through the box is marched, and an origin INSIDE the box then collects NEGATIVE
    distances from what lies behind it (so a pinhole camera's rays give DepthRaycaster's moments); t_near=0.0 makes every ray
    start at its origin and M1 / A a range.
    ray_grad=True: origins and directions may require grad and receive their gradients."""

    def forward(self, volume, tf, origins, directions):
        """volume (1,D,H,W), tf (4,R), origins, directions (...,3) -> (...,3) = (M1, M2, A). The directions are normalised
        here, in torch (a zero-length one raises), so their gradient is that of the direction handed in."""
        self._check(volume, tf, origins, directions)
        if not self.ray_grad:
            L.refuse_pose_grad("RayBundleDepthRaycaster",
                               "construct RayBundleDepthRaycaster(..., ray_grad=True) for ray gradients", origins=origins,
                               directions=directions)
        length = torch.sqrt((directions * directions).sum(-1, keepdim=True))
        if bool((length == 0).any()):
            raise ValueError("a direction has zero length")
        self._check_devices(volume, tf, origins, directions)
        dirs = (directions / length).reshape(-1, 3)
        out = RayBundleDepthFunction.apply(self, L.field_view(volume), tf.transpose(-1, -2), origins.reshape(-1, 3), dirs,
                                           self.sampling_rate, self.jitter)
        steps = self._steps
        self._steps = None if steps is None else steps.reshape(origins.shape[:-1])
        return out[:, (0, 1, 3)].reshape(*origins.shape[:-1], 3)
