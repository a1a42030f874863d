"""The layout convention every renderer module shares (internal).

A user volume ([BS,]C,D,H,W) is marched in the reference's field order (VX, VY, VZ) = (W, D, H) (VR.py:481), as a strided view
and never a copy; an image leaves the kernels as ([BS,]W,H,K) and the user as ([BS,]K,H,W) with H flipped (VR.py:513,523);
batched inputs agree on BS and un-batched ones are shared by all views. The renderer modules differ in which inputs they take and
what they check about them, not in any of this -- nor in what their autograd functions do around the family's own march: ray
setup, what is saved for the backward, and the camera gradients back in the shapes of the camera tensors (march_forward,
saved_rays, camera_grads).
"""
import contextlib
import math

import torch

from . import _native as N
from . import functional as F


def field_view(volume):
    """Scalar volume ([BS,]1,D,H,W) -> its ([BS,]W,D,H) view."""
    return volume.squeeze(1).permute(0, 3, 1, 2) if volume.ndim == 5 else volume.squeeze(0).permute(2, 0, 1)


def field_view_rgba(volume):
    """RGBA volume ([BS,]4,D,H,W) -> its ([BS,]4,W,D,H) view: whatever axis order the volume has in memory (rgba.interleaved)
    reaches the kernels as strides."""
    return volume.permute(0, 1, 4, 2, 3) if volume.ndim == 5 else volume.permute(0, 3, 1, 2)


def batch_rule(look_from, *inputs):
    """inputs: (tensor, its rank when batched) of everything beside look_from ([BS,]3). -> (batched, BS, look_from (BS,3)):
    BS is the leading size the batched inputs agree on (ValueError otherwise), 0 and look_from (1,3) when none is batched;
    an un-batched look_from is expanded to the batch, not copied."""
    sizes = {t.shape[0] for t, rank in (*inputs, (look_from, 2)) if t.ndim == rank}
    if not sizes:
        return False, 0, look_from.reshape(1, 3)
    if len(sizes) != 1:
        raise ValueError(f"batched inputs disagree on the batch size: {sorted(sizes)}")
    bs = sizes.pop()
    return True, bs, look_from if look_from.ndim == 2 else look_from.reshape(1, 3).expand(bs, 3)


def pose_rule(look_from, pose, *inputs):
    """batch_rule for the free camera: pose = (look_at, up, fov) -- look_at and up ([BS,]3), fov ([BS,]) degrees,
    a 0-d tensor or a number, each may be None -- joins the rule: a batched one sets BS like any other input, an un-batched one
    is shared by all views. -> (batched, BS, look_from (BS,3), (look_at, up (BS,3), fov (BS,))): the pose as tensors on
    look_from's device with one row per view (expanded, not copied), None staying None."""
    look_at, up, fov = pose
    if fov is not None and not torch.is_tensor(fov):
        fov = torch.tensor(float(fov), dtype=torch.float32, device=look_from.device)
    for name, t, ranks, last in (("look_at", look_at, (1, 2), 3), ("up", up, (1, 2), 3), ("fov", fov, (0, 1), None)):
        if t is not None and (t.ndim not in ranks or (last is not None and t.shape[-1] != last)):
            raise ValueError(f"expected {name} ([BS,]{last or ''}), got {tuple(t.shape)}")
    posed = [(t, rank) for t, rank in ((look_at, 2), (up, 2), (fov, 1)) if t is not None]
    batched, bs, lf = batch_rule(look_from, *inputs, *posed)
    views = bs if batched else 1
    rows = lambda t, k: None if t is None else t.to(look_from.device).reshape(-1, *k).expand(views, *k)
    return batched, bs, lf, (rows(look_at, (3,)), rows(up, (3,)), rows(fov, ()))


def has_pose(look_at, up, fov):
    """False when all are None: the renderers then take the fixed camera's code path, untouched."""
    return not (look_at is None and up is None and fov is None)


def pose_or_none(look_at, up, fov):
    """(look_at, up, fov) for pose_rule, None for the fixed camera (has_pose)."""
    return (look_at, up, fov) if has_pose(look_at, up, fov) else None


def views(look_from, pose, *inputs):
    """batch_rule, or pose_rule when pose = (look_at, up, fov) is not None, at one length -> (batched, look_from rows, the pose as
    rows per view or None)."""
    if pose is None:
        batched, _, lf = batch_rule(look_from, *inputs)
        return batched, lf, None
    batched, _, lf, pose = pose_rule(look_from, pose, *inputs)
    return batched, lf, pose


def check_inputs(expected, *inputs):
    """The rank and one fixed size of every input of a module's forward. inputs: (tensor, its rank when batched, the axis -- from
    the end -- that holds `size`, size); expected: the ValueError's wording of all of them."""
    for t, rank, _, _ in inputs:
        if t.ndim != rank and t.ndim != rank - 1:
            raise ValueError(f"expected {expected}")
    for t, _, axis, size in inputs:
        if t.shape[axis] != size:
            raise ValueError(f"expected {expected}; got " + ", ".join(str(tuple(t.shape)) for t, *_ in inputs))


def wants_grad(*tensors):
    """Whether autograd is on and one of the tensors (None and numbers allowed) requires grad."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def refuse_pose_grad(who, hint="use volume_raycaster.Raycaster for camera gradients", **tensors):
    """Raycaster2D, and RaycasterRGBA unless built with camera_grad=True, have no camera gradients: a camera tensor that requires
    grad is an error, not a silent None. hint: what the caller can do instead, beside detaching the tensor."""
    for name, t in tensors.items():
        if t is not None and wants_grad(t):   # (the fixed camera hands in three Nones: no call for those)
            raise ValueError(f"{who} has no gradient w.r.t. {name}: {hint}, or pass {name}.detach()")


def reduce_to(d, shape, dtype):
    """A per-view gradient (views, ...) back in the shape its input came in: an un-batched input that was shared by the views
    gets their sum."""
    if d.numel() != math.prod(shape):
        d = d.sum(0)
    return d.reshape(shape).to(dtype)


def sanitised(t):
    """None, or the gradient t after nan_to_num: the plain kernels propagate NaN like the reference, whose backward ends in
    nan_to_num (VR.py:463-464,474-475)."""
    return None if t is None else torch.nan_to_num(t)


def image(out):
    """Kernel image ([BS,]W,H,K) -> user image ([BS,]K,H,W), H flipped, contiguous (VR.py:513,523). A projection's
    ([BS,]W,H) is K = 1: image(out.unsqueeze(-1))."""
    return torch.flip(out, (-2,)).transpose(-1, -3).contiguous()


def unbatch(t, batched):
    """The (views, ...) result of the functional calls as the caller's ([BS,] ...)."""
    return t if batched else t[0]


def pose_tensors(cam, pose):
    """pose_rule's (look_at, up, fov) for the cameras cam (views,3) -> what the kernels read: the pose (views,9)
    float32 and fov_v (views,) float32 in RADIANS, None when fov is (the module's scalar fov serves every view)."""
    look_at, up, fov = pose
    fov_v = None if fov is None else torch.deg2rad(fov.to(cam.device, torch.float32).reshape(-1).expand(cam.shape[0])).contiguous()
    return F.pack_pose(cam, look_at, up), fov_v


def diff_rays(volume, look_from, jitter, output_shape, sampling_rate, fov, near, pose=None):
    """What the autograd forwards do before their march -> (volume, cam, seed, (entry, exit, rays, n), pose9, fov_v): the volume as
    the kernels read it, the cameras (views,3), the jitter seed drawn for this forward (0: none), the ray buffers of ray_setup, and
    None, None. pose: pose_rule's (look_at, up, fov) -- the buffers are ray_setup_pose's then, cam is the pose's float32 look_from
    rows, and pose9, fov_v are the pose (views,9) and the per-view fov (pose_tensors)."""
    cam = look_from.reshape(-1, 3)
    volume = F.as_volume(volume)
    seed = F.new_jitter_seed() if jitter else 0
    if pose is None:
        return volume, cam, seed, F.ray_setup(cam, output_shape, volume.shape[-3:], sampling_rate, fov, near, seed), None, None
    pose9, fov_v = pose_tensors(cam, pose)
    rays = F.ray_setup_pose(pose9, output_shape, volume.shape[-3:], sampling_rate, fov, near, seed, fov_v=fov_v)
    return volume, pose9[:, :3], seed, rays, pose9, fov_v


@contextlib.contextmanager
def nondiff_rays(volume, look_from, sampling_rate, module_rate, output_shape, fov, near, pose=None):
    """The scope and preamble of every raycast_nondiff (VR.py:490-523): no autograd, no autocast, the default rate of 4x the
    module's, never jittered. Yields (sampling_rate, volume, cam, (entry, exit, rays, n)) for the march inside the scope --
    and, with pose = pose_rule's (look_at, up, fov), the pose (views,9) and fov_v as two more (diff_rays): Raycaster's march
    reads them; RayModule._raycast_nondiff does not."""
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        sr = sampling_rate if sampling_rate is not None else 4.0 * module_rate
        volume = F.as_volume(volume)
        cam = look_from.reshape(-1, 3).float()
        if pose is None:
            yield sr, volume, cam, F.ray_setup(cam, output_shape, volume.shape[-3:], sr, fov, near, 0)
        else:
            pose9, fov_v = pose_tensors(cam, pose)
            rays = F.ray_setup_pose(pose9, output_shape, volume.shape[-3:], sr, fov, near, 0, fov_v=fov_v)
            yield sr, volume, pose9[:, :3], rays, pose9, fov_v


_RAD_PER_DEG = math.pi / 180.0


def camera_shapes(*tensors):
    """(shape, dtype) of each camera tensor as the caller handed it in (None for None): what its gradient goes back as."""
    return [None if t is None else (t.shape, t.dtype) for t in tensors]


def pose_grads(d_pose, shapes, needs):
    """d_pose (views, 10) of the kernels -> the gradients of look_from, look_at, up and fov in the shapes they came in (an
    un-batched one gets the sum over the views); fov.grad is per degree."""
    cols = (d_pose[:, 0:3], d_pose[:, 3:6], d_pose[:, 6:9], d_pose[:, 9] * _RAD_PER_DEG)
    return [reduce_to(c, *sh) if need and sh is not None else None for c, sh, need in zip(cols, shapes, needs)]


def march_forward(ctx, rc, march, volume, tensors, look_from, sampling_rate, batched, jitter, pose, camera=None, needs=()):
    """The forward of the march families' autograd functions: ray setup, `march(volume, cam, rays) -> (out, steps)`, rc._steps, and
    the image as the caller's ([BS,]W,H,4). Saved for the backward (saved_rays): the volume, the family's prepared `tensors`, the
    ray buffers, out and cam (views,3). camera: look_from, look_at, up, fov as the caller handed them in when the function
    returns their gradients, `needs` says which are wanted: the pose (views,9) is then saved in cam's place, whose first columns
    cam is, fov_v where there is one, and `steps` when any gradient is wanted."""
    volume, cam, seed, rays, pose9, fov_v = diff_rays(volume, look_from, jitter, rc.output_shape, sampling_rate, rc.fov, rc.near,
                                                      pose)
    out, steps = march(volume, cam, rays)
    if camera is None:
        pose9 = fov_v = None
    kept = steps if any(needs) else None
    ctx.save_for_backward(volume, *tensors, *rays, out,
                          *[t for t in (cam if pose9 is None else None, kept, pose9, fov_v) if t is not None])
    ctx.has_steps, ctx.has_pose, ctx.has_fov = kept is not None, pose9 is not None, fov_v is not None
    ctx.shapes, ctx.seed = camera_shapes(*(camera or ())), seed
    ctx.rc, ctx.sampling_rate, ctx.batched = rc, sampling_rate, batched
    rc._steps = unbatch(steps, batched)
    return unbatch(out, batched)


def saved_rays(ctx):
    """march_forward's tensors back -> ([volume, the family's tensors ..., entry, exit, rays, n, out], cam, steps, pose9, fov_v),
    None for what was not saved."""
    saved = list(ctx.saved_tensors)
    fov_v = saved.pop() if ctx.has_fov else None
    pose9 = saved.pop() if ctx.has_pose else None
    steps = saved.pop() if ctx.has_steps else None
    return saved, (pose9[:, :3] if ctx.has_pose else saved.pop()), steps, pose9, fov_v


def camera_grads(ctx, needs, bwd_cam, bwd_pose):
    """The gradients of look_from, look_at, up and fov (`needs`: which of them) from the family's camera backwards, called with
    fov_deg, near and the forward's jitter_seed: bwd_pose -> d_pose (views,10) when the forward had a pose, else bwd_cam ->
    d look_from (views,3), the only camera tensor there is then. Nothing is called when nothing is needed."""
    if not any(needs):
        return [None] * 4
    opts = dict(fov_deg=ctx.rc.fov, near=ctx.rc.near, jitter_seed=ctx.seed)
    if ctx.has_pose:
        return pose_grads(bwd_pose(**opts), ctx.shapes, needs)
    return [reduce_to(bwd_cam(**opts), *ctx.shapes[0]), None, None, None]


class RayModule(torch.nn.Module):
    """What Raycaster2D, RaycasterLit, RaycasterRGBA, DepthRaycaster and Projector keep alike: the volume shape in field order, the
    image shape, the sampling options and the camera. (Raycaster keeps the reference's attributes and its VolumeRaycaster
    instead.) A module's _batch(inputs..., look_from, pose) checks its inputs and returns (batched, the inputs' views ..., look_from
    rows, the pose as rows per view or None)."""

    def __init__(self, volume_shape, output_shape, sampling_rate, jitter, max_samples, fov, near, far):
        super().__init__()
        self.volume_shape = (volume_shape[2], volume_shape[0], volume_shape[1])  # (W, D, H), as Raycaster
        self.output_shape = tuple(output_shape)
        self.sampling_rate = sampling_rate
        self.jitter = jitter
        self.max_samples = max_samples
        self.fov, self.near, self.far = fov, near, far
        self._steps = None
        N.lib()  # fail loudly at construction time if the HIP library is missing

    @staticmethod
    def _check_built(volume_shape, output_shape, tf_shape=None, max_samples=None):
        """What the constructors check alike, in their order; tf_shape: a 1-D table's R; None: the module has no such option."""
        if len(tuple(volume_shape)) != 3 or len(tuple(output_shape)) != 2:
            raise ValueError("expected volume_shape (D, H, W) and output_shape (H, W)")
        if tf_shape is not None and int(tf_shape) < 1:
            raise ValueError(f"tf_shape must be the TF resolution R >= 1, got {tf_shape}")
        if max_samples is not None and int(max_samples) < 1:
            raise ValueError(f"max_samples must be >= 1, got {max_samples}")

    def _check_built_for(self, volume):
        """The (D, H, W) of a user volume ([BS,]C,D,H,W) against the shape the module was built for."""
        w, d, h = self.volume_shape
        if tuple(volume.shape[-3:]) != (d, h, w):
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {(d, h, w)}")

    def _check_tf_inputs(self, volume, tf, look_from):
        """The inputs of a module with a 1-D table of self.tf_shape entries."""
        check_inputs("volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3)", (volume, 5, -4, 1), (tf, 3, -2, 4),
                     (look_from, 2, -1, 3))
        self._check_built_for(volume)
        if tf.shape[-1] != self.tf_shape:
            raise ValueError(f"tf has R = {tf.shape[-1]}, the module was built for {self.tf_shape}")

    def _determine_batch(self, *inputs, **pose):
        """The module's _batch(inputs ..., look_from[, lighting], pose=None), same parameters, at the length callers outside the
        module hold: (batched, the inputs' views ..., look_from rows), and with pose = (look_at, up, fov) that pose as rows per
        view behind them."""
        res = self._batch(*inputs, **pose)
        return res if res[-1] is not None else res[:-1]

    def _raycast_nondiff(self, vol, look_from, sampling_rate, pose, batched, march):
        """The body of every raycast_nondiff: nondiff_rays' scope, `march(vol, cam, rays, sampling_rate) -> (out, steps)` inside
        it, self._steps and the image."""
        with nondiff_rays(vol, look_from, sampling_rate, self.sampling_rate, self.output_shape, self.fov, self.near,
                          pose) as (sr, vol, cam, rays, *_):
            out, steps = march(vol, cam, rays, sr)
            self._steps = unbatch(steps, batched)
            return image(unbatch(out, batched))

    @staticmethod
    def _image(out, batched):
        """([BS,]W,H,4) -> ([BS,]4,H,W); `batched` restates out's rank."""
        return image(out)
