"""The layout convention every renderer module shares (internal).

A user volume ([BS,]C,D,H,W) is marched in the reference's field order (VX, VY, VZ) = (W, D, H) (VR.py:481), as a strided view
and never a copy; an image leaves the kernels as ([BS,]W,H,K) and the user as ([BS,]K,H,W) with H flipped (VR.py:513,523);
batched inputs agree on BS and un-batched ones are shared by all views. Raycaster, Raycaster2D, Projector and RaycasterRGBA
differ in which inputs they take and what they check about them, not in any of this.
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


def wants_grad(*tensors):
    """Whether autograd is on and one of the tensors (None and numbers allowed) requires grad."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def refuse_pose_grad(who, hint="use volume_raycaster.Raycaster for camera gradients", **tensors):
    """Raycaster2D, and RaycasterRGBA unless built with camera_grad=True, have no camera gradients: a camera tensor that requires
    grad is an error, not a silent None. hint: what the caller can do instead, beside detaching the tensor."""
    for name, t in tensors.items():
        if wants_grad(t):
            raise ValueError(f"{who} has no gradient w.r.t. {name}: {hint}, or pass {name}.detach()")


def reduce_to(d, shape, dtype):
    """A per-view gradient (views, ...) back in the shape its input came in: an un-batched input that was shared by the views
    gets their sum."""
    if d.numel() != math.prod(shape):
        d = d.sum(0)
    return d.reshape(shape).to(dtype)


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
    """What the autograd forwards do before their march -> (volume, cam, seed, (entry, exit, rays, n)): the volume as the kernels
    read it, the cameras (views,3), the jitter seed drawn for this forward (0: none) and the ray buffers of ray_setup.
    pose: pose_rule's (look_at, up, fov) -- the buffers are ray_setup_pose's then, cam is the pose's float32 look_from rows, and
    the result has two more entries: the pose (views,9) and fov_v (pose_tensors)."""
    cam = look_from.reshape(-1, 3)
    volume = F.as_volume(volume)
    seed = F.new_jitter_seed() if jitter else 0
    if pose is None:
        return volume, cam, seed, F.ray_setup(cam, output_shape, volume.shape[-3:], sampling_rate, fov, near, seed)
    pose9, fov_v = pose_tensors(cam, pose)
    rays = F.ray_setup_pose(pose9, output_shape, volume.shape[-3:], sampling_rate, fov, near, seed, fov_v=fov_v)
    return volume, pose9[:, :3], seed, rays, pose9, fov_v


@contextlib.contextmanager
def nondiff_rays(volume, look_from, sampling_rate, module_rate, output_shape, fov, near, pose=None):
    """The scope and preamble of every raycast_nondiff (VR.py:490-523): no autograd, no autocast, the default rate of 4x the
    module's, never jittered. Yields (sampling_rate, volume, cam, (entry, exit, rays, n)) for the march inside the scope --
    and, with pose = pose_rule's (look_at, up, fov), the pose (views,9) and fov_v as two more (diff_rays)."""
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


class RayModule(torch.nn.Module):
    """What Raycaster2D, Projector and RaycasterRGBA keep alike: the volume shape in field order, the image shape, the sampling
    options and the camera. (Raycaster keeps the reference's attributes and its VolumeRaycaster instead.)"""

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

    def _check_built_for(self, volume):
        """The (D, H, W) of a user volume ([BS,]C,D,H,W) against the shape the module was built for."""
        w, d, h = self.volume_shape
        if tuple(volume.shape[-3:]) != (d, h, w):
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {(d, h, w)}")

    def _nondiff_rays(self, volume, look_from, sampling_rate, pose=None):
        return nondiff_rays(volume, look_from, sampling_rate, self.sampling_rate, self.output_shape, self.fov, self.near, pose)

    @staticmethod
    def _image(out, batched):
        """([BS,]W,H,4) -> ([BS,]4,H,W); `batched` restates out's rank."""
        return image(out)
