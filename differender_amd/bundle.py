"""Differentiable rendering of arbitrary ray bundles with the 1-D TF raycaster.

Every other renderer draws its rays from one pinhole camera per view, over a whole image. Here a ray is an input:

    rc = RayBundleRaycaster(volume.shape[-3:], R, ray_grad=True)
    rgba = rc(volume, tf, origins, directions)          # (..., 3), (..., 3) -> (..., 4)

origins and directions share any leading shape and live in look_from's world coordinates (the volume fills [-1, 1]^3). Each ray
is marched as Raycaster marches a pixel's -- same samples, classification, shading and compositing, the light at origin +
(0, 1, 0) -- so the rays of a pinhole camera give that camera's image, and a random minibatch of rays drawn across many views, a
parallel-beam geometry or a distorted lens is a few lines of torch in front of this one module:

    o, d = pinhole_rays(look_from, look_at, up, fov, (H, W))             # Raycaster's own rays, (H, W, 3) each
    o, d = orthographic_rays(look_from, look_at, up, extent, (H, W))     # parallel rays from a plane through look_from
    o, d = cone_beam_rays(source, det_center, det_u, det_v, (H, W))      # a point source and a flat detector

The rays of an image are fastest in tiles, not rows (a wave is 64 consecutive rays): `perm = tile_order((H, W))`, march
`o.reshape(-1, 3)[perm]`, and put the result back with `out[perm] = result`. projection.RayBundleProjector takes
the same bundles for X-ray and maximum intensity projections.

Gradients flow to the volume and the TF; a module built with ray_grad=True gives origins and directions theirs as well, and
autograd carries them on into whatever made the rays (both helpers are plain differentiable torch).
"""
import math

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["RayBundleRaycaster", "RayBundleFunction", "pinhole_rays", "orthographic_rays", "cone_beam_rays", "tile_order"]


def _unit(a):
    return a / torch.sqrt((a * a).sum(-1, keepdim=True))


def _camera_basis(look_from, look_at, up):
    """The free camera's basis: view_dir, right, up'."""
    look_at = torch.as_tensor(look_at, dtype=look_from.dtype, device=look_from.device)
    up = torch.as_tensor(up, dtype=look_from.dtype, device=look_from.device)
    view_dir = _unit(look_at - look_from)
    right = _unit(torch.linalg.cross(view_dir, up))
    return view_dir, right, _unit(torch.linalg.cross(right, view_dir))


def _pixel_grid(output_shape, like):
    """The near-plane coordinates (u, v) of every pixel in the user image's orientation -> two (H, W, 1) tensors and (W, H).
    output_shape is what Raycaster takes: its first entry counts the pixels along `right`, the image's last axis W; its second
    those along up', the image's axis H, which runs downwards (the image is flipped, VR.py:513)."""
    W, H = int(output_shape[0]), int(output_shape[1])
    i = torch.arange(W, dtype=like.dtype, device=like.device)
    j = torch.arange(H - 1, -1, -1, dtype=like.dtype, device=like.device)
    u = ((i + 0.5) / W - 0.5)[None, :, None].expand(H, W, 1)
    v = ((j + 0.5) / H - 0.5)[:, None, None].expand(H, W, 1)
    return u, v, W, H


def pinhole_rays(look_from, look_at, up, fov, output_shape, near=0.1):
    """The rays of the free camera -> origins, directions (H, W, 3) in the user image's orientation, as
    differentiable torch functions of look_from, look_at, up (3,) and fov (degrees; a number or a 0-d tensor):
    `rc(vol, tf, *pinhole_rays(...)).permute(2, 0, 1)` is Raycaster's image for that camera and output_shape up to the float
    rounding of the directions. (The extent of the near plane is 2 near tan(fov), as everywhere in the reference.)"""
    view_dir, right, upp = _camera_basis(look_from, look_at, up)
    u, v, W, H = _pixel_grid(output_shape, look_from)
    fov_rad = torch.as_tensor(fov, dtype=look_from.dtype, device=look_from.device) * (math.pi / 180.0)
    near_h = 2.0 * torch.tan(fov_rad) * near
    near_w = near_h * (W / H)
    near_pos = (look_from + near * view_dir) + (u * near_w) * right + (v * near_h) * upp
    return look_from.expand(H, W, 3), _unit(near_pos - look_from)


def orthographic_rays(look_from, look_at, up, extent, output_shape):
    """Parallel rays along look_at - look_from from the plane through look_from that is `extent` world units high (and
    extent W / H wide) -> origins, directions (H, W, 3) in the user image's orientation; differentiable torch, like
    pinhole_rays. Pixel centres are extent / H apart."""
    view_dir, right, upp = _camera_basis(look_from, look_at, up)
    u, v, W, H = _pixel_grid(output_shape, look_from)
    ext_h = torch.as_tensor(extent, dtype=look_from.dtype, device=look_from.device)
    origins = look_from + (u * (ext_h * (W / H))) * right + (v * ext_h) * upp
    return origins, view_dir.expand(H, W, 3)


def cone_beam_rays(source, det_center, det_u, det_v, det_shape):
    """The rays of a cone beam: a point source and a flat detector of det_shape = (H, W) pixels whose pixel (r, c) sits at
    det_center + (c - (W-1)/2) det_u + (r - (H-1)/2) det_v -- det_u, det_v (3,) the steps to the next column and row, any pitch,
    any offset of det_center from the source's axis -> origins (the source), directions (unit vectors to the pixels), (H, W, 3)
    each; differentiable torch in all four, like pinhole_rays."""
    H, W = int(det_shape[0]), int(det_shape[1])
    like = dict(dtype=source.dtype, device=source.device)
    det_center, det_u, det_v = (torch.as_tensor(a, **like) for a in (det_center, det_u, det_v))
    c = (torch.arange(W, **like) - (W - 1) / 2)[None, :, None]
    r = (torch.arange(H, **like) - (H - 1) / 2)[:, None, None]
    pixels = det_center + c * det_u + r * det_v
    return source.expand(H, W, 3), _unit(pixels - source)


def tile_order(shape, tile=16):
    """A permutation (int64, H*W) of the flattened (H, W) grid sorted by tile x tile tile, then by (tile/2) x (tile/2) sub-tile
    within it, then row-major within the sub-tile: where H and W are multiples of 16, each run of 256 is one 16 x 16 tile (a
    group of the bundle projections' windowed backward) and each run of 64 one 8 x 8 block (a wave of every bundle kernel).
    Edge tiles are cut at the grid's border."""
    H, W, tile = int(shape[0]), int(shape[1]), int(tile)
    if H < 1 or W < 1 or tile < 2 or tile % 2:
        raise ValueError(f"tile_order needs a grid of >= 1 x 1 and an even tile >= 2, got {(H, W)}, {tile}")
    half = tile // 2
    r = torch.arange(H)[:, None].expand(H, W).reshape(-1)
    c = torch.arange(W)[None, :].expand(H, W).reshape(-1)
    tiles_w, in_r, in_c = (W + tile - 1) // tile, r % tile, c % tile
    key = (r // tile) * tiles_w + c // tile                      # the tile
    key = key * 4 + (in_r // half) * 2 + in_c // half            # its sub-tile
    key = key * (half * half) + (in_r % half) * half + in_c % half
    return torch.argsort(key, stable=True)


class RayBundleFunction(torch.autograd.Function):
    """Autograd boundary of the bundle march: `apply(rc, volume, tf, origins, dirs, sampling_rate, jitter)`. volume (W,D,H),
    any strides; tf (R,4); origins, dirs (N,3), the directions of unit length. Returns (N,4). origins and dirs receive gradients
    where they require them (RayBundleRaycaster refuses that unless built with ray_grad=True)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf, origins, dirs, sampling_rate, jitter=True):
        volume = F.as_volume(volume)
        tf = tf.float().contiguous()
        origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
        seed = F.new_jitter_seed() if jitter else 0
        e, x, n = F.bundle_setup(origins, dirs, volume.shape[-3:], sampling_rate, rc.t_near, seed)
        out, steps = F.march_bundle_fwd(volume, tf, origins, dirs, e, x, n, rc.max_samples, sampling_rate)
        ctx.save_for_backward(volume, tf, origins, dirs, e, x, n, steps, out)
        ctx.rc, ctx.sampling_rate, ctx.seed = rc, sampling_rate, seed
        rc._steps = steps
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, tf, origins, dirs, e, x, n, steps, out = ctx.saved_tensors
        rc, sr = ctx.rc, ctx.sampling_rate
        dv, dt = F.march_bundle_bwd(volume, tf, origins, dirs, e, x, n, rc.max_samples, sr, grad_output, out,
                                    want_vol=ctx.needs_input_grad[1], want_tf=ctx.needs_input_grad[2])
        d_o = d_d = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            d_o, d_d = F.march_bundle_bwd_rays(volume, tf, origins, dirs, e, x, n, steps, rc.max_samples, sr, grad_output, out,
                                               rc.t_near, ctx.seed)
        return (None, L.sanitised(dv), L.sanitised(dt), d_o if ctx.needs_input_grad[3] else None,
                d_d if ctx.needs_input_grad[4] else None, None, None)


class RayBundleRaycaster(torch.nn.Module):
    """The 1-D TF raycaster over a bundle of rays.

    volume_shape (D, H, W) and tf_shape (R) as for Raycaster.
    forward(volume (1,D,H,W), tf (4,R), origins (...,3), directions (...,3)) -> (...,4) RGBA; one volume and one table per call.
    t_near: None marches the reference's line through the box, which also shows what lies behind an origin inside it (so a
    pinhole camera's rays give Raycaster's image); 0.0 makes every ray start at its origin.
    ray_grad=True: origins and directions may require grad and receive their gradients."""

    def __init__(self, volume_shape, tf_shape, sampling_rate=1.0, jitter=True, max_samples=512, t_near=None, ray_grad=False):
        super().__init__()
        if len(tuple(volume_shape)) != 3:
            raise ValueError("expected volume_shape (D, H, W)")
        if int(tf_shape) < 1:
            raise ValueError(f"tf_shape must be the TF resolution R >= 1, got {tf_shape}")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples must be >= 1, got {max_samples}")
        if t_near is not None and math.isnan(float(t_near)):
            raise ValueError("t_near must be a number or None")
        self.volume_shape = (int(volume_shape[2]), int(volume_shape[0]), int(volume_shape[1]))  # (W, D, H), as Raycaster
        self.tf_shape = int(tf_shape)
        self.sampling_rate, self.jitter, self.max_samples = sampling_rate, jitter, int(max_samples)
        self.t_near = None if t_near is None else float(t_near)
        self.ray_grad = bool(ray_grad)
        self._steps = None
        N.lib()  # fail loudly at construction time if the HIP library is missing

    def _check(self, volume, tf, origins, directions):
        expected = "volume (1,D,H,W), tf (4,R), origins (...,3), directions (...,3) of one shape"
        if volume.ndim != 4 or volume.shape[0] != 1 or tf.ndim != 2 or tf.shape[0] != 4:
            raise ValueError(f"expected {expected}; got volume {tuple(volume.shape)}, tf {tuple(tf.shape)}")
        w, d, h = self.volume_shape
        if tuple(volume.shape[-3:]) != (d, h, w):
            raise ValueError(f"volume has (D, H, W) = {tuple(volume.shape[-3:])}, the module was built for {(d, h, w)}")
        if tf.shape[-1] != self.tf_shape:
            raise ValueError(f"tf has R = {tf.shape[-1]}, the module was built for {self.tf_shape}")
        if origins.ndim < 1 or origins.shape[-1] != 3 or origins.shape != directions.shape or origins.numel() == 0:
            raise ValueError(f"expected {expected}; got origins {tuple(origins.shape)}, directions {tuple(directions.shape)}")

    @staticmethod
    def _check_devices(volume, tf, origins, directions):
        for name, t in (("volume", volume), ("tf", tf), ("origins", origins), ("directions", directions)):
            F._require_gpu(t, name)
            if t.device != volume.device:
                raise ValueError(f"{name} lives on {t.device}, the volume on {volume.device}")

    def forward(self, volume, tf, origins, directions):
        """volume (1,D,H,W), tf (4,R), origins, directions (...,3) -> (...,4). The directions are normalised here, in torch (a
        zero-length one raises), so their gradient is that of the direction handed in."""
        self._check(volume, tf, origins, directions)
        if not self.ray_grad:
            L.refuse_pose_grad("RayBundleRaycaster", "construct RayBundleRaycaster(..., ray_grad=True) for ray gradients",
                               origins=origins, directions=directions)
        length = torch.sqrt((directions * directions).sum(-1, keepdim=True))
        if bool((length == 0).any()):
            raise ValueError("a direction has zero length")
        self._check_devices(volume, tf, origins, directions)
        dirs = (directions / length).reshape(-1, 3)
        out = RayBundleFunction.apply(self, L.field_view(volume), tf.transpose(-1, -2), origins.reshape(-1, 3), dirs,
                                      self.sampling_rate, self.jitter)
        steps = self._steps
        self._steps = None if steps is None else steps.reshape(origins.shape[:-1])
        return out.reshape(*origins.shape[:-1], 4)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), TF ({self.tf_shape}), Max Samples = {self.max_samples}, "
                f"t_near = {self.t_near}, ray_grad = {self.ray_grad}")
