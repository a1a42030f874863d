"""Differentiable 2-D (value, gradient-magnitude) transfer functions.

A 1-D transfer function classifies a sample by its value alone, so a material boundary cannot be told from the interior of a
material of the same value. A value x gradient-magnitude table (Levoy 1988, Kniss et al. 2002) can: its second axis is the
length of the central-difference gradient every sample already computes for its shading normal, scaled by `g_scale`
(u = |grad| * g_scale; u = 1 is the table's last column).

    rc = Raycaster2D(volume.shape[-3:], (H, W), (RV, RG), g_scale=gradient_scale(volume))
    img = rc(volume, tf2d, look_from)        # volume ([BS,]1,D,H,W), tf2d ([BS,]4,RV,RG), look_from ([BS,]3) -> ([BS,]4,H,W)

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster; a (4, RV, 1) table renders exactly what
Raycaster renders with the (4, RV) TF. Gradients flow to the volume and the table; the camera gradient is Raycaster's alone.
"""
import math

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["Raycaster2D", "Tf2dRaycastFunction", "gradient_scale"]

_DELTA = 1e-3   # the half-step of the shading normal's central differences, in the renderer's [-1, 1] coordinates


def gradient_scale(volume, q=0.99):
    """The g_scale that maps the q-quantile of the gradient magnitude to u = 1, for a volume ([BS,]1,D,H,W) or (D,H,W) (a batch:
    over the voxels of all its volumes, each differenced on its own).

    An ESTIMATE over voxel centres: the renderer takes its taps at trilinearly interpolated positions +-1e-3 around each sample,
    which span 1e-3 (N_axis - 1 - 1e-4) voxels along an axis of N_axis voxels; here each voxel's central difference (one-sided at
    the faces) |dv| per voxel is scaled by that span, and the magnitude's q-quantile over all voxels (of a strided subsample of at
    most 2^24 of them) is taken. Samples between voxel centres, and structures thinner than a voxel, can exceed it: their u
    lands in the table's last column."""
    v = volume.detach()
    if v.ndim not in (3, 4, 5) or (v.ndim > 3 and v.shape[-4] != 1):
        raise ValueError("volume must be ([BS,]1,D,H,W) or (D,H,W)")
    v = v.reshape(-1, *v.shape[-3:]).double()   # (volumes, D, H, W): no difference crosses from one volume into the next
    mag2 = torch.zeros_like(v)
    for axis in (1, 2, 3):
        n = v.shape[axis]
        if n < 2:
            continue
        d = torch.gradient(v, dim=axis)[0] * (2.0 * _DELTA * 0.5 * (n - 1 - 1e-4))
        mag2 += d * d
    mag = mag2.sqrt().flatten()
    if mag.numel() > (1 << 24):
        mag = mag[::-(-mag.numel() // (1 << 24))]
    g = float(torch.quantile(mag, float(q)))
    if not (g > 0.0 and math.isfinite(g)):
        raise ValueError("the volume's gradient magnitude quantile is zero or not finite: no g_scale maps it to u = 1")
    return 1.0 / g


class Tf2dRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the 2-D TF march: `apply(rc, volume, tf2d, look_from, sampling_rate, batched, jitter)`.
    volume (W,D,H) or (BS,W,D,H), any strides; tf2d (RV,RG,4) or (BS,RV,RG,4); look_from (BS,3). Returns (W,H,4) or
    (BS,W,H,4). d look_from is not defined here (Raycaster has it)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf2d, look_from, sampling_rate, batched, jitter=True, pose=None):
        tf2d = tf2d.float().contiguous()
        march = lambda volume, cam, rays: F.march_tf2d_fwd(volume, tf2d, cam, *rays, rc.max_samples, sampling_rate, rc.g_scale,
                                                           N.DR_MODE_DIFF)
        return L.march_forward(ctx, rc, march, volume, (tf2d,), look_from, sampling_rate, batched, jitter, pose)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        (volume, tf2d, e, x, r, n, out), cam, *_ = L.saved_rays(ctx)
        g = grad_output if ctx.batched else grad_output[None]
        dv, dt = F.march_tf2d_bwd(volume, tf2d, cam, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, ctx.rc.g_scale, g, out,
                                  want_vol=ctx.needs_input_grad[1], want_tf=ctx.needs_input_grad[2])
        return None, L.sanitised(dv), L.sanitised(dt), None, None, None, None, None


class Raycaster2D(L.RayModule):
    """Raycaster with a 2-D (value, gradient-magnitude) transfer function.

    volume_shape (D, H, W), output_shape (H, W) as for Raycaster, tf_shape (RV, RG), g_scale > 0 (gradient_scale() estimates one).
    forward(volume ([BS,]1,D,H,W), tf2d ([BS,]4,RV,RG), look_from ([BS,]3)) -> ([BS,]4,H,W)."""

    def __init__(self, volume_shape, output_shape, tf_shape, g_scale, sampling_rate=1.0, jitter=True, max_samples=512,
                 fov=30.0, near=0.1, far=100.0):
        if len(tuple(volume_shape)) != 3 or len(tuple(output_shape)) != 2 or len(tuple(tf_shape)) != 2:
            raise ValueError("expected volume_shape (D, H, W), output_shape (H, W) and tf_shape (RV, RG)")
        if min(tf_shape) < 1:
            raise ValueError(f"tf_shape must be (RV >= 1, RG >= 1), got {tuple(tf_shape)}")
        g = float(g_scale)
        if not (math.isfinite(g) and g > 0.0):
            raise ValueError(f"g_scale must be finite and > 0, got {g_scale}")
        super().__init__(volume_shape, output_shape, sampling_rate, jitter, max_samples, fov, near, far)
        self.tf_shape = tuple(int(v) for v in tf_shape)
        self.g_scale = g

    def _batch(self, volume, tf2d, look_from, pose=None):
        """-> (batched, vol ([BS,] W, D, H) view, tf2d ([BS,] RV, RG, 4) view, look_from (BS, 3), pose); un-batched inputs are
        shared by all views. pose = (look_at, up, fov): they join the batch rule and come back as rows per view; else None."""
        L.check_inputs("volume ([BS,]1,D,H,W), tf2d ([BS,]4,RV,RG), look_from ([BS,]3)", (volume, 5, -4, 1), (tf2d, 4, -3, 4),
                       (look_from, 2, -1, 3))
        if tuple(tf2d.shape[-2:]) != self.tf_shape:
            raise ValueError(f"tf2d has (RV, RG) = {tuple(tf2d.shape[-2:])}, the module was built for {self.tf_shape}")
        batched, lf, pose = L.views(look_from, pose, (volume, 5), (tf2d, 4))
        return batched, L.field_view(volume), tf2d.movedim(-3, -1), lf, pose

    def forward(self, volume, tf2d, look_from, look_at=None, up=None, fov=None):
        """volume ([BS,]1,D,H,W), tf2d ([BS,]4,RV,RG), look_from ([BS,]3) -> ([BS,]4,H,W).
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera for the image and the volume / table
        gradients; like look_from they may not require grad. All None: the fixed camera."""
        if torch.is_grad_enabled() and look_from.requires_grad:
            raise ValueError("Raycaster2D has no gradient w.r.t. look_from: use volume_raycaster.Raycaster (1-D transfer "
                             "function) for camera gradients, or pass look_from.detach()")
        L.refuse_pose_grad("Raycaster2D", look_at=look_at, up=up, fov=fov)
        batched, vol, tf, lf, pose = self._batch(volume, tf2d, look_from, L.pose_or_none(look_at, up, fov))
        res = Tf2dRaycastFunction.apply(self, vol, tf, lf, self.sampling_rate, batched, self.jitter, pose)
        return self._image(res, batched)

    def raycast_nondiff(self, volume, tf2d, look_from, sampling_rate=None, look_at=None, up=None, fov=None):
        """Non-differentiable render (never jittered); default rate 4x the module's, as Raycaster.raycast_nondiff."""
        batched, vol, tf, lf, pose = self._batch(volume, tf2d, look_from, L.pose_or_none(look_at, up, fov))
        march = lambda vol, cam, rays, sr: F.march_tf2d_fwd(vol, tf.float().contiguous(), cam, *rays, self.max_samples, sr,
                                                            self.g_scale, N.DR_MODE_NONDIFF)
        return self._raycast_nondiff(vol, lf, sampling_rate, pose, batched, march)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), TF2D ({self.tf_shape}), "
                f"g_scale = {self.g_scale:.6g}, Max Samples = {self.max_samples}")
