"""The free camera of Raycaster and Projector: look_at, up and a per-view fov beside look_from, with gradients.

The reference's camera looks at the origin with up = +y and one field of view (VR.py:127-151), and RaycastFunction keeps the
reference's signature; a pose goes through the autograd functions here instead. The renderers call them only when one of
look_at, up, fov is given -- with all three None their fixed-camera path runs untouched:

    rc = Raycaster(volume.shape[-3:], (H, W), R)
    img = rc(volume, tf, look_from, look_at=look_at, up=up, fov=fov)    # each ([BS,]3) / ([BS,]) degrees, or None
    loss(img).backward()                                                # look_from.grad, look_at.grad, up.grad, fov.grad (per degree)

A missing entry defaults to the origin, +y and the module's fov. An un-batched entry is shared by all views and receives the
sum of their gradients. The light stays at look_from + (0, 1, 0) in world space: it does not follow `up`. `up` parallel to the
viewing direction is degenerate (as the fixed camera on the y axis is), and a fov outside (0, 90) degrees is not checked: the
values live on the device, and checking them would synchronise.
"""
import torch

from . import _layout as L
from . import _native as N
from . import functional as F
from . import projection
from ._layout import camera_shapes as _shapes, pose_grads as _pose_grads

__all__ = ["PoseRaycastFunction", "PoseProjectFunction"]


class PoseRaycastFunction(torch.autograd.Function):
    """`apply(vr, volume, tf, look_from, look_at, up, fov, sampling_rate, batched, jitter, hints)`: RaycastFunction for the free
    camera. volume (W,D,H) or (BS,W,D,H), tf (R,4) or (BS,R,4); look_from, look_at, up ([BS,]3) and fov ([BS,]) degrees as
    _layout.pose_rule expanded them (views rows, or None). Returns (W,H,4) or (BS,W,H,4) and gradients for volume, tf
    and the four camera tensors."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, vr, volume, tf, look_from, look_at, up, fov, sampling_rate, batched, jitter=True, hints="auto"):
        is_batched, bs = batched
        cam = look_from.reshape(-1, 3)
        if is_batched and cam.shape[0] != bs:
            cam = cam.expand(bs, 3)
        tf = tf.float().contiguous()
        volume, cam, seed, rays, pose, fov_v = L.diff_rays(volume, cam, jitter, vr.resolution, sampling_rate, vr.fov_deg, vr.near,
                                                           pose=(look_at, up, fov))
        ws = F.alloc_workspace(cam.shape[0], vr.resolution, volume.shape[-3:], tf.shape[-2], volume.device)
        out, steps = F.march_fwd(volume, tf, cam, *rays, vr.max_samples, sampling_rate, N.DR_MODE_DIFF, fov_deg=vr.fov_deg,
                                 near=vr.near, workspace=ws, hints=hints, pose=pose, fov_v=fov_v)
        ctx.want_pose = any(ctx.needs_input_grad[3:7])
        ctx.save_for_backward(volume, tf, pose, *rays, out, *((steps,) if ctx.want_pose else ()),
                              *((fov_v,) if fov_v is not None else ()))
        ctx.has_fov = fov_v is not None
        ctx.shapes = _shapes(look_from, look_at, up, fov)
        ctx.workspace = ws
        ctx.vr, ctx.sampling_rate, ctx.batched, ctx.jitter_seed = vr, sampling_rate, is_batched, seed
        vr._steps = steps if is_batched else steps[0]
        vr._watch_workspace(ws, rays[3].numel(), forward=True)
        return out if is_batched else out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, tf, pose, e, x, r, n, out = ctx.saved_tensors[:8]
        fov_v = ctx.saved_tensors[-1] if ctx.has_fov else None
        vr = ctx.vr
        g = grad_output if ctx.batched else grad_output[None]
        want_vol, want_tf = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        cam = pose[:, :3]
        dv, dt = F.march_bwd(volume, tf, cam, e, x, r, n, vr.max_samples, ctx.sampling_rate, g, out, want_vol=want_vol,
                             want_tf=want_tf, fov_deg=vr.fov_deg, near=vr.near, workspace=ctx.workspace, pose=pose, fov_v=fov_v)
        vr._watch_workspace(ctx.workspace, n.numel())
        if not F.bwd_is_sanitised(volume, tf, dv, ctx.workspace, n):   # as RaycastFunction.backward
            dv = None if dv is None else torch.nan_to_num(dv)
            dt = None if dt is None else torch.nan_to_num(dt)
        grads = [None] * 4
        if ctx.want_pose:   # after march_bwd, on the same stream
            d_pose = F.march_bwd_pose(volume, tf, pose, e, x, r, n, ctx.saved_tensors[8], vr.max_samples, ctx.sampling_rate, g,
                                      out, fov_deg=vr.fov_deg, near=vr.near, jitter_seed=ctx.jitter_seed, fov_v=fov_v)
            grads = _pose_grads(d_pose, ctx.shapes, ctx.needs_input_grad[3:7])
        return (None, dv, dt, *grads, None, None, None, None)


class PoseProjectFunction(torch.autograd.Function):
    """`apply(pj, volume, look_from, look_at, up, fov, batched, jitter)`: projection.ProjectFunction for the free camera, with
    gradients for the volume and the four camera tensors."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pj, volume, look_from, look_at, up, fov, batched, jitter=True):
        return projection._forward(ctx, pj, volume, look_from, batched, jitter, (look_at, up, fov))

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, pose, e, x, r, n, *rest = ctx.saved_tensors
        arg = rest[0] if ctx.has_arg else None
        fov_v = rest[-1] if ctx.has_fov else None
        pj = ctx.pj
        g = grad_output if ctx.batched else grad_output[None]
        dv = None
        grads = [None] * 4
        if ctx.needs_input_grad[1]:
            dv = torch.nan_to_num(F.project_bwd(volume, pose[:, :3], e, x, r, n, g, pj.max_samples, pj.mode, arg))
        if any(ctx.needs_input_grad[2:6]):
            d_pose = F.project_bwd_pose(volume, pose, e, x, r, n, g, pj.max_samples, pj.mode, arg, fov_deg=pj.fov, near=pj.near,
                                        jitter_seed=ctx.seed, fov_v=fov_v)
            grads = _pose_grads(d_pose, ctx.shapes, ctx.needs_input_grad[2:6])
        return (None, dv, *grads, None, None)
