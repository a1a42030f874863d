"""A differentiable light and Phong material for the 1-D TF raycaster.

Raycaster shades with the reference's hard-wired lighting: a white light at look_from + (0, 1, 0), ambient 0.4, diffuse 0.8,
specular 0.3, shininess 32 (VR.py:91-95, 281-299). RaycasterLit renders the same program with these as arguments -- a light
position and colour, and the four material scalars -- and returns their gradients, so a light can be placed (a headlight, a
studio light), a target's look matched, or lighting fitted to images:

    rc = RaycasterLit(volume.shape[-3:], (H, W), R, headlight=False)
    img = rc(volume, tf, look_from, light_pos=p, light_color=c, ambient=ka, diffuse=kd, specular=ks, shininess=sh)

Batching, image orientation and AMP casting are those of volume_raycaster.Raycaster; with every lighting argument None the
image is Raycaster's plain-kernel image. Gradients flow to the volume, the TF and every lighting tensor that requires grad;
camera gradients are Raycaster's alone.
"""
import math

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["RaycasterLit", "LitRaycastFunction"]

# name -> (components, the reference's value); the order of the kernels' light[view][10] (light_pos is the headlight offset)
_LIGHTING = (("light_pos", 3, (0.0, 1.0, 0.0)), ("light_color", 3, (1.0, 1.0, 1.0)), ("ambient", 1, (0.4,)),
             ("diffuse", 1, (0.8,)), ("specular", 1, (0.3,)), ("shininess", 1, (32.0,)))


def _check_lighting(values):
    """The six lighting arguments as given -> [(name, k, value or None)], with every check that needs no device: a Python number
    (or a sequence of k numbers) is finite, the shininess > 0; a tensor is (), (k,) or (BS, k) -- a scalar parameter also (BS,)."""
    out = []
    for (name, k, _), v in zip(_LIGHTING, values):
        if v is None:
            out.append((name, k, None))
            continue
        if torch.is_tensor(v):
            ok = v.ndim == 0 or (v.ndim == 1 and (v.shape[0] == k or k == 1)) or (v.ndim == 2 and v.shape[1] == k)
            if not ok:
                raise ValueError(f"expected {name} as a number or a tensor of shape (), ({k},) or (BS, {k}), got {tuple(v.shape)}")
            if not v.is_floating_point():
                v = v.float()
            if k == 1 and v.ndim == 1 and v.shape[0] != 1:
                v = v[:, None]   # (BS,) -> (BS, 1)
            out.append((name, k, v))
            continue
        seq = [float(x) for x in v] if isinstance(v, (tuple, list)) else [float(v)]
        if len(seq) not in (1, k):
            raise ValueError(f"expected {name} as a number or {k} numbers, got {len(seq)}")
        if not all(math.isfinite(x) for x in seq):
            raise ValueError(f"{name} must be finite, got {v}")
        if name == "shininess" and not seq[0] > 0.0:
            raise ValueError(f"shininess must be > 0, got {v}")
        out.append((name, k, tuple(seq) if len(seq) == k else tuple(seq) * k))
    return out


def _light_rows(lighting, cam, headlight):
    """The (views, 10) rows the kernels read, built from the checked lighting arguments with torch operations on cam's device:
    autograd carries the kernels' d_light back to every tensor among them, summed over the views for a shared one.
    cam (views, 3): the cameras, detached; with headlight the light's position is cam + light_pos, formed in float32."""
    views, dev = cam.shape[0], cam.device
    cols = []
    for (name, k, v), (_, _, default) in zip(lighting, _LIGHTING):
        if not torch.is_tensor(v):
            v = torch.tensor(default if v is None else v, dtype=torch.float32, device=dev)
        t = v.to(device=dev, dtype=torch.float32)
        t = t.reshape(1, 1).expand(views, k) if t.ndim == 0 else t.reshape(-1, k).expand(views, k)
        if name == "light_pos" and headlight:
            t = cam + t
        cols.append(t)
    return torch.cat(cols, dim=1)


class LitRaycastFunction(torch.autograd.Function):
    """Autograd boundary of the lit march: `apply(rc, volume, tf, look_from, light, sampling_rate, batched, jitter, pose)`.
    volume (W,D,H) or (BS,W,D,H), any strides; tf (R,4) or (BS,R,4); look_from (views,3); light (views,10): world position,
    colour, ambient, diffuse, specular, shininess. Returns (W,H,4) or (BS,W,H,4). d look_from is not defined here."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rc, volume, tf, look_from, light, sampling_rate, batched, jitter=True, pose=None):
        tf = tf.float().contiguous()
        light = light.float().contiguous()
        march = lambda volume, cam, rays: F.march_lit_fwd(volume, tf, cam, light, *rays, rc.max_samples, sampling_rate,
                                                          N.DR_MODE_DIFF)
        return L.march_forward(ctx, rc, march, volume, (tf, light), look_from, sampling_rate, batched, jitter, pose)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        (volume, tf, light, e, x, r, n, out), cam, *_ = L.saved_rays(ctx)
        g = grad_output if ctx.batched else grad_output[None]
        dv, dt, dl = F.march_lit_bwd(volume, tf, cam, light, e, x, r, n, ctx.rc.max_samples, ctx.sampling_rate, g, out,
                                     want_vol=ctx.needs_input_grad[1], want_tf=ctx.needs_input_grad[2],
                                     want_light=ctx.needs_input_grad[4])
        return None, L.sanitised(dv), L.sanitised(dt), None, dl, None, None, None, None   # (d_light: sanitised in functional)


class RaycasterLit(L.RayModule):
    """Raycaster (1-D transfer function) with a differentiable light and Phong material.

    volume_shape (D, H, W), output_shape (H, W) and tf_shape (R) as for Raycaster. headlight=True: light_pos is an offset added
    to look_from (default (0, 1, 0), the reference's light); headlight=False: light_pos is a world position.
    forward(volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3), light_pos, light_color, ambient, diffuse, specular,
    shininess) -> ([BS,]4,H,W)."""

    def __init__(self, volume_shape, output_shape, tf_shape, sampling_rate=1.0, jitter=True, max_samples=512, fov=30.0,
                 near=0.1, far=100.0, headlight=True):
        self._check_built(volume_shape, output_shape, tf_shape)
        super().__init__(volume_shape, output_shape, sampling_rate, jitter, max_samples, fov, near, far)
        self.tf_shape = int(tf_shape)
        self.headlight = bool(headlight)

    def _batch(self, volume, tf, look_from, lighting, pose=None):
        """-> (batched, vol ([BS,] W, D, H) view, tf ([BS,] R, 4) view, look_from (views, 3), pose); un-batched inputs are shared
        by all views. A (BS, k) lighting tensor joins the batch rule like any other input, and so does pose = (look_at, up, fov),
        which comes back as rows per view; else None."""
        self._check_tf_inputs(volume, tf, look_from)
        inputs = ((volume, 5), (tf, 3), *((v, 2) for _, _, v in lighting if torch.is_tensor(v)))
        batched, lf, pose = L.views(look_from, pose, *inputs)
        return batched, L.field_view(volume), tf.transpose(-1, -2), lf, pose

    def _prepare(self, volume, tf, look_from, lighting_values, look_at, up, fov):
        """Every check that needs no device, then the views' inputs -> (batched, vol, tf, lf, light rows (views, 10), pose)."""
        L.refuse_pose_grad("RaycasterLit", look_from=look_from, look_at=look_at, up=up, fov=fov)
        lighting = _check_lighting(lighting_values)
        batched, vol, tf_in, lf, pose = self._batch(volume, tf, look_from, lighting, L.pose_or_none(look_at, up, fov))
        light = _light_rows(lighting, lf.detach().to(torch.float32), self.headlight)
        return batched, vol, tf_in, lf, light, pose

    def forward(self, volume, tf, look_from, light_pos=None, light_color=None, ambient=None, diffuse=None, specular=None,
                shininess=None, look_at=None, up=None, fov=None):
        """volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3) -> ([BS,]4,H,W).
        light_pos, light_color (3 components), ambient, diffuse, specular, shininess (1): each None (the reference's value), a
        Python number (or 3 numbers), or a tensor of shape (), (k,) or (BS, k); one that requires grad receives its gradient, a
        shared one the sum over the views. light_pos is an offset from look_from with headlight=True, else a world position.
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera. No camera tensor may require grad: camera
        gradients are volume_raycaster.Raycaster's."""
        batched, vol, tf_in, lf, light, pose = self._prepare(volume, tf, look_from, (light_pos, light_color, ambient, diffuse,
                                                                                     specular, shininess), look_at, up, fov)
        res = LitRaycastFunction.apply(self, vol, tf_in, lf, light, self.sampling_rate, batched, self.jitter, pose)
        return self._image(res, batched)

    def raycast_nondiff(self, volume, tf, look_from, sampling_rate=None, light_pos=None, light_color=None, ambient=None,
                        diffuse=None, specular=None, shininess=None, look_at=None, up=None, fov=None):
        """Non-differentiable render (never jittered, lighting not clamped); default rate 4x the module's, as
        Raycaster.raycast_nondiff."""
        with torch.no_grad():
            batched, vol, tf_in, lf, light, pose = self._prepare(volume, tf, look_from, (light_pos, light_color, ambient, diffuse,
                                                                                         specular, shininess), look_at, up, fov)
        march = lambda vol, cam, rays, sr: F.march_lit_fwd(vol, tf_in.float().contiguous(), cam, light, *rays, self.max_samples, sr,
                                                           N.DR_MODE_NONDIFF)
        return self._raycast_nondiff(vol, lf, sampling_rate, pose, batched, march)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), TF ({self.tf_shape}), "
                f"Max Samples = {self.max_samples}, headlight = {self.headlight}")
