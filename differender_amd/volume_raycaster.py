"""Drop-in host side of Differender's `differender.volume_raycaster` on MI355X.

Same public surface as the reference module (`VolumeRaycaster`, `RaycastFunction`, `Raycaster`;
reference: differender/volume_raycaster.py, "VR.py"), but every kernel is a hand-written HIP kernel
behind the C ABI of include/differender_hip.h; no Taichi, no tape, no per-item Python loops.

Differences from the reference that a caller can observe (all documented in DESIGN.md):
  * batched calls run all views in one native launch; an un-batched volume/tf is shared, not cloned
    BS times (VR.py:566-568), and receives one accumulated gradient;
  * the ray buffers and the jitter seed of the forward pass are saved in the autograd context, so
    backward differentiates the image that was actually returned (the reference re-renders with new
    jitter, VR.py:452-458) and a second forward before backward is harmless (VR.py:429-430);
  * there is no render tape: `max_samples` only bounds the number of marched samples (H2);
  * flat-normal samples contribute no normal-path gradient instead of NaN (H3).
"""
import math
import os
import warnings

import torch

from . import _layout as L
from . import _native as N
from . import functional as F

__all__ = ["VolumeRaycaster", "RaycastFunction", "Raycaster"]


class _Field:
    """Tensor-backed stand-in for the ti.field objects user code may poke (`vr.volume.grad.to_torch()`)."""

    def __init__(self, owner, name, needs_grad=False):
        self._owner, self._name = owner, name
        self.grad = _Field(owner, name + "_grad") if needs_grad else None

    @property
    def tensor(self):
        return getattr(self._owner, "_" + self._name)

    @property
    def shape(self):
        t = self.tensor
        if t is None:
            return self._owner._field_shape(self._name)
        return tuple(t.shape[:-1]) if self._name in ("tf_tex", "tf_tex_grad", "output_rgba", "output_rgba_grad",
                                                     "rays") else tuple(t.shape)

    @property
    def n(self):  # vector width of ti.Vector.field
        return {"tf_tex": 4, "tf_tex_grad": 4, "output_rgba": 4, "output_rgba_grad": 4, "rays": 3}.get(self._name, 1)

    def from_torch(self, t):
        setattr(self._owner, "_" + self._name, t)

    def to_torch(self, device=None):
        t = self.tensor
        if t is None:
            raise RuntimeError(f"field `{self._name}` has not been produced yet")
        return t if device is None else t.to(device)

    def fill(self, value):
        t = self.tensor
        if t is not None:
            t.fill_(value)


class _Kernel:
    """Callable with a `.grad` attribute, mirroring how Taichi exposes `kernel.grad` (VR.py:460-461)."""

    def __init__(self, fwd, bwd=None):
        self._fwd, self.grad = fwd, bwd

    def __call__(self, *a, **k):
        return self._fwd(*a, **k)


class VolumeRaycaster:
    """Stateful single-view kernel host with the method names of the reference class (VR.py:56-389).

    State is a handful of torch tensors; each method enqueues the corresponding HIP kernel. The
    autograd path (`RaycastFunction`) does not go through this object's state -- it calls the batched
    functional ops directly -- but the step-by-step API keeps working for scripts written against it.
    """

    def __init__(self, volume_resolution, render_resolution, max_samples=512, tf_resolution=128, fov=30.0,
                 nearfar=(0.1, 100.0)):
        self.resolution = tuple(render_resolution)
        self.aspect = render_resolution[0] / render_resolution[1]
        self.fov_deg = fov
        self.fov_rad = math.radians(fov)  # VR.py:77
        self.near, self.far = nearfar
        self.max_samples = max_samples
        self.volume_resolution = tuple(volume_resolution)
        self.tf_resolution = tf_resolution
        self.ambient, self.diffuse, self.specular, self.shininess = 0.4, 0.8, 0.3, 32.0  # VR.py:91-94 (fixed in-kernel)
        for name in ("volume", "tf_tex", "cam_pos", "entry", "exit", "rays", "sample_step_nums",
                     "steps", "output_rgba", "volume_grad", "tf_tex_grad", "output_rgba_grad",
                     "tape_last", "workspace"):
            setattr(self, "_" + name, None)
        self.volume = _Field(self, "volume", needs_grad=True)
        self.tf_tex = _Field(self, "tf_tex", needs_grad=True)
        self.output_rgba = _Field(self, "output_rgba", needs_grad=True)
        self.cam_pos = _Field(self, "cam_pos")
        self.entry, self.exit, self.rays = _Field(self, "entry"), _Field(self, "exit"), _Field(self, "rays")
        self.sample_step_nums = _Field(self, "sample_step_nums")
        self.valid_sample_step_count = _Field(self, "valid_sample_step_count")
        self.raycast = _Kernel(self._raycast, self._raycast_grad)
        self.get_final_image = _Kernel(self._get_final_image, self._get_final_image_grad)
        self._jitter_seed = 0
        self._sr = 1.0
        self._stats_host, self._stats_event, self._stats_rays = None, None, 0
        self.last_stats = None         # workspace header of the most recent forward whose snapshot has arrived (int32 x32)
        self._warned_fallback = False
        self._warned_stale = False
        self._fwd_seq, self._snap_seq, self._reported_seq = 0, 0, -1   # forwards issued / the one a snapshot shows / the one last reported

    def _watch_workspace(self, workspace, n_rays, forward=False):
        """Keeps an eye on the fast path's fallback counters without ever synchronising: a 128-byte snapshot of the
        workspace header is copied to pinned memory after a forward or a backward, and looked at when a LATER call finds it
        complete. Warns once if more than 1 % of the rays had to be marched one by one (single-sample rays or rays whose
        segments failed the count check: correct, but the 10-40x slower kernels)."""
        if forward:
            self._fwd_seq += 1
        if workspace is None:
            return
        if self._stats_event is not None and self._stats_event.query():
            self.last_stats = self._stats_host.clone()
            slow = int(self.last_stats[2])
            # the device found a "no early termination" hint wrong: reported once per FORWARD (its backward's snapshot shows the
            # same header). Keyed on a count of the forwards issued here, not on the header's fingerprint: a training loop renders
            # the same volume into the same recycled buffers, so every iteration's fingerprint is the same and all wrong-hint
            # reports after the first would be dropped
            if int(self.last_stats[8]) and self._snap_seq != self._reported_seq:
                self._reported_seq = self._snap_seq
                F._hints.report_wrong_hint()
            if int(self.last_stats[9]) and not self._warned_stale:
                self._warned_stale = True
                warnings.warn("differender_amd: a backward pass did not find its forward's coarse tape in the workspace it "
                              "was given (fingerprint mismatch) and marched every ray with the per-ray kernels: correct, "
                              "but 10-40x slower -- pass the forward's ray buffers, volume and workspace unchanged",
                              RuntimeWarning, stacklevel=3)
            if slow > 0.01 * self._stats_rays and not self._warned_fallback:
                self._warned_fallback = True
                warnings.warn(f"differender_amd: {slow} of {self._stats_rays} rays were marched by the per-ray fallback "
                              "kernels in a recent render (functional.workspace_stats): expect a slow-down",
                              RuntimeWarning, stacklevel=3)
            self._stats_event = None
        if self._stats_event is None:
            if self._stats_host is None:
                self._stats_host = torch.empty(32, dtype=torch.int32, pin_memory=True)
            with torch.cuda.device(workspace.device):   # (the event must sit on the stream the copy runs on)
                self._stats_host.copy_(workspace[:128].view(torch.int32), non_blocking=True)
                self._stats_event = torch.cuda.Event()
                self._stats_event.record()
            self._stats_rays = int(n_rays)
            self._snap_seq = self._fwd_seq

    def _field_shape(self, name):
        if name.startswith("volume"):
            return self.volume_resolution
        if name.startswith("tf_tex"):
            return (self.tf_resolution,)
        return self.resolution

    @property
    def _valid_sample_step_count(self):
        """The reference's field starts at 1 and counts one per live sample (VR.py:303,381); the kernels report
        the live samples themselves (`steps`)."""
        return None if self._steps is None else self._steps + 1

    @_valid_sample_step_count.setter
    def _valid_sample_step_count(self, t):
        self._steps = None if t is None else t - 1

    # -- setters (VR.py:118-125): keep a float32 (or float16) view, no relayout copy
    def set_volume(self, volume):
        self._volume = F.as_volume(volume)

    def set_tf_tex(self, tf_tex):
        self._tf_tex = tf_tex.float().contiguous()

    def set_cam_pos(self, cam_pos):
        self._cam_pos = cam_pos.float().reshape(1, 3).contiguous()

    @property
    def max_valid_sample_step_count(self):
        """VR.py:89,370-372 diagnostic: max over pixels of valid_sample_step_count - 1 (computed on demand; forces a
        device sync)."""
        return 0 if self._steps is None else int(self._steps.max().item())

    def clear_framebuffer(self):  # VR.py:374-382
        dev = self._volume.device
        self._output_rgba = torch.zeros((*self.resolution, 4), dtype=torch.float32, device=dev)
        self._steps = torch.zeros(self.resolution, dtype=torch.int32, device=dev)  # valid_sample_step_count = 1
        self._tape_last = None

    def clear_grad(self):  # VR.py:384-389
        self._volume_grad = None
        self._tf_tex_grad = None
        self._output_rgba_grad = None

    def compute_entry_exit(self, sampling_rate, jitter):  # VR.py:221-259
        self._jitter_seed = F.new_jitter_seed() if jitter else 0
        e, x, r, n = F.ray_setup(self._cam_pos, self.resolution, self._volume.shape, sampling_rate, self.fov_deg,
                                 self.near, self._jitter_seed)
        self._entry, self._exit, self._rays, self._sample_step_nums = e[0], x[0], r[0], n[0]

    def _march(self, sampling_rate, mode):
        self._workspace = F.alloc_workspace(1, self.resolution, self._volume.shape, self._tf_tex.shape[0],
                                            self._volume.device)
        out, steps = F.march_fwd(self._volume, self._tf_tex, self._cam_pos, self._entry[None], self._exit[None],
                                 self._rays[None], self._sample_step_nums[None], self.max_samples, sampling_rate, mode,
                                 fov_deg=self.fov_deg, near=self.near, workspace=self._workspace)
        self._tape_last = out[0]
        self._steps = steps[0]
        self._sr = sampling_rate

    def _raycast(self, sampling_rate):  # VR.py:261-306
        self._march(sampling_rate, N.DR_MODE_DIFF)

    def raycast_nondiff(self, sampling_rate):  # VR.py:308-351
        self._march(sampling_rate, N.DR_MODE_NONDIFF)

    def _get_final_image(self):  # VR.py:363-372
        self._output_rgba = self._output_rgba + self._tape_last

    def get_final_image_nondiff(self):  # VR.py:353-361 (the clamp to <= 1 is fused into the march kernel)
        self._output_rgba = self._tape_last

    def _get_final_image_grad(self):
        if self._output_rgba_grad is None:
            raise RuntimeError("set vr.output_rgba.grad.from_torch(grad) before get_final_image.grad()")

    def _raycast_grad(self, sampling_rate):
        dv, dt = F.march_bwd(self._volume, self._tf_tex, self._cam_pos, self._entry[None], self._exit[None],
                             self._rays[None], self._sample_step_nums[None], self.max_samples, sampling_rate,
                             self._output_rgba_grad[None], self._tape_last[None], fov_deg=self.fov_deg,
                             near=self.near, workspace=self._workspace)
        self._volume_grad = dv if self._volume_grad is None else self._volume_grad + dv
        self._tf_tex_grad = dt if self._tf_tex_grad is None else self._tf_tex_grad + dt


def tape_fits(n_views, out_shape, vol_shape, R, max_samples, sampling_rate):
    """Is the per-sample tape of a TF-only forward (DR_TAPE_TF) worth its memory here? It has a fixed stride per ray (8 B x the longest
    march the volume allows), known up front: 6.4 GB per 512^2 view of a 512^3 volume, 49 GB per 1024^2 view of a 1024^3 one. Above
    DIFFERENDER_TAPE_MAX_GIB (default 64 of the card's 288) the brick-centric TF-only backward serves the call instead: same results,
    ~1.4x the step, no tape."""
    cap = int(float(os.environ.get("DIFFERENDER_TAPE_MAX_GIB", "64")) * (1 << 30))
    need = F.tape_workspace_bytes(n_views, out_shape, vol_shape, R, max_samples, sampling_rate)
    return 0 < need <= cap


class RaycastFunction(torch.autograd.Function):
    """Autograd boundary (VR.py:392-476). `apply(vr, volume, tf, look_from, sampling_rate, (batched, bs), jitter)`.

    volume: (W,D,H) or (BS,W,D,H), any strides; tf: (R,4) or (BS,R,4); look_from: (3,) or (BS,3).
    Unlike the reference, un-batched volume/tf may be combined with batched look_from: they are shared by
    all views and receive one accumulated gradient.
    Returns (W,H,4) or (BS,W,H,4)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, vr, volume, tf, look_from, sampling_rate, batched, jitter=True, hints="auto"):
        is_batched, bs = batched
        cam = look_from.reshape(-1, 3)
        if is_batched and cam.shape[0] != bs:
            cam = cam.expand(bs, 3)
        volume = F.as_volume(volume)          # set_volume's .float() (VR.py:119); float16 storage is kept
        tf = tf.float().contiguous()          # set_tf_tex's .float() (VR.py:122)
        seed = F.new_jitter_seed() if jitter else 0
        e, x, r, n = F.ray_setup(cam, vr.resolution, volume.shape[-3:], sampling_rate, vr.fov_deg, vr.near, seed)
        # only the transfer function is being optimised (the reference's TF demo; BASELINE config C3): the forward leaves a
        # per-sample tape of (intensity, lighting) and the backward never touches the volume again (csrc/tf_tape.hip)
        tape = bool(ctx.needs_input_grad[2] and not ctx.needs_input_grad[1]) and tape_fits(
            cam.shape[0], vr.resolution, volume.shape[-3:], tf.shape[-2], vr.max_samples, sampling_rate)
        ws = F.alloc_workspace(cam.shape[0], vr.resolution, volume.shape[-3:], tf.shape[-2], volume.device,
                               tape=(vr.max_samples, sampling_rate) if tape else None)
        tape = tape and ws is not None
        out, steps = F.march_fwd(volume, tf, cam, e, x, r, n, vr.max_samples, sampling_rate, N.DR_MODE_DIFF,
                                 fov_deg=vr.fov_deg, near=vr.near, workspace=ws, hints=hints, tape=tape)
        # the camera gradient needs the forward's live samples; nothing more is kept when it is not asked for
        ctx.want_cam = bool(ctx.needs_input_grad[3])
        ctx.save_for_backward(volume, tf, cam, e, x, r, n, out, *((steps,) if ctx.want_cam else ()))
        ctx.lf_shape, ctx.lf_dtype = look_from.shape, look_from.dtype
        ctx.workspace = ws  # coarse tape of the forward (per-segment prefixes), consumed by backward
        ctx.tape = tape
        ctx.vr, ctx.sampling_rate, ctx.batched, ctx.jitter_seed = vr, sampling_rate, is_batched, seed
        vr._steps = steps if is_batched else steps[0]
        vr._watch_workspace(ws, n.numel(), forward=True)
        return out if is_batched else out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        volume, tf, cam, e, x, r, n, out = ctx.saved_tensors[:8]
        g = grad_output if ctx.batched else grad_output[None]
        want_vol, want_tf = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dv, dt = F.march_bwd(volume, tf, cam, e, x, r, n, ctx.vr.max_samples, ctx.sampling_rate, g, out,
                             want_vol=want_vol, want_tf=want_tf, fov_deg=ctx.vr.fov_deg, near=ctx.vr.near,
                             workspace=ctx.workspace, tape=ctx.tape and not want_vol)
        ctx.vr._watch_workspace(ctx.workspace, n.numel())
        # VR.py:463-464,474-475: nan_to_num. The fast kernels drop NaN adjoints and clamp infinite ones themselves
        # ("non-finite upstream gradients"), so the two full passes over d_volume are only run when the
        # plain kernels served the call.
        if not F.bwd_is_sanitised(volume, tf, dv, ctx.workspace, n):
            if dv is not None:
                dv = torch.nan_to_num(dv)
            if dt is not None:
                dt = torch.nan_to_num(dt)
        d_cam = None
        if ctx.want_cam:   # after march_bwd, on the same stream
            d_cam = F.march_bwd_cam(volume, tf, cam, e, x, r, n, ctx.saved_tensors[8], ctx.vr.max_samples, ctx.sampling_rate,
                                    g, out, fov_deg=ctx.vr.fov_deg, near=ctx.vr.near, jitter_seed=ctx.jitter_seed)
            # back to the shape look_from came in: an un-batched camera expanded to the batch's views gets their sum
            if d_cam.shape[0] * 3 != math.prod(ctx.lf_shape):
                d_cam = d_cam.sum(0)
            d_cam = d_cam.reshape(ctx.lf_shape).to(ctx.lf_dtype)
        return None, dv, dt, d_cam, None, None, None, None


class Raycaster(torch.nn.Module):
    """VR.py:478-574. `ti_kwargs` is accepted and ignored (there is no Taichi runtime)."""

    def __init__(self, volume_shape, output_shape, tf_shape, sampling_rate=1.0, jitter=True, max_samples=512,
                 fov=30.0, near=0.1, far=100.0, ti_kwargs={}):
        super().__init__()
        self.volume_shape = (volume_shape[2], volume_shape[0], volume_shape[1])  # (W, D, H), VR.py:481
        self.output_shape = output_shape
        self.tf_shape = tf_shape
        self.sampling_rate = sampling_rate
        self.jitter = jitter
        N.lib()  # fail loudly at construction time if the HIP library is missing
        self.vr = VolumeRaycaster(self.volume_shape, output_shape, max_samples=max_samples, tf_resolution=tf_shape,
                                  fov=fov, nearfar=(near, far))

    def _determine_batch(self, volume, tf, look_from, pose=None):
        """VR.py:551-571, without the copies: returns (batched, bs, vol, tf, lf) where vol is the
        ([BS,] W, D, H) *view* of the input, tf is ([BS,] R, 4); un-batched inputs stay un-batched (shared).
        pose = (look_at, up, fov): they join the batch rule, and a sixth result holds them as rows per view (_layout.pose_rule)."""
        if volume.ndim not in (4, 5) or tf.ndim not in (2, 3) or look_from.ndim not in (1, 2):
            raise ValueError("expected volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3)")
        inputs = ((volume, 5), (tf, 3))
        batched, bs, lf, *posed = L.batch_rule(look_from, *inputs) if pose is None else L.pose_rule(look_from, pose, *inputs)
        # (the un-batched look_from stays (3,), as the reference hands it on)
        return (batched, bs, L.field_view(volume), tf.transpose(-1, -2), lf if batched else look_from, *posed)

    def _hints(self, tf, vol_in, sampling_rate, mode):
        """DR_HINT_* from the USER's TF tensor ([BS,] 4, R) -- the object that lives across iterations and whose version
        counter torch keeps; the (R, 4) copy handed to the kernels is a fresh temporary every call."""
        if not tf.is_cuda:
            return 0
        return F.termination_hints(tf, vol_in.shape[-3:], sampling_rate, self.vr.max_samples, mode,
                                   alpha=lambda t: t[..., 3, :])

    def raycast_nondiff(self, volume, tf, look_from, sampling_rate=None, look_at=None, up=None, fov=None):
        """VR.py:490-523: non-differentiable render (never jittered); default rate 4x the module's.
        look_at, up ([BS,]3), fov ([BS,] degrees): the free camera, as in forward."""
        if L.has_pose(look_at, up, fov):
            batched, bs, vol_in, tf_in, lf_in, pose = self._determine_batch(volume, tf, look_from, (look_at, up, fov))
            with L.nondiff_rays(vol_in, lf_in, sampling_rate, self.sampling_rate, self.vr.resolution, self.vr.fov_deg,
                                self.vr.near, pose) as (sr, vol_in, cam, rays, pose9, fov_v):
                out, steps = F.march_fwd(vol_in, tf_in.float().contiguous(), cam, *rays, self.vr.max_samples, sr,
                                         N.DR_MODE_NONDIFF, fov_deg=self.vr.fov_deg, near=self.vr.near,
                                         hints=self._hints(tf, vol_in, sr, N.DR_MODE_NONDIFF), pose=pose9, fov_v=fov_v)
                self.vr._steps = L.unbatch(steps, batched)
                return L.image(L.unbatch(out, batched))
        batched, bs, vol_in, tf_in, lf_in = self._determine_batch(volume, tf, look_from)
        with L.nondiff_rays(vol_in, lf_in, sampling_rate, self.sampling_rate, self.vr.resolution, self.vr.fov_deg,
                            self.vr.near) as (sr, vol_in, cam, rays):
            out, steps = F.march_fwd(vol_in, tf_in.float().contiguous(), cam, *rays, self.vr.max_samples, sr,
                                     N.DR_MODE_NONDIFF, fov_deg=self.vr.fov_deg, near=self.vr.near,
                                     hints=self._hints(tf, vol_in, sr, N.DR_MODE_NONDIFF))
            self.vr._steps = L.unbatch(steps, batched)
            return L.image(L.unbatch(out, batched))

    def forward(self, volume, tf, look_from, look_at=None, up=None, fov=None):
        """VR.py:525-548. volume ([BS,]1,D,H,W), tf ([BS,]4,R), look_from ([BS,]3) -> ([BS,]4,H,W).
        look_at, up ([BS,]3), fov ([BS,] degrees, a 0-d tensor or a number): the free camera (pose.py), with
        gradients for every one that requires grad; a missing one is the origin, +y, the module's fov. All None: the reference's
        camera and this method as it always was."""
        if L.has_pose(look_at, up, fov):
            from .pose import PoseRaycastFunction
            batched, bs, vol_in, tf_in, lf_in, pose = self._determine_batch(volume, tf, look_from, (look_at, up, fov))
            res = PoseRaycastFunction.apply(self.vr, vol_in, tf_in, lf_in, *pose, self.sampling_rate, (batched, bs), self.jitter,
                                            self._hints(tf, vol_in, self.sampling_rate, N.DR_MODE_DIFF))
            return L.image(res)
        batched, bs, vol_in, tf_in, lf_in = self._determine_batch(volume, tf, look_from)
        res = RaycastFunction.apply(self.vr, vol_in, tf_in, lf_in, self.sampling_rate, (batched, bs), self.jitter,
                                    self._hints(tf, vol_in, self.sampling_rate, N.DR_MODE_DIFF))
        return L.image(res)

    def extra_repr(self):
        return (f"Volume ({self.volume_shape}), Output Render ({self.output_shape}), TF ({self.tf_shape}), "
                f"Max Samples = {self.vr.max_samples}")
