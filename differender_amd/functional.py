"""Tensor-level wrappers over the C ABI (include/differender_hip.h).

Buffers are torch tensors on a ROCm device; the HIP library allocates nothing and runs on the
current torch stream. Volume tensors live in the reference's field index space (VX, VY, VZ) =
(W, D, H) of the user's (1, D, H, W) tensor (VR.py:481) and may have arbitrary strides, so the
permuted view of VR.py:566,571 is consumed without a copy.
"""
import ctypes
import math
import warnings

import numpy as np
import torch

from . import _native as N

__all__ = ["ray_setup", "ray_setup_pose", "pack_pose", "march_fwd", "march_bwd", "march_bwd_cam", "march_bwd_pose", "project_bwd_pose", "march_tf2d_fwd", "march_tf2d_bwd", "march_lit_fwd", "march_lit_bwd", "default_light", "march_rgba_fwd", "march_rgba_bwd", "march_depth_fwd", "march_depth_bwd", "march_depth_bwd_cam", "march_depth_bwd_pose", "project_fwd", "project_bwd",
           "project_bwd_cam", "new_jitter_seed", "alloc_workspace", "workspace_stats", "evaluated_samples",
           "mse_loss_grad", "dssim_mse_fwd", "dssim_mse_bwd", "dssim_mse_loss_grad", "msssim_mse_fwd", "msssim_mse_bwd",
           "msssim_mse_loss_grad", "tv3d_fwd", "tv3d_bwd", "tf_momentum_step", "as_volume", "bwd_is_sanitised", "termination_hints"]
__all__ += ["bundle_setup", "march_bundle_fwd", "march_bundle_bwd", "march_bundle_bwd_rays"]
__all__ += ["project_bundle_fwd", "project_bundle_bwd", "project_bundle_bwd_rays"]
__all__ += ["march_rgba_bundle_fwd", "march_rgba_bundle_bwd", "march_rgba_bundle_bwd_rays"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, device, *args):
    """The C entry `name` on `device`, on its current stream (the entry's last argument); an error names the entry."""
    with torch.cuda.device(device):
        rc = getattr(N.lib(), name)(*args, _stream())
    N.check(rc, name)


def _require_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"differender_amd: `{name}` must live on a ROCm GPU (got {t.device}); "
                           "there is no CPU path")


def as_volume(vol):
    """The reference's setters call `.float()` on whatever they are given (VR.py:118-125): float64, bfloat16 or
    integer volumes are converted; float32 and float16 (storage extension) pass through untouched."""
    return vol if vol.dtype in (torch.float32, torch.float16) else vol.float()


def bwd_is_sanitised(vol, tf, d_vol, workspace, n):
    """True if march_bwd(vol, tf, ..., n, ..., workspace=workspace) is served by the fast kernels, which sanitise their
    gradients themselves (dr_march_bwd_variant -- the function dr_march_bwd_rows itself asks; finite by construction, the float
    atomics that combine bricks saturate at +-FLT_MAX: include/differender_hip.h) -- also when the per-ray second pass ends up
    serving the whole call (a stale workspace, a repaired wrong hint): it sanitises whenever it runs for this path; False for the plain kernels, which propagate NaN like the reference and want the
    reference's nan_to_num. n: the (views, W, H) sample-count buffer of the call."""
    if workspace is None:
        return False
    if workspace.numel() == 0:
        return False
    sv = vol.stride()[-3:]
    sd = d_vol.stride()[-3:] if d_vol is not None else (0, 0, 0)
    V, W, H = (int(v) for v in n.shape)
    return N.lib().dr_march_bwd_variant(V, W, H, *(int(v) for v in vol.shape[-3:]), int(tf.shape[-2]), *sv, *sd,
                                        int(d_vol is not None), N.DR_VARIANT_AUTO, 1) == N.DR_VARIANT_AUTO


def _dtype_tag(vol, rule):
    """DR_F32 / DR_F16 of a volume the kernels read as it is; `rule` words the TypeError of any other dtype."""
    if vol.dtype == torch.float32:
        return N.DR_F32
    if vol.dtype == torch.float16:
        return N.DR_F16
    raise TypeError(f"{rule}, got {vol.dtype}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _vol_args(vol, n_views):
    """-> (ptr, dtype_tag, VX, VY, VZ, sx, sy, sz, view_stride)"""
    tag = _dtype_tag(vol, "volume dtype must be float32 or float16")
    if vol.ndim == 3:
        vs, (VX, VY, VZ), (sx, sy, sz) = 0, vol.shape, vol.stride()
    elif vol.ndim == 4:
        if vol.shape[0] != n_views:
            raise ValueError(f"batched volume has {vol.shape[0]} items, expected {n_views}")
        vs, (VX, VY, VZ), (sx, sy, sz) = vol.stride(0), vol.shape[1:], vol.stride()[1:]
    else:
        raise ValueError("volume must be (VX,VY,VZ) or (views,VX,VY,VZ)")
    return vol.data_ptr(), tag, VX, VY, VZ, sx, sy, sz, vs


def _tf_args(tf, n_views):
    if tf.dtype != torch.float32 or not tf.is_contiguous():
        raise TypeError("tf must be a contiguous float32 tensor")
    if tf.ndim == 2 and tf.shape[1] == 4:
        return tf.data_ptr(), tf.shape[0], 0
    if tf.ndim == 3 and tf.shape[2] == 4 and tf.shape[0] == n_views:
        return tf.data_ptr(), tf.shape[1], tf.stride(0)
    raise ValueError("tf must be (R,4) or (views,R,4)")


def new_jitter_seed():
    """Non-zero 32-bit seed drawn from torch's CPU generator (so torch.manual_seed controls jitter)."""
    return int(torch.randint(1, 2 ** 31 - 1, (1,)).item())


def alloc_workspace(n_views, out_shape, vol_shape, R, device, tape=None):
    """Scratch buffer of the fast (brick-centric) kernels for one forward(+backward) pair, or None when only
    the baseline kernels can serve this problem (dr_workspace_bytes() == 0). The forward leaves its coarse
    tape here; hand the same buffer to march_bwd.
    tape=(max_samples, sampling_rate): room for the per-sample tape of a DR_TAPE_TF forward as well (march_fwd(tape=True) /
    march_bwd(tape=True): the backward w.r.t. the transfer function alone) -- 8 B per ray and possible sample."""
    W, H = int(out_shape[0]), int(out_shape[1])
    VX, VY, VZ = (int(s) for s in vol_shape)
    if tape is not None:
        nbytes = N.lib().dr_workspace_bytes_tape(int(n_views), W, H, VX, VY, VZ, int(R), int(tape[0]), float(tape[1]))
    else:
        nbytes = N.lib().dr_workspace_bytes(int(n_views), W, H, VX, VY, VZ, int(R))
    if nbytes == 0:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def tape_workspace_bytes(n_views, out_shape, vol_shape, R, max_samples, sampling_rate):
    """Bytes alloc_workspace(..., tape=(max_samples, sampling_rate)) would ask for (0: only the baseline kernels serve this problem).
    The tape has a fixed stride per ray -- the longest march the volume allows at this rate -- so it is known before any ray is:
    6.4 GB for one 512^2 view of a 512^3 volume at rate 1, 49 GB for a 1024^2 view of a 1024^3 volume."""
    W, H = int(out_shape[0]), int(out_shape[1])
    VX, VY, VZ = (int(s) for s in vol_shape)
    return int(N.lib().dr_workspace_bytes_tape(int(n_views), W, H, VX, VY, VZ, int(R), int(max_samples), float(sampling_rate)))


def workspace_stats(workspace):
    """Diagnostics the last forward left in the workspace header: [0] = rays whose segments failed the
    sample-count check and were marched individually (expected 0), [2] = all rays the per-ray fallback marched
    (those plus the irregular ones: single-sample rays), [4] = bricks whose d_volume box accumulated in double (last
    backward), [5] = overflow work items heavy bricks were cut into, [8] = views for which a DR_HINT_NO_EARLY_TERMINATION
    hint turned out wrong (their rays were marched one by one), [9] = backward calls that did not find their forward's
    fingerprint in this workspace and marched every ray one by one, [3] = the forward's fingerprint (0: nobody's),
    [12] = (ray, layer) segments the colour march skipped because the alpha pre-pass had found them unlit, [13] = brick workgroups
    (of all forward passes) that took the empty-brick path -- both SAMPLED (every 64th workgroup reports), 0 when the mechanisms have
    nothing to do; [15] = rays whose pixel was recomputed sample by sample in the reference's sequential float32 order
    (ray_exact_kernel, DESIGN.md D4: runs of contributions of the size of an ulp of the running composite)."""
    return workspace[:64].view(torch.int32).cpu()


def evaluated_samples(workspace):
    """(alpha pre-pass, colour march, backward): samples whose taps the brick kernels actually EVALUATED in the calls that were
    given DR_COUNT_EVALUATED (march_fwd(hints=... | N.DR_COUNT_EVALUATED), march_bwd(count_evaluated=True)) since the last forward
    -- the work-skipping paths (empty bricks, unlit segments) evaluate nothing for samples that still count as marched. bench.py
    prices its roofline with these, not with the marched count. Synchronises."""
    w = workspace[58 * 4:64 * 4].view(torch.int64).cpu()
    return int(w[0]), int(w[1]), int(w[2])


def _ws_args(workspace):
    if workspace is None:
        return None, 0
    return workspace.data_ptr(), workspace.numel()


def _rows(rows, W):
    """rows = None (whole image) or (row0, image_rows): the W buffer rows are image rows [row0, row0 + W)."""
    if rows is None:
        return int(W), 0
    row0, img_w = int(rows[0]), int(rows[1])
    if row0 < 0 or img_w < W or row0 > img_w - W:
        raise ValueError(f"band rows [{row0}, {row0 + W}) do not fit an image of {img_w} rows")
    return img_w, row0


def pack_pose(look_from, look_at=None, up=None):
    """The (views, 9) float32 pose the kernels read -- look_from, look_at, up of every view -- from look_from
    (views, 3) and look_at, up (views, 3), (3,) (shared by the views) or None (the origin, +y)."""
    cam = look_from.reshape(-1, 3).to(torch.float32)
    V = cam.shape[0]

    def rows(t, default):
        if t is None:
            return cam.new_tensor(default).expand(V, 3)
        t = t.to(device=cam.device, dtype=torch.float32).reshape(-1, 3)
        if t.shape[0] not in (1, V):
            raise ValueError(f"a pose entry has {t.shape[0]} rows, look_from {V}")
        return t.expand(V, 3)

    return torch.cat([cam, rows(look_at, (0.0, 0.0, 0.0)), rows(up, (0.0, 1.0, 0.0))], 1).contiguous()


def _pose_args(pose, fov_v, V):
    """A pose (views, 9) and its optional per-view fov in RADIANS (views,) as the float32 contiguous tensors the kernels read ->
    (pose, fov_v, then their two C-ABI arguments). The caller keeps the tensors until its call has been issued."""
    pose = pose.to(torch.float32).contiguous()
    if pose.shape != (V, 9):
        raise ValueError(f"pose must be (views, 9) = ({V}, 9): look_from, look_at, up; got {tuple(pose.shape)}")
    if fov_v is not None:
        fov_v = fov_v.to(device=pose.device, dtype=torch.float32).contiguous()
        if fov_v.shape != (V,):
            raise ValueError(f"fov_v must be (views,) = ({V},) radians, got {tuple(fov_v.shape)}")
    return pose, fov_v, pose.data_ptr(), _ptr(fov_v)


def ray_setup_pose(pose, out_shape, vol_shape, sampling_rate, fov_deg=30.0, near=0.1, jitter_seed=0, view_base=0, rows=None,
                   fov_v=None):
    """ray_setup for the free camera (dr_ray_setup_pose_rows): pose (views, 9) = look_from, look_at, up
    (pack_pose); fov_v (views,) float32 RADIANS gives every view its own field of view, None takes fov_deg for all. The default
    pose (look_at 0, up +y) without fov_v gives ray_setup's buffers bit for bit."""
    return _ray_setup(None, pose, fov_v, out_shape, vol_shape, sampling_rate, fov_deg, near, jitter_seed, view_base, rows)


def ray_setup(cam, out_shape, vol_shape, sampling_rate, fov_deg=30.0, near=0.1, jitter_seed=0, view_base=0, rows=None):
    """compute_entry_exit (VR.py:221-259) for cam (views,3) -> entry, exit (views,W,H), rays (views,W,H,3),
    n (views,W,H) int32. rows=(row0, image_rows) renders a band of a taller image (see distributed.shard_rows)."""
    return _ray_setup(cam, None, None, out_shape, vol_shape, sampling_rate, fov_deg, near, jitter_seed, view_base, rows)


def _ray_setup(cam, pose, fov_v, out_shape, vol_shape, sampling_rate, fov_deg, near, jitter_seed, view_base, rows):
    if pose is not None:
        _require_gpu(pose, "pose")
        pose, fov_v, *pargs = _pose_args(pose, fov_v, pose.shape[0])
        cam = pose
    else:
        _require_gpu(cam, "look_from")
        cam = cam.to(torch.float32).contiguous()
    V = cam.shape[0]
    W, H = int(out_shape[0]), int(out_shape[1])
    dev = cam.device
    entry = torch.empty((V, W, H), dtype=torch.float32, device=dev)
    exit_ = torch.empty((V, W, H), dtype=torch.float32, device=dev)
    rays = torch.empty((V, W, H, 3), dtype=torch.float32, device=dev)
    n = torch.empty((V, W, H), dtype=torch.int32, device=dev)
    VX, VY, VZ = (int(s) for s in vol_shape)
    args = (V, W, H, *_rows(rows, W), VX, VY, VZ, float(np.radians(fov_deg)), float(near), float(sampling_rate),
            int(jitter_seed) & 0xFFFFFFFF, int(view_base), entry.data_ptr(), exit_.data_ptr(), rays.data_ptr(), n.data_ptr())
    with torch.cuda.device(dev):
        if pose is None:
            rc = N.lib().dr_ray_setup_rows(cam.data_ptr(), *args, _stream())
        else:
            rc = N.lib().dr_ray_setup_pose_rows(None, *args, *pargs, _stream())
    N.check(rc, "dr_ray_setup_rows" if pose is None else "dr_ray_setup_pose_rows")
    return entry, exit_, rays, n


def _ray_args(vol, cam, entry, exit_, rays, n):
    """What every call on ray buffers starts with -> (cam, V, W, H, args): the camera as the float32 contiguous tensor the kernels
    read, the extents of the (views, W, H) ray buffers, and the eight C-ABI arguments cam, entry, exit, rays, n, V, W, H. The
    caller keeps `cam` (a temporary when it had to be converted) until its call has been issued."""
    _require_gpu(vol, "volume")
    V, W, H = n.shape
    cam = cam.to(torch.float32).contiguous()
    return cam, V, W, H, (cam.data_ptr(), entry.data_ptr(), exit_.data_ptr(), rays.data_ptr(), n.data_ptr(), V, W, H)


def _fwd_buffers(V, W, H, device, want_steps):
    """A march forward's out (views,W,H,4) float32 and steps (views,W,H) int32 (None when not wanted)."""
    out = torch.empty((V, W, H, 4), dtype=torch.float32, device=device)
    return out, torch.empty((V, W, H), dtype=torch.int32, device=device) if want_steps else None


def _bwd_images(grad_out, out):
    """A march backward's upstream gradient and forward image as the kernels read them: float32, contiguous."""
    return grad_out.to(torch.float32).contiguous(), out.contiguous()


def _cam_grad_buffers(V, W, H, device, per_ray, k=3):
    """A camera backward's d_cam (views, k), zeros in float64 for the workgroups' atomics, and the per-ray d_ray (views,W,H,k)
    float32 (None when not wanted); k = 3 for look_from, 10 for a pose."""
    d_cam = torch.zeros((V, k), dtype=torch.float64, device=device)
    return d_cam, torch.empty((V, W, H, k), dtype=torch.float32, device=device) if per_ray else None


def _cam_grad_result(d_cam, d_ray):
    """What a camera backward returns. D5: a sum beyond the float range saturates, as nan_to_num makes of d_tf."""
    d_cam = torch.nan_to_num(d_cam.float())
    return d_cam if d_ray is None else (d_cam, d_ray)


class _TerminationHints:
    """DR_HINT_* for march_fwd, derived from the transfer function WITHOUT ever synchronising with the device.

    Whether a ray can reach alpha 0.99 at all is a property of the TF's largest alpha (and of the longest possible ray): the
    library decides it on the device at the start of every forward and gates its alpha pre-pass off -- but the gated
    launches themselves (five per forward: ~45 us at 512^3, ~25 us at 256^3) are still issued, and how finely a pre-pass
    that DOES run should proceed front to back is a host decision too. A TF that is rendered again and again unchanged (a
    fixed TF under volume optimisation, OPT.py; the ground-truth TF; every benchmark) lets the host know: the largest alpha
    of a TF tensor is computed once per tensor VERSION (torch bumps `_version` on every in-place write, for every view and
    `.detach()` of the tensor alike), copied to pinned memory asynchronously, and used by later calls once the copy has landed
    (event.query(), never a wait). A TF seen for the first time gets no hint; one that is written to between calls gets
    "no early termination" never, and "early termination" from its last reading (refreshed every few calls). A stale answer
    (data changed behind the version counter's back) cannot produce a wrong image: the device re-checks and repairs
    (include/differender_hip.h).

    Writes the version counter does NOT see (`tf.data.add_()`, a raw-pointer write: `_version` stays put) would leave a
    reading "exact" for ever, and a TF whose alphas grow under such updates would keep getting "no early termination" -- which
    the device repairs correctly, but by marching every ray of the view with the per-ray kernels (10-40 x slower). Two
    safeguards: the largest alpha is re-read every REFRESH_EVERY-th call even when the version has not moved, and the device's
    own verdict feeds back -- when a workspace header reports a wrong hint (word 8, `report_wrong_hint`), the TFs that were
    recently GIVEN that hint (not every cached TF, and nothing at all if the hint was the caller's own: ADVICE r04) lose it for
    DISTRUST_REFRESHES re-readings of their largest alpha, twice as long after every further report (a wrong "no termination"
    is the only hint that costs anything)."""

    REFRESH_EVERY = 8   # the largest alpha of a TF is re-read on every 8th call at most (whether or not its version moved)
    DISTRUST_REFRESHES = 4   # clean re-readings before a TF that was given a wrong "no termination" hint may get it again

    def __init__(self, capacity=8):
        # key -> entry. The key is WHERE the data lives (storage address, offset, shape, strides) and the entry holds a
        # reference to the tensor, so that the memory cannot be handed to anybody else while the entry exists (a TF is a few
        # KB; at most `capacity` of them are kept): `tf.detach()` -- a new Python object every call, same storage, same
        # version counter -- matches; a temporary such as `tf.permute(1, 0).contiguous()` gets another address every call
        # and never does.
        self._seen = {}
        self._capacity = capacity
        self._handed = []            # keys of the TFs that were most recently given DR_HINT_NO_EARLY_TERMINATION (newest last)
        self._warned = False

    def report_wrong_hint(self):
        """The device found DR_HINT_NO_EARLY_TERMINATION wrong for some view of a recent render (workspace header word 8).
        If that hint came from here, the TFs it was recently derived from had their data moved behind the version counter's
        back: they lose it for a while (see the class docstring). A hint the CALLER passed explicitly is the caller's business:
        nothing is withdrawn. Returns the number of cached TFs that were blamed."""
        blamed = [self._seen[k] for k in self._handed if k in self._seen]
        self._handed = []
        for ent in blamed:
            ent["strikes"] += 1
            ent["distrust"] = min(self.DISTRUST_REFRESHES << (ent["strikes"] - 1), 1 << 16)
        if blamed and not self._warned:
            self._warned = True
            warnings.warn("differender_amd: the hint DR_HINT_NO_EARLY_TERMINATION (derived from the transfer function's largest "
                          "alpha) was wrong for a recent render -- the TF was written to without torch's version counter seeing "
                          "it (`tf.data`, a raw pointer). The device repaired the render (every ray marched one by one: slow); "
                          "the hint is withheld from that TF until its largest alpha has been re-read a few times.",
                          RuntimeWarning, stacklevel=4)
        return len(blamed)

    @staticmethod
    def _key(tf):
        return (tf.untyped_storage().data_ptr(), tf.storage_offset(), tuple(tf.shape), tuple(tf.stride()), tf.dtype)

    def invalidate(self, tf):
        base = tf.untyped_storage().data_ptr()
        for k in [k for k in self._seen if k[0] == base]:
            del self._seen[k]

    def _start_read(self, ent, tf, alpha):
        host = ent["host"]   # one pinned scalar per entry (at most one read of an entry is in flight)
        if host is None:
            host = ent["host"] = torch.empty((), dtype=torch.float32, pin_memory=True)
        with torch.no_grad(), torch.cuda.device(tf.device):   # (the event must sit on the stream the copy runs on)
            host.copy_(torch.nan_to_num(alpha(tf.detach()).float(), nan=float("inf")).max(), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        ent["pending"] = (host, ev, tf._version)
        ent["since"] = 0

    def amax(self, tf, alpha=lambda t: t[..., 3]):
        """(value, exact): the largest alpha of `tf` (inf if any alpha is NaN) as last read, and whether that reading is of
        the tensor's CURRENT version; (None, False) while nothing is known. Never waits for the device."""
        key = self._key(tf)
        ent = self._seen.get(key)
        if ent is None:
            if len(self._seen) >= self._capacity:
                self._seen.pop(next(iter(self._seen)))
            self._seen[key] = {"tensor": tf.detach(), "seen": tf._version, "value": None, "value_version": None,
                               "pending": None, "since": 0, "host": None, "distrust": 0, "strikes": 0}
            # A LEAF that requires grad is a parameter somebody optimises: it WILL be seen again (unlike a temporary -- and unlike
            # the result of a differentiable op, e.g. torch.sigmoid(logits): a new tensor every iteration that also "requires
            # grad"), so its largest alpha is read at once -- the harmless "many rays terminate" hint is then there from the second
            # or third iteration of a training loop instead of the ninth (OPT.py's TF: forward 1.81 -> 1.63 ms per iteration).
            if tf.requires_grad and tf.is_leaf:
                self._start_read(self._seen[key], tf, alpha)
            return None, False
        if ent["pending"] is not None and ent["pending"][1].query():
            host, _, ver = ent["pending"]
            ent["value"], ent["value_version"], ent["pending"] = float(host.item()), ver, None
            ent["distrust"] = max(ent["distrust"] - 1, 0)   # one more re-reading since the last wrong hint
        v = tf._version
        ent["since"] += 1
        if ent["value_version"] == v:
            # (re-read now and then all the same: `tf.data` writes do not bump the version)
            if ent["pending"] is None and ent["since"] >= self.REFRESH_EVERY:
                self._start_read(ent, tf, alpha)
            return ent["value"], ent["distrust"] == 0
        if ent["pending"] is None:
            # an unchanged tensor is read on the second sighting of its version; one that is written to between calls on
            # every REFRESH_EVERY-th call (its last reading keeps serving the harmless hint meanwhile)
            if ent["seen"] == v or ent["since"] >= self.REFRESH_EVERY:
                self._start_read(ent, tf, alpha)
        ent["seen"] = v
        return ent["value"], False

    def hints(self, tf, vol_shape, sampling_rate, max_samples, mode, alpha=lambda t: t[..., 3]):
        a, exact = self.amax(tf, alpha)
        if a is None:
            return 0
        # may_terminate() of the device (csrc/dr_brick_common.h), in double, with a margin on either side of its 0.02
        VX, VY, VZ = (int(v) for v in vol_shape)
        diag = math.sqrt((VX - 1) ** 2 + (VY - 1) ** 2 + (VZ - 1) ** 2)
        n_max = math.floor(float(sampling_rate) * 2.0 * math.sqrt(3.0) * diag) + 1.0
        if mode == N.DR_MODE_DIFF and n_max > max_samples:
            n_max = float(max_samples)
        n_max = max(n_max, 1.0)
        if not (a == a) or a == float("inf"):
            return 0
        base = max(1.0 - min(a, 1.0), 0.0)
        op = 1.0 - base ** (1.0 / float(sampling_rate))
        remain = (1.0 - op) ** n_max if op < 1.0 else 0.0
        # "no ray terminates" only from a reading of the CURRENT version (a wrong one costs a slow repair on the device);
        # "many rays terminate" also from the last reading of a tensor that has been written to since (OPT.py clamps its TF
        # in place every iteration): that hint only chooses how finely the pre-pass proceeds
        if exact and remain > 0.03:   # (the device's threshold is 0.02, evaluated in float: 1.5 x is a wide margin for rounding)
            key = self._key(tf)
            if not self._handed or self._handed[-1] != key:
                self._handed = [k for k in self._handed if k != key][-3:] + [key]
            return N.DR_HINT_NO_EARLY_TERMINATION
        if remain < 1e-4:
            return N.DR_HINT_EARLY_TERMINATION
        return 0


_hints = _TerminationHints()


def termination_hints(tf, vol_shape, sampling_rate, max_samples, mode, alpha=lambda t: t[..., 3]):
    """DR_HINT_* bits for march_fwd(hints=...) from a TF tensor the CALLER holds on to (see _TerminationHints); `alpha`
    selects its alpha entries when the layout is not (..., R, 4) -- e.g. `lambda t: t[..., 3, :]` for the user-facing
    ([BS,] 4, R) layout of Raycaster."""
    return _hints.hints(tf, vol_shape, sampling_rate, max_samples, mode, alpha)


def _pose_entry(name, pose, fov_v, V):
    """The entry point `name` and (None, None), or `name`_pose and _pose_args' (pose, fov_v, their two C-ABI arguments)."""
    if pose is None:
        if fov_v is not None:
            raise ValueError("fov_v comes with a pose")
        return getattr(N.lib(), name), (None, None)
    return getattr(N.lib(), name + "_pose"), _pose_args(pose, fov_v, V)


def march_fwd(vol, tf, cam, entry, exit_, rays, n, max_samples, sampling_rate, mode=N.DR_MODE_DIFF,
              variant=N.DR_VARIANT_AUTO, want_steps=True, fov_deg=30.0, near=0.1, workspace="auto", rows=None,
              hints="auto", tape=False, pose=None, fov_v=None):
    """raycast + get_final_image (VR.py:261-306,363-372) or the nondiff pair (VR.py:308-361).
    Returns out (views,W,H,4) and steps (views,W,H) int32 (or None).
    workspace: a buffer from alloc_workspace() (keep it for march_bwd), "auto" to allocate a throw-away one,
    or None to force the baseline kernels.
    hints: "auto" (DR_HINT_* from the TF's largest alpha once it is known, see _TerminationHints), 0 / None, or explicit bits.
    tape: DR_TAPE_TF -- the caller will ask for the TF gradient only (march_bwd(want_vol=False, tape=True)); the workspace must come
    from alloc_workspace(..., tape=(max_samples, sampling_rate)). Differentiable mode only; same image.
    pose, fov_v: those of ray_setup_pose when the buffers come from it (cam: the pose's look_from, pose[:, :3]) -- the fast
    kernels' brick geometry follows the camera's basis (dr_march_fwd_rows_pose); None: the fixed camera, as ever."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    dev = vol.device
    out, steps = _fwd_buffers(V, W, H, dev, want_steps)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    if isinstance(workspace, str):
        workspace = alloc_workspace(V, (W, H), vargs[2:5], targs[1], dev) if variant == N.DR_VARIANT_AUTO else None
    if isinstance(hints, str):
        hints = _hints.hints(tf, vargs[2:5], sampling_rate, max_samples, mode) if variant == N.DR_VARIANT_AUTO else 0
    entry_point, pargs = _pose_entry("dr_march_fwd_rows", pose, fov_v, V)
    with torch.cuda.device(dev):
        rc = entry_point(*vargs, *targs, *rargs, int(max_samples), float(sampling_rate),
                         float(np.radians(fov_deg)), float(near), int(mode),
                         int(variant) | int(hints or 0) | (N.DR_TAPE_TF if tape else 0), out.data_ptr(),
                         _ptr(steps), *_ws_args(workspace), *_rows(rows, W), *pargs[2:], _stream())
    N.check(rc, "dr_march_fwd_rows" if pose is None else "dr_march_fwd_rows_pose")
    return out, steps


def _d_vol(vol, want):
    """The backward's d_volume (zeros, float32, vol's layout) and its C-ABI arguments (pointer, x/y/z strides, view stride);
    (None, (None, 0, 0, 0, 0)) when not wanted."""
    if not want:
        return None, (None, 0, 0, 0, 0)
    d_vol = torch.zeros_like(vol, dtype=torch.float32, memory_format=torch.preserve_format)
    if vol.ndim == 3:
        return d_vol, (d_vol.data_ptr(), *d_vol.stride(), 0)
    return d_vol, (d_vol.data_ptr(), *d_vol.stride()[1:], d_vol.stride(0))


def _d_tf(tf, want, batched_ndim):
    """A plain backward's d_tf (zeros like the table, whose rank is batched_ndim when every view has its own) and its C-ABI
    arguments (pointer, view stride); (None, (None, 0)) when not wanted."""
    if not want:
        return None, (None, 0)
    d_tf = torch.zeros_like(tf)
    return d_tf, (d_tf.data_ptr(), d_tf.stride(0) if tf.ndim == batched_ndim else 0)


def march_bwd(vol, tf, cam, entry, exit_, rays, n, max_samples, sampling_rate, grad_out, out, want_vol=True,
              want_tf=True, variant=N.DR_VARIANT_AUTO, fov_deg=30.0, near=0.1, workspace=None, rows=None, count_evaluated=False,
              tape=False, pose=None, fov_v=None):
    """Adjoint of the differentiable march w.r.t. vol and tf (replaces raycast.grad, VR.py:460-461,470-471).
    Shared (un-batched) vol / tf receive one gradient accumulated over all views.
    workspace: the buffer the matching march_fwd filled (fast path); None runs the baseline kernels.
    count_evaluated: measurement only (DR_COUNT_EVALUATED; see evaluated_samples()).
    tape: the forward was run with tape=True and only d_tf is wanted: the per-ray pass over the tape (csrc/tf_tape.hip).
    pose, fov_v: those the forward was given."""
    if tape and want_vol:
        raise ValueError("tape=True serves the backward w.r.t. the transfer function alone (want_vol=False)")
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf = None
    dt = (None, 0)
    if want_tf:
        d_tf = torch.zeros_like(tf)
        dt = (d_tf.data_ptr(), d_tf.stride(0) if tf.ndim == 3 else 0)
    if not (want_vol or want_tf):
        return None, None
    entry_point, pargs = _pose_entry("dr_march_bwd_rows", pose, fov_v, V)
    with torch.cuda.device(vol.device):
        rc = entry_point(*vargs, *targs, *rargs, int(max_samples), float(sampling_rate),
                         float(np.radians(fov_deg)), float(near),
                         int(variant) | (N.DR_COUNT_EVALUATED if count_evaluated else 0) | (N.DR_TAPE_TF if tape else 0),
                         grad_out.data_ptr(), out.data_ptr(), *dv, *dt, *_ws_args(workspace),
                         *_rows(rows, W), *pargs[2:], _stream())
    N.check(rc, "dr_march_bwd_rows" if pose is None else "dr_march_bwd_rows_pose")
    return d_vol, d_tf


def march_bwd_pose(vol, tf, pose, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                   near=0.1, jitter_seed=0, view_base=0, rows=None, per_ray=False, fov_v=None):
    """Gradient of the differentiable march w.r.t. the pose (views, 9) and the field of view (dr_march_bwd_pose):
    march_bwd_cam for the free camera of ray_setup_pose, whose buffers, pose and fov_v these are. Returns d_pose (views, 10)
    float32 -- d look_from, d look_at, d up, d fov PER RADIAN (of fov_v's entries, or of fov_deg's angle when fov_v is None) --
    and, with per_ray=True, each ray's contribution (views, W, H, 10) as well."""
    return march_bwd_cam(vol, tf, pose[:, :3], entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg,
                         near, jitter_seed, view_base, rows, per_ray, pose=pose, fov_v=fov_v)


def march_bwd_cam(vol, tf, cam, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                  near=0.1, jitter_seed=0, view_base=0, rows=None, per_ray=False, pose=None, fov_v=None):
    """Gradient of the differentiable march w.r.t. the camera positions `cam` (views, 3) (dr_march_bwd_cam; the
    reference has none, VR.py:465). The ray buffers, `steps`, `out`, jitter_seed, view_base and rows are those of the forward
    (ray_setup + march_fwd). Returns d_cam (views, 3) float32 -- and, with per_ray=True, each ray's contribution
    (views, W, H, 3) float32 as well."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    head = (*_vol_args(vol, V), *_tf_args(tf, V), *rargs, int(max_samples), float(sampling_rate))
    return _camera_bwd("dr_march_bwd", vol, n, head, (fov_deg, near, jitter_seed, view_base),
                       (steps.data_ptr(), grad_out.data_ptr(), out.data_ptr()), per_ray, pose, fov_v, rows)


def _camera_bwd(name, vol, n, head_args, camera, image_args, per_ray, pose, fov_v, rows=False):
    """The end of every camera backward: the entry `name`_cam (d look_from, k = 3 columns) or, with a pose, `name`_pose (d pose
    and d fov, k = 10) -- the one place that chooses between them. The C-ABI arguments are the family's head_args, then camera =
    (fov_deg, near, jitter_seed, view_base), the image band of `rows` (march_bwd_cam's; False: the entry takes none; checked
    behind the pose, as it always was), the family's image_args, the pose pointers, d_cam (views, k) and the per-ray d_ray
    (views, W, H, k). The caller keeps its temporaries until this returns. -> _cam_grad_result."""
    V, W, H = n.shape
    fov_deg, near, jitter_seed, view_base = camera
    d_cam, d_ray = _cam_grad_buffers(V, W, H, vol.device, per_ray, 3 if pose is None else 10)
    pargs = () if pose is None else _pose_args(pose, fov_v, V)
    _call(name + ("_cam" if pose is None else "_pose"), vol.device, *head_args, float(np.radians(fov_deg)), float(near),
          int(jitter_seed) & 0xFFFFFFFF, int(view_base), *(() if rows is False else _rows(rows, W)), *image_args, *pargs[2:],
          d_cam.data_ptr(), _ptr(d_ray))
    return _cam_grad_result(d_cam, d_ray)


def _tf2d_args(tf2d, n_views):
    if tf2d.dtype != torch.float32 or not tf2d.is_contiguous():
        raise TypeError("tf2d must be a contiguous float32 tensor")
    if tf2d.ndim == 3 and tf2d.shape[2] == 4:
        return tf2d.data_ptr(), tf2d.shape[0], tf2d.shape[1], 0
    if tf2d.ndim == 4 and tf2d.shape[3] == 4 and tf2d.shape[0] == n_views:
        return tf2d.data_ptr(), tf2d.shape[1], tf2d.shape[2], tf2d.stride(0)
    raise ValueError("tf2d must be (RV,RG,4) or (views,RV,RG,4)")


def _g_scale(g_scale):
    g = float(g_scale)
    if not (math.isfinite(g) and g > 0.0):
        raise ValueError(f"g_scale must be finite and > 0, got {g_scale}")
    return g


def march_tf2d_fwd(vol, tf2d, cam, entry, exit_, rays, n, max_samples, sampling_rate, g_scale, mode=N.DR_MODE_DIFF,
                   want_steps=True):
    """The march with a 2-D (value, gradient-magnitude) transfer function (dr_march_tf2d_fwd): march_fwd with the
    classification rgba = T[I (RV-1), u (RG-1)] (bilinear, value axis first), u = |central-difference taps| * g_scale.
    tf2d: (RV, RG, 4) shared or (views, RV, RG, 4) float32 contiguous. Returns out (views,W,H,4) and steps (views,W,H) int32
    (or None). A (RV, 1) table gives march_fwd's bits with the 1-D TF of RV entries."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    out, steps = _fwd_buffers(V, W, H, vol.device, want_steps)
    vargs = _vol_args(vol, V)
    targs = _tf2d_args(tf2d, V)
    _call("dr_march_tf2d_fwd", vol.device, *vargs, *targs, _g_scale(g_scale), *rargs, int(max_samples), float(sampling_rate),
          int(mode), out.data_ptr(), _ptr(steps))
    return out, steps


def march_tf2d_bwd(vol, tf2d, cam, entry, exit_, rays, n, max_samples, sampling_rate, g_scale, grad_out, out, want_vol=True,
                   want_tf=True):
    """Adjoint of the differentiable march_tf2d_fwd w.r.t. vol and tf2d (dr_march_tf2d_bwd). Returns (d_vol, d_tf2d), either
    None when not wanted; a shared (un-batched) vol / tf2d receives one gradient accumulated over all views. NaN propagates (the
    plain kernels' convention: the caller applies nan_to_num, as tf2d.Raycaster2D does)."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    vargs = _vol_args(vol, V)
    targs = _tf2d_args(tf2d, V)
    g = _g_scale(g_scale)
    if not (want_vol or want_tf):
        return None, None
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf, dt = _d_tf(tf2d, want_tf, 4)
    _call("dr_march_tf2d_bwd", vol.device, *vargs, *targs, g, *rargs, int(max_samples), float(sampling_rate), grad_out.data_ptr(),
          out.data_ptr(), *dv, *dt)
    return d_vol, d_tf


def default_light(cam):
    """The reference's lighting (VR.py:91-95, 281-299) as the (views, 10) rows march_lit_fwd reads, for the cameras cam
    (views, 3): a white light at look_from + (0, 1, 0) formed in float32, ambient 0.4, diffuse 0.8, specular 0.3, shininess 32."""
    cam = cam.to(torch.float32).reshape(-1, 3)
    light = cam.new_empty((cam.shape[0], 10))
    light[:, :3] = cam + cam.new_tensor([0.0, 1.0, 0.0])
    light[:, 3:] = cam.new_tensor([1.0, 1.0, 1.0, 0.4, 0.8, 0.3, 32.0])
    return light


def _light_arg(light, n_views, device):
    """light (views, 10) as the float32 contiguous device tensor the kernels read (kept by the caller until its call is issued)."""
    if not torch.is_tensor(light) or light.ndim != 2 or tuple(light.shape) != (n_views, 10):
        raise ValueError(f"light must be a (views, 10) tensor with views = {n_views}: position, colour, ambient, diffuse, "
                         "specular, shininess")
    _require_gpu(light, "light")
    return light.to(device=device, dtype=torch.float32).contiguous()


def march_lit_fwd(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, mode=N.DR_MODE_DIFF, want_steps=True):
    """The 1-D TF march with a free light and Phong material (dr_march_lit_fwd): the plain kernels' march_fwd with
    light (views, 10) float32 = the light's WORLD position (3), its colour (3), ambient, diffuse, specular, shininess per view.
    Returns out (views,W,H,4) and steps (views,W,H) int32 (or None). default_light(cam) gives the bits of
    march_fwd(variant=DR_VARIANT_BASELINE)."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    out, steps = _fwd_buffers(V, W, H, vol.device, want_steps)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    light = _light_arg(light, V, vol.device)
    _call("dr_march_lit_fwd", vol.device, *vargs, *targs, *rargs, int(max_samples), float(sampling_rate), light.data_ptr(), int(mode),
          out.data_ptr(), _ptr(steps))
    return out, steps


def march_lit_bwd(vol, tf, cam, light, entry, exit_, rays, n, max_samples, sampling_rate, grad_out, out, want_vol=True,
                  want_tf=True, want_light=True, per_ray=False):
    """Adjoint of the differentiable march_lit_fwd w.r.t. vol, tf and light (dr_march_lit_bwd). Returns (d_vol, d_tf, d_light),
    each None when not wanted -- d_light (views, 10) float32 in light's order -- and, with per_ray=True, a fourth result: each
    ray's contribution to d_light, (views, W, H, 10) float32. A shared (un-batched) vol / tf receives one gradient accumulated
    over all views. NaN propagates into d_vol and d_tf (the plain kernels' convention: the caller applies nan_to_num, as
    lighting.RaycasterLit does); a NaN ray contributes nothing to d_light (D5)."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    light = _light_arg(light, V, vol.device)
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf, dt = _d_tf(tf, want_tf, 3)
    d_light = torch.zeros((V, 10), dtype=torch.float64, device=vol.device) if want_light else None
    d_ray = torch.empty((V, W, H, 10), dtype=torch.float32, device=vol.device) if per_ray else None
    if want_vol or want_tf or want_light or per_ray:
        _call("dr_march_lit_bwd", vol.device, *vargs, *targs, *rargs, int(max_samples), float(sampling_rate), light.data_ptr(),
              N.DR_MODE_DIFF, grad_out.data_ptr(), out.data_ptr(), *dv, *dt, _ptr(d_light), _ptr(d_ray))
    if d_light is not None:
        d_light = torch.nan_to_num(d_light.float())   # D5: a sum beyond the float range saturates
    return (d_vol, d_tf, d_light, d_ray) if per_ray else (d_vol, d_tf, d_light)


def _vol4_args(vol4, n_views):
    """-> (ptr, dtype_tag, VX, VY, VZ, sx, sy, sz, sc, view_stride) of an RGBA volume ([views,] 4, VX, VY, VZ), any strides"""
    tag = _dtype_tag(vol4, "RGBA volume dtype must be float32 or float16")
    if vol4.ndim not in (4, 5) or vol4.shape[-4] != 4:
        raise ValueError(f"RGBA volume must be (4,VX,VY,VZ) or (views,4,VX,VY,VZ), got {tuple(vol4.shape)}")
    if vol4.ndim == 5 and vol4.shape[0] != n_views:
        raise ValueError(f"batched RGBA volume has {vol4.shape[0]} items, expected {n_views}")
    sc, sx, sy, sz = vol4.stride()[-4:]
    return (vol4.data_ptr(), tag, *(int(v) for v in vol4.shape[-3:]), sx, sy, sz, sc, vol4.stride(0) if vol4.ndim == 5 else 0)


def march_rgba_fwd(vol4, cam, entry, exit_, rays, n, max_samples, sampling_rate, mode=N.DR_MODE_DIFF, want_steps=True):
    """The march through a pre-classified RGBA volume (dr_march_rgba_fwd): every sample is the trilinear
    interpolation of the volume's four channels, composited with its opacity 1 - (1 - a)^(1/sampling_rate): no transfer function,
    no shading. vol4: (4, VX, VY, VZ) shared or (views, 4, VX, VY, VZ), float32 or float16, any strides, never copied (with the
    channel axis at stride 1 -- rgba.interleaved() -- a voxel is one load). Returns out (views,W,H,4) and steps (views,W,H) int32
    (or None)."""
    cam, V, W, H, rargs = _ray_args(vol4, cam, entry, exit_, rays, n)
    vargs = _vol4_args(vol4, V)
    out, steps = _fwd_buffers(V, W, H, vol4.device, want_steps)
    _call("dr_march_rgba_fwd", vol4.device, *vargs, *rargs, int(max_samples), float(sampling_rate), int(mode), out.data_ptr(),
          _ptr(steps))
    return out, steps


def march_rgba_bwd(vol4, cam, entry, exit_, rays, n, max_samples, sampling_rate, grad_out, out):
    """d_vol of sum(march_rgba_fwd(...) * grad_out) (dr_march_rgba_bwd): float32, in vol4's own layout; a shared (un-batched)
    volume receives one gradient summed over the views. NaN propagates (the plain kernels' convention: the caller applies
    nan_to_num, as rgba.RaycasterRGBA does)."""
    cam, V, W, H, rargs = _ray_args(vol4, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    vargs = _vol4_args(vol4, V)
    d_vol = torch.zeros_like(vol4, dtype=torch.float32, memory_format=torch.preserve_format)
    dc, dx, dy, dz = d_vol.stride()[-4:]
    _call("dr_march_rgba_bwd", vol4.device, *vargs, *rargs, int(max_samples), float(sampling_rate), grad_out.data_ptr(),
          out.data_ptr(), d_vol.data_ptr(), dx, dy, dz, dc, d_vol.stride(0) if d_vol.ndim == 5 else 0)
    return d_vol


def march_rgba_bwd_pose(vol4, pose, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                        near=0.1, jitter_seed=0, view_base=0, per_ray=False, fov_v=None):
    """d pose of sum(march_rgba_fwd(...) * grad_out) (dr_march_rgba_bwd_pose): march_rgba_bwd_cam for the free
    camera of ray_setup_pose, as march_bwd_pose is march_bwd_cam's. Returns d_pose (views, 10) float32 (the fov column per
    radian) -- and, with per_ray=True, each ray's contribution (views, W, H, 10) as well."""
    return march_rgba_bwd_cam(vol4, pose[:, :3], entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg,
                              near, jitter_seed, view_base, per_ray, pose=pose, fov_v=fov_v)


def march_rgba_bwd_cam(vol4, cam, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                       near=0.1, jitter_seed=0, view_base=0, per_ray=False, pose=None, fov_v=None):
    """d look_from of sum(march_rgba_fwd(...) * grad_out) (dr_march_rgba_bwd_cam): cam (views, 3), the ray
    buffers, jitter_seed and view_base those of the forward's ray_setup, `steps` and `out` those of march_rgba_fwd. Returns
    d_cam (views, 3) float32 -- and, with per_ray=True, each ray's contribution (views, W, H, 3) as well."""
    cam, V, W, H, rargs = _ray_args(vol4, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    head = (*_vol4_args(vol4, V), *rargs, int(max_samples), float(sampling_rate))
    return _camera_bwd("dr_march_rgba_bwd", vol4, n, head, (fov_deg, near, jitter_seed, view_base),
                       (steps.data_ptr(), grad_out.data_ptr(), out.data_ptr()), per_ray, pose, fov_v)


def march_depth_fwd(vol, tf, cam, entry, exit_, rays, n, max_samples, sampling_rate, want_steps=True):
    """The ray-depth moments of the differentiable march (dr_march_depth_fwd): march_fwd's samples, classified by
    the table's alpha alone (one tap, no shading), compositing the sample's distance t from look_from and its square. Returns
    out (views,W,H,4) = (M1, M2, 0, A) -- A and steps the bits of march_fwd(variant=DR_VARIANT_BASELINE) -- and steps (views,W,H)
    int32 (or None)."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    out, steps = _fwd_buffers(V, W, H, vol.device, want_steps)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    _call("dr_march_depth_fwd", vol.device, *vargs, *targs, *rargs, int(max_samples), float(sampling_rate), out.data_ptr(),
          _ptr(steps))
    return out, steps


def march_depth_bwd(vol, tf, cam, entry, exit_, rays, n, max_samples, sampling_rate, grad_out, out, want_vol=True, want_tf=True):
    """Adjoint of march_depth_fwd w.r.t. vol and tf (dr_march_depth_bwd). Returns (d_vol, d_tf), either None when not wanted; a
    shared (un-batched) vol / tf receives one gradient accumulated over all views. Only the alpha column of d_tf is non-zero.
    Channel 2 of grad_out is not used. NaN propagates (the plain kernels' convention: the caller applies nan_to_num, as
    depth.DepthRaycaster does)."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    vargs = _vol_args(vol, V)
    targs = _tf_args(tf, V)
    if not (want_vol or want_tf):
        return None, None
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf, dt = _d_tf(tf, want_tf, 3)
    _call("dr_march_depth_bwd", vol.device, *vargs, *targs, *rargs, int(max_samples), float(sampling_rate), grad_out.data_ptr(),
          out.data_ptr(), *dv, *dt)
    return d_vol, d_tf


def march_depth_bwd_pose(vol, tf, pose, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                         near=0.1, jitter_seed=0, view_base=0, per_ray=False, fov_v=None):
    """d pose of sum(march_depth_fwd(...) * grad_out) (dr_march_depth_bwd_pose): march_depth_bwd_cam for the free
    camera of ray_setup_pose, as march_bwd_pose is march_bwd_cam's. Returns d_pose (views, 10) float32 (the fov column per
    radian) -- and, with per_ray=True, each ray's contribution (views, W, H, 10) as well."""
    return march_depth_bwd_cam(vol, tf, pose[:, :3], entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out,
                               fov_deg, near, jitter_seed, view_base, per_ray, pose=pose, fov_v=fov_v)


def march_depth_bwd_cam(vol, tf, cam, entry, exit_, rays, n, steps, max_samples, sampling_rate, grad_out, out, fov_deg=30.0,
                        near=0.1, jitter_seed=0, view_base=0, per_ray=False, pose=None, fov_v=None):
    """d look_from of sum(march_depth_fwd(...) * grad_out) (dr_march_depth_bwd_cam): cam (views, 3), the ray
    buffers, jitter_seed and view_base those of the forward's ray_setup, `steps` and `out` those of march_depth_fwd. Returns
    d_cam (views, 3) float32 -- and, with per_ray=True, each ray's contribution (views, W, H, 3) as well."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    head = (*_vol_args(vol, V), *_tf_args(tf, V), *rargs, int(max_samples), float(sampling_rate))
    return _camera_bwd("dr_march_depth_bwd", vol, n, head, (fov_deg, near, jitter_seed, view_base),
                       (steps.data_ptr(), grad_out.data_ptr(), out.data_ptr()), per_ray, pose, fov_v)


def _t_near(t_near):
    """t_near as the C ABI takes it: None = off (-inf)."""
    return -math.inf if t_near is None else float(t_near)


def _bundle_rays(origins, dirs):
    """A bundle's origins and directions (N, 3) as the float32 contiguous tensors the kernels read -> (origins, dirs, N). The
    caller keeps them until its call has been issued."""
    _require_gpu(origins, "origins")
    _require_gpu(dirs, "directions")
    if origins.ndim != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape or origins.shape[0] < 1:
        raise ValueError(f"origins and directions must both be (N, 3) with N >= 1, got {tuple(origins.shape)} and "
                         f"{tuple(dirs.shape)}")
    if origins.device != dirs.device:
        raise ValueError(f"origins and directions live on different devices: {origins.device}, {dirs.device}")
    return origins.to(torch.float32).contiguous(), dirs.to(torch.float32).contiguous(), int(origins.shape[0])


def bundle_setup(origins, dirs, vol_shape, sampling_rate, t_near=None, jitter_seed=0, ray_base=0):
    """ray_setup for a bundle of rays (dr_bundle_setup): origins, dirs (N, 3) in look_from's world coordinates,
    the directions of unit length and used as given -> entry, exit (N,) float32 and n (N,) int32. For the origin and direction
    of a ray_setup pixel these are that pixel's, bit for bit. t_near: None marches the reference's whole line through the box
    (also behind an origin inside it); a number clamps the entry distance from below before the hit test and the sample count
    (0: a ray). jitter_seed != 0 draws ray p's offset from (jitter_seed, ray_base, p)."""
    origins, dirs, n_rays = _bundle_rays(origins, dirs)
    dev = origins.device
    entry = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    exit_ = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    n = torch.empty((n_rays,), dtype=torch.int32, device=dev)
    VX, VY, VZ = (int(s) for s in vol_shape)
    _call("dr_bundle_setup", dev, origins.data_ptr(), dirs.data_ptr(), n_rays, VX, VY, VZ, float(sampling_rate), _t_near(t_near),
          int(jitter_seed) & 0xFFFFFFFF, int(ray_base) & 0xFFFFFFFF, entry.data_ptr(), exit_.data_ptr(), n.data_ptr())
    return entry, exit_, n


def _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate):
    """What the three bundle marches start with -> (origins, dirs, N, their C-ABI arguments up to sampling_rate): one volume
    (VX, VY, VZ) with any strides and one table (R, 4)."""
    _require_gpu(vol, "volume")
    origins, dirs, n_rays = _bundle_rays(origins, dirs)
    if vol.ndim != 3 or tf.ndim != 2:
        raise ValueError("a bundle is marched through one volume (VX,VY,VZ) and one table (R,4)")
    for name, t in (("entry", entry), ("exit", exit_), ("n", n)):
        if tuple(t.shape) != (n_rays,) or not t.is_contiguous():
            raise ValueError(f"{name} must be bundle_setup's contiguous ({n_rays},) buffer, got {tuple(t.shape)}")
    vargs, targs = _vol_args(vol, 1), _tf_args(tf, 1)
    return origins, dirs, n_rays, (*vargs[:8], *targs[:2], origins.data_ptr(), dirs.data_ptr(), entry.data_ptr(), exit_.data_ptr(),
                                   n.data_ptr(), n_rays, int(max_samples), float(sampling_rate))


def march_bundle_fwd(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate, want_steps=True):
    """The differentiable march of a bundle's rays (dr_march_bundle_fwd): march_fwd's DR_MODE_DIFF samples with
    the ray's origin in the camera's place and the light at origin + (0, 1, 0). Returns out (N, 4) and steps (N,) int32 (or
    None): for a pinhole view's rays, the bits of march_fwd(variant=DR_VARIANT_BASELINE)."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    out = torch.empty((n_rays, 4), dtype=torch.float32, device=vol.device)
    steps = torch.empty((n_rays,), dtype=torch.int32, device=vol.device) if want_steps else None
    _call("dr_march_bundle_fwd", vol.device, *head, out.data_ptr(), _ptr(steps))
    return out, steps


def march_bundle_bwd(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate, grad_out, out, want_vol=True,
                     want_tf=True):
    """Adjoint of march_bundle_fwd w.r.t. vol and tf (dr_march_bundle_bwd). Returns (d_vol, d_tf), either None when not wanted.
    NaN propagates (the plain kernels' convention: the caller applies nan_to_num, as bundle.RayBundleRaycaster does)."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    if not (want_vol or want_tf):
        return None, None
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf, dt = _d_tf(tf, want_tf, 3)
    _call("dr_march_bundle_bwd", vol.device, *head, grad_out.data_ptr(), out.data_ptr(), *dv[:4], dt[0])
    return d_vol, d_tf


def march_bundle_bwd_rays(vol, tf, origins, dirs, entry, exit_, n, steps, max_samples, sampling_rate, grad_out, out, t_near=None,
                          jitter_seed=0, ray_base=0):
    """Gradient of march_bundle_fwd w.r.t. every ray's origin and direction (dr_march_bundle_bwd_rays): the
    buffers, t_near, jitter_seed and ray_base those of bundle_setup, `steps` and `out` those of march_bundle_fwd. Returns
    d_origins, d_dirs (N, 3) float32 -- d_dirs w.r.t. the direction as a free 3-vector. A NaN ray gets zeros (D5)."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    d_origins = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    d_dirs = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    _call("dr_march_bundle_bwd_rays", vol.device, *head, steps.data_ptr(), _t_near(t_near), int(jitter_seed) & 0xFFFFFFFF,
          int(ray_base) & 0xFFFFFFFF, grad_out.data_ptr(), out.data_ptr(), d_origins.data_ptr(), d_dirs.data_ptr())
    return d_origins, d_dirs


def march_depth_bundle_fwd(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate, want_steps=True):
    """The ray-depth moments of a bundle's rays (dr_march_depth_bundle_fwd): march_depth_fwd's samples with the
    ray's origin in the camera's place. Returns out (N, 4) = (M1, M2, 0, A), the distances measured from each ray's origin along
    its unit direction, and steps (N,) int32 (or None): for a pinhole view's rays the bits of march_depth_fwd, and on any
    bundle A and steps are march_bundle_fwd's."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    out = torch.empty((n_rays, 4), dtype=torch.float32, device=vol.device)
    steps = torch.empty((n_rays,), dtype=torch.int32, device=vol.device) if want_steps else None
    _call("dr_march_depth_bundle_fwd", vol.device, *head, out.data_ptr(), _ptr(steps))
    return out, steps


def march_depth_bundle_bwd(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate, grad_out, out, want_vol=True,
                           want_tf=True):
    """Adjoint of march_depth_bundle_fwd w.r.t. vol and tf (dr_march_depth_bundle_bwd). Returns (d_vol, d_tf), either None when
    not wanted. Only the alpha column of d_tf is non-zero; channel 2 of grad_out is not used. NaN propagates (the plain kernels'
    convention: the caller applies nan_to_num, as depth.RayBundleDepthRaycaster does)."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    if not (want_vol or want_tf):
        return None, None
    d_vol, dv = _d_vol(vol, want_vol)
    d_tf, dt = _d_tf(tf, want_tf, 3)
    _call("dr_march_depth_bundle_bwd", vol.device, *head, grad_out.data_ptr(), out.data_ptr(), *dv[:4], dt[0])
    return d_vol, d_tf


def march_depth_bundle_bwd_rays(vol, tf, origins, dirs, entry, exit_, n, steps, max_samples, sampling_rate, grad_out, out,
                                t_near=None, jitter_seed=0, ray_base=0):
    """Gradient of march_depth_bundle_fwd w.r.t. every ray's origin and direction (dr_march_depth_bundle_bwd_rays, DESIGN.md
    D22): the buffers, t_near, jitter_seed and ray_base those of bundle_setup, `steps` and `out` those of march_depth_bundle_fwd.
    Returns d_origins, d_dirs (N, 3) float32 -- d_dirs w.r.t. the direction as a free 3-vector with the sample distances the
    march's own parameter (no radial term). A NaN ray gets zeros (D5)."""
    origins, dirs, n_rays, head = _bundle_head(vol, tf, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    d_origins = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    d_dirs = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    _call("dr_march_depth_bundle_bwd_rays", vol.device, *head, steps.data_ptr(), _t_near(t_near), int(jitter_seed) & 0xFFFFFFFF,
          int(ray_base) & 0xFFFFFFFF, grad_out.data_ptr(), out.data_ptr(), d_origins.data_ptr(), d_dirs.data_ptr())
    return d_origins, d_dirs


def _rgba_bundle_head(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate):
    """What the three RGBA bundle marches start with -> (origins, dirs, N, their C-ABI arguments up to sampling_rate): one RGBA
    volume (4, VX, VY, VZ), float32 or float16, with any strides."""
    _require_gpu(vol4, "volume")
    origins, dirs, n_rays = _bundle_rays(origins, dirs)
    if vol4.ndim != 4:
        raise ValueError(f"a bundle is marched through one RGBA volume (4,VX,VY,VZ), got {tuple(vol4.shape)}")
    for name, t in (("entry", entry), ("exit", exit_), ("n", n)):
        if tuple(t.shape) != (n_rays,) or not t.is_contiguous():
            raise ValueError(f"{name} must be bundle_setup's contiguous ({n_rays},) buffer, got {tuple(t.shape)}")
    return origins, dirs, n_rays, (*_vol4_args(vol4, 1)[:9], origins.data_ptr(), dirs.data_ptr(), entry.data_ptr(),
                                   exit_.data_ptr(), n.data_ptr(), n_rays, int(max_samples), float(sampling_rate))


def march_rgba_bundle_fwd(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate, want_steps=True):
    """The differentiable RGBA march of a bundle's rays (dr_march_rgba_bundle_fwd): march_rgba_fwd's DR_MODE_DIFF
    samples with the ray's origin in the camera's place; origins, dirs (N, 3) and the buffers of bundle_setup. Returns out (N, 4)
    and steps (N,) int32 (or None): for a pinhole view's rays, the bits of march_rgba_fwd."""
    origins, dirs, n_rays, head = _rgba_bundle_head(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    out = torch.empty((n_rays, 4), dtype=torch.float32, device=vol4.device)
    steps = torch.empty((n_rays,), dtype=torch.int32, device=vol4.device) if want_steps else None
    _call("dr_march_rgba_bundle_fwd", vol4.device, *head, out.data_ptr(), _ptr(steps))
    return out, steps


def march_rgba_bundle_bwd(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate, grad_out, out, d_vol=None):
    """d_vol of sum(march_rgba_bundle_fwd(...) * grad_out) (dr_march_rgba_bundle_bwd): float32, in vol4's own layout -- or
    accumulated into `d_vol`, a float32 tensor of vol4's shape with any strides, which is then returned. NaN propagates (the
    plain kernels' convention: the caller applies nan_to_num, as rgba.RayBundleRaycasterRGBA does)."""
    origins, dirs, n_rays, head = _rgba_bundle_head(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    if d_vol is None:
        d_vol = torch.zeros_like(vol4, dtype=torch.float32, memory_format=torch.preserve_format)
    elif d_vol.dtype != torch.float32 or d_vol.shape != vol4.shape or d_vol.device != vol4.device:
        raise ValueError(f"d_vol must be a float32 tensor of the volume's shape {tuple(vol4.shape)} on its device")
    dc, dx, dy, dz = d_vol.stride()
    _call("dr_march_rgba_bundle_bwd", vol4.device, *head, grad_out.data_ptr(), out.data_ptr(), d_vol.data_ptr(), dx, dy, dz, dc)
    return d_vol


def march_rgba_bundle_bwd_rays(vol4, origins, dirs, entry, exit_, n, steps, max_samples, sampling_rate, grad_out, out, t_near=None,
                               jitter_seed=0, ray_base=0):
    """Gradient of march_rgba_bundle_fwd w.r.t. every ray's origin and direction (dr_march_rgba_bundle_bwd_rays):
    the buffers, t_near, jitter_seed and ray_base those of bundle_setup, `steps` and `out` those of march_rgba_bundle_fwd.
    Returns d_origins, d_dirs (N, 3) float32 -- d_dirs w.r.t. the direction as a free 3-vector. A NaN ray gets zeros (D5)."""
    origins, dirs, n_rays, head = _rgba_bundle_head(vol4, origins, dirs, entry, exit_, n, max_samples, sampling_rate)
    grad_out, out = _bwd_images(grad_out, out)
    steps = steps.to(torch.int32).contiguous()
    d_origins = torch.empty((n_rays, 3), dtype=torch.float32, device=vol4.device)
    d_dirs = torch.empty((n_rays, 3), dtype=torch.float32, device=vol4.device)
    _call("dr_march_rgba_bundle_bwd_rays", vol4.device, *head, steps.data_ptr(), _t_near(t_near), int(jitter_seed) & 0xFFFFFFFF,
          int(ray_base) & 0xFFFFFFFF, grad_out.data_ptr(), out.data_ptr(), d_origins.data_ptr(), d_dirs.data_ptr())
    return d_origins, d_dirs


_PROJ_MODES = {"sum": N.DR_PROJ_SUM, "max": N.DR_PROJ_MAX}
NO_SAMPLE_LIMIT = 2 ** 31 - 1   # a max_samples no ray reaches


def _proj_mode(mode):
    if mode in _PROJ_MODES:
        return _PROJ_MODES[mode]
    if mode in _PROJ_MODES.values():
        return int(mode)
    raise ValueError(f"projection mode must be 'sum' or 'max', got {mode!r}")


def _max_samples(max_samples):
    return NO_SAMPLE_LIMIT if max_samples is None else int(max_samples)


def _proj_bwd_args(max_samples, mode, arg_max):
    """What both projection backwards make of their options -> (arg_max as the int32 contiguous tensor the kernels read, or
    None; the C-ABI arguments max_samples, mode)."""
    md = _proj_mode(mode)
    if md == N.DR_PROJ_MAX and arg_max is None:
        raise ValueError("mode 'max' needs the forward's arg_max")
    arg = arg_max.to(torch.int32).contiguous() if arg_max is not None else None
    return arg, (_max_samples(max_samples), md)


def project_fwd(vol, cam, entry, exit_, rays, n, max_samples=None, mode="sum"):
    """X-ray line integral (mode "sum": D * sum of the trilinear samples, D = (exit - entry) / n) or maximum intensity projection
    ("max") of vol along the rays of ray_setup (dr_project_fwd). Returns out (views, W, H) float32 and, for "max",
    arg_max (views, W, H) int32, the index of the first maximal sample (-1: none) -- None for "sum". max_samples None: no limit."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    dev = vol.device
    md = _proj_mode(mode)
    out = torch.empty((V, W, H), dtype=torch.float32, device=dev)
    arg = torch.empty((V, W, H), dtype=torch.int32, device=dev) if md == N.DR_PROJ_MAX else None
    vargs = _vol_args(vol, V)
    _call("dr_project_fwd", dev, *vargs, *rargs, _max_samples(max_samples), md, out.data_ptr(), _ptr(arg))
    return out, arg


def project_bwd(vol, cam, entry, exit_, rays, n, grad_out, max_samples=None, mode="sum", arg_max=None,
                variant=N.DR_VARIANT_AUTO):
    """d_vol of sum(project_fwd(...) * grad_out) (dr_project_bwd): a back-projection. A shared (un-batched) vol receives one
    gradient summed over the views. variant DR_VARIANT_AUTO: the windowed "sum" kernel; DR_VARIANT_BASELINE: per-tap global
    atomics. "max" needs the forward's arg_max."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    arg, pargs = _proj_bwd_args(max_samples, mode, arg_max)
    grad_out = grad_out.to(torch.float32).contiguous()
    vargs = _vol_args(vol, V)
    d_vol, dv = _d_vol(vol, True)
    _call("dr_project_bwd", vol.device, *vargs, *rargs, *pargs, grad_out.data_ptr(), _ptr(arg), *dv, int(variant))
    return d_vol


def project_bwd_pose(vol, pose, entry, exit_, rays, n, grad_out, max_samples=None, mode="sum", arg_max=None, fov_deg=30.0,
                     near=0.1, jitter_seed=0, view_base=0, per_ray=False, fov_v=None):
    """d pose of sum(project_fwd(...) * grad_out) (dr_project_bwd_pose): project_bwd_cam for the free camera, as march_bwd_pose
    is march_bwd_cam's. Returns d_pose (views, 10) float32 (the fov column per radian) -- and, with per_ray=True, each ray's
    contribution (views, W, H, 10) as well."""
    return project_bwd_cam(vol, pose[:, :3], entry, exit_, rays, n, grad_out, max_samples, mode, arg_max, fov_deg, near,
                           jitter_seed, view_base, per_ray, pose=pose, fov_v=fov_v)


def project_bwd_cam(vol, cam, entry, exit_, rays, n, grad_out, max_samples=None, mode="sum", arg_max=None, fov_deg=30.0,
                    near=0.1, jitter_seed=0, view_base=0, per_ray=False, pose=None, fov_v=None):
    """d look_from of sum(project_fwd(...) * grad_out) (dr_project_bwd_cam): cam (views, 3), the ray buffers, jitter_seed and
    view_base those of the forward's ray_setup. Returns d_cam (views, 3) float32 -- and, with per_ray=True, each ray's
    contribution (views, W, H, 3) as well."""
    cam, V, W, H, rargs = _ray_args(vol, cam, entry, exit_, rays, n)
    arg, pargs = _proj_bwd_args(max_samples, mode, arg_max)
    grad_out = grad_out.to(torch.float32).contiguous()
    vargs = _vol_args(vol, V)
    return _camera_bwd("dr_project_bwd", vol, n, (*vargs, *rargs, *pargs), (fov_deg, near, jitter_seed, view_base),
                       (grad_out.data_ptr(), _ptr(arg)), per_ray, pose, fov_v)


def _proj_bundle_head(vol, origins, dirs, entry, exit_, n, max_samples, mode):
    """What the three bundle projections start with -> (origins, dirs, N, their C-ABI arguments up to mode): one volume
    (VX, VY, VZ) with any strides."""
    _require_gpu(vol, "volume")
    origins, dirs, n_rays = _bundle_rays(origins, dirs)
    if vol.ndim != 3:
        raise ValueError("a bundle is projected through one volume (VX,VY,VZ)")
    for name, t in (("entry", entry), ("exit", exit_), ("n", n)):
        if tuple(t.shape) != (n_rays,) or not t.is_contiguous():
            raise ValueError(f"{name} must be bundle_setup's contiguous ({n_rays},) buffer, got {tuple(t.shape)}")
    return origins, dirs, n_rays, (*_vol_args(vol, 1)[:8], origins.data_ptr(), dirs.data_ptr(), entry.data_ptr(), exit_.data_ptr(),
                                   n.data_ptr(), n_rays, _max_samples(max_samples), _proj_mode(mode))


def _ray_values(t, n_rays, name):
    """A per-ray vector (N,) as the float32 contiguous tensor the kernels read."""
    if tuple(t.shape) != (n_rays,):
        raise ValueError(f"{name} must be ({n_rays},), got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def project_bundle_fwd(vol, origins, dirs, entry, exit_, n, max_samples=None, mode="sum"):
    """project_fwd over a bundle of rays (dr_project_bundle_fwd): origins, dirs (N, 3) and the buffers of
    bundle_setup. Returns out (N,) float32 and, for "max", arg_max (N,) int32 -- None for "sum". For a pinhole view's rays, the
    bits of project_fwd."""
    origins, dirs, n_rays, head = _proj_bundle_head(vol, origins, dirs, entry, exit_, n, max_samples, mode)
    out = torch.empty((n_rays,), dtype=torch.float32, device=vol.device)
    arg = torch.empty((n_rays,), dtype=torch.int32, device=vol.device) if head[-1] == N.DR_PROJ_MAX else None
    _call("dr_project_bundle_fwd", vol.device, *head, out.data_ptr(), _ptr(arg))
    return out, arg


def project_bundle_bwd(vol, origins, dirs, entry, exit_, n, grad_out, max_samples=None, mode="sum", arg_max=None,
                       variant=N.DR_VARIANT_AUTO):
    """d_vol of sum(project_bundle_fwd(...) * grad_out) (dr_project_bundle_bwd): a back-projection. variant DR_VARIANT_AUTO: the
    "sum" kernel that collects the taps of 256 consecutive rays per depth window in LDS (order an image's rays with
    bundle.tile_order); DR_VARIANT_BASELINE: per-tap global atomics. "max" needs the forward's arg_max."""
    origins, dirs, n_rays, head = _proj_bundle_head(vol, origins, dirs, entry, exit_, n, max_samples, mode)
    arg, _ = _proj_bwd_args(max_samples, mode, arg_max)
    grad_out = _ray_values(grad_out, n_rays, "grad_out")
    d_vol, dv = _d_vol(vol, True)
    _call("dr_project_bundle_bwd", vol.device, *head, grad_out.data_ptr(), _ptr(arg), *dv[:4], int(variant))
    return d_vol


def project_bundle_bwd_rays(vol, origins, dirs, entry, exit_, n, grad_out, max_samples=None, mode="sum", arg_max=None,
                            t_near=None, jitter_seed=0, ray_base=0):
    """Gradient of project_bundle_fwd w.r.t. every ray's origin and direction (dr_project_bundle_bwd_rays): t_near, jitter_seed
    and ray_base those of bundle_setup. Returns d_origins, d_dirs (N, 3) float32 -- d_dirs w.r.t. the direction as a free
    3-vector. A NaN ray gets zeros (D5)."""
    origins, dirs, n_rays, head = _proj_bundle_head(vol, origins, dirs, entry, exit_, n, max_samples, mode)
    arg, _ = _proj_bwd_args(max_samples, mode, arg_max)
    grad_out = _ray_values(grad_out, n_rays, "grad_out")
    d_origins = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    d_dirs = torch.empty((n_rays, 3), dtype=torch.float32, device=vol.device)
    _call("dr_project_bundle_bwd_rays", vol.device, *head, _t_near(t_near), int(jitter_seed) & 0xFFFFFFFF,
          int(ray_base) & 0xFFFFFFFF, grad_out.data_ptr(), _ptr(arg), d_origins.data_ptr(), d_dirs.data_ptr())
    return d_origins, d_dirs


def mse_loss_grad(out, reference, inv_norm=None, want_grad=True, loss=None):
    """Image loss and its gradient in one pass over the render (dr_mse_loss_grad; replaces compute_loss,
    EX.py:368-373, and the torch mse_loss round trip of EX.py:439-443).
    Returns (loss, grad_out): loss is a 0-d float64 tensor on the device (accumulated into `loss` if given),
    grad_out has the shape of `out`. inv_norm defaults to 1/numel (= torch.nn.functional.mse_loss)."""
    _require_gpu(out, "out")
    if reference.shape != out.shape or reference.device != out.device:
        raise ValueError("reference must match out in shape and device")
    if out.dtype != torch.float32 or reference.dtype != torch.float32:
        raise TypeError("out and reference must be float32")
    out = out.contiguous()
    reference = reference.contiguous()
    if loss is None:
        loss = torch.zeros((), dtype=torch.float64, device=out.device)
    grad = torch.empty_like(out) if want_grad else None
    inv_norm = 1.0 / out.numel() if inv_norm is None else float(inv_norm)
    with torch.cuda.device(out.device):
        rc = N.lib().dr_mse_loss_grad(out.data_ptr(), reference.data_ptr(), out.numel(), inv_norm,
                                      grad.data_ptr() if want_grad else None, loss.data_ptr(), _stream())
    N.check(rc, "dr_mse_loss_grad")
    return loss, grad


def _dense(t):
    """True if t's elements occupy one dense block in some axis order (no gaps, no overlaps): a gradient with its strides can
    be written without two pixels landing on one element."""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _disjoint(t):
    """True if no two elements of t lie on one storage element, gaps allowed (a padded or sliced buffer): taken by |stride|,
    every axis steps over all that the smaller ones span. Sufficient, not necessary: interleaved layouts are turned down."""
    span = 1
    for st, sz in sorted((abs(st), sz) for st, sz in zip(t.stride(), t.shape) if sz > 1):
        if st < span:
            return False
        span += st * (sz - 1)
    return True


def _loss_inputs(out, reference):
    if out.ndim != 4 or reference.shape != out.shape:
        raise ValueError("the DSSIM + MSE loss expects two (N, C, H, W) tensors of the same shape")
    _require_gpu(out, "out")
    _require_gpu(reference, "reference")
    if reference.device != out.device:
        raise ValueError("reference must be on the device of out")
    if out.dtype != torch.float32 or reference.dtype != torch.float32:
        raise TypeError("out and reference must be float32")
    if out.stride() != reference.stride() or not _dense(out):   # one set of strides serves x, y and the gradients
        out, reference = out.contiguous(), reference.contiguous()
    return out, reference, (ctypes.c_int64 * 4)(*out.stride())


def _loss_bwd_buffers(x, stats, numel, stats_msg, upstream, middle, want_ref_grad):
    """What both loss backwards check and allocate: `stats` is the forward's (numel float64 on x's device), `upstream` three
    float32 on the device or None; returns (upstream, d out, d reference or None), the gradients with x's strides."""
    if stats.dtype != torch.float64 or stats.numel() != numel or stats.device != x.device or not stats.is_contiguous():
        raise ValueError(stats_msg)
    if upstream is not None:
        upstream = upstream.to(device=x.device, dtype=torch.float32).contiguous()
        if upstream.numel() != 3:
            raise ValueError(f"upstream holds the gradients of (loss, {middle}, mse): 3 elements")
    gx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    gy = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device) if want_ref_grad else None
    return upstream, gx, gy


def _loss_config(data_range, win_size, win_sigma, K, nonnegative_ssim):
    return (float(data_range), int(win_size), float(win_sigma), float(K[0]), float(K[1]),
            N.DR_SSIM_NONNEGATIVE if nonnegative_ssim else 0)


def dssim_mse_fwd(out, reference, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=True):
    """Forward of the demo's loss nan_to_num(1 - ssim(out, reference)) + mse(out, reference) (dr_dssim_mse_fwd, DESIGN.md D9;
    OPT.py:70-72 with differender_amd.utils.ssim2d's semantics). out, reference: (N, C, H, W) float32 on the GPU.
    Returns `stats`, a float64 tensor of N*C + 3 on the device: the per-plane SSIM, then loss, dssim, mse."""
    x, y, strides = _loss_inputs(out, reference)
    n, c, h, w = x.shape
    stats = torch.empty(n * c + 3, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        rc = N.lib().dr_dssim_mse_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, strides,
                                      *_loss_config(data_range, win_size, win_sigma, K, nonnegative_ssim),
                                      stats.data_ptr(), _stream())
    N.check(rc, "dr_dssim_mse_fwd")
    return stats


def dssim_mse_bwd(out, reference, stats, upstream=None, want_ref_grad=False, data_range=1.0, win_size=11, win_sigma=1.5,
                  K=(0.01, 0.03), nonnegative_ssim=True):
    """Gradient of dssim_mse_fwd's outputs (dr_dssim_mse_bwd): `stats` is that forward's, `upstream` the gradients of the
    caller's objective w.r.t. (loss, dssim, mse), a 3-element float32 tensor on the device (None = (1, 0, 0): loss.backward()).
    Returns (d out, d reference or None); bitwise deterministic."""
    x, y, strides = _loss_inputs(out, reference)
    n, c, h, w = x.shape
    upstream, gx, gy = _loss_bwd_buffers(x, stats, n * c + 3, "stats must be the float64 output of dssim_mse_fwd for these images",
                                         upstream, "dssim", want_ref_grad)
    with torch.cuda.device(x.device):
        rc = N.lib().dr_dssim_mse_bwd(x.data_ptr(), y.data_ptr(), n, c, h, w, strides,
                                      *_loss_config(data_range, win_size, win_sigma, K, nonnegative_ssim),
                                      stats.data_ptr(), None if upstream is None else upstream.data_ptr(), gx.data_ptr(),
                                      None if gy is None else gy.data_ptr(), _stream())
    N.check(rc, "dr_dssim_mse_bwd")
    return gx, gy


def dssim_mse_loss_grad(out, reference, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=True):
    """The demo's loss and its gradient w.r.t. `out` in one forward + backward (the counterpart of mse_loss_grad).
    Returns (loss, dssim, mse, grad_out): three 0-d float64 tensors on the device and a float32 gradient shaped like out."""
    cfg = dict(data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=K, nonnegative_ssim=nonnegative_ssim)
    stats = dssim_mse_fwd(out, reference, **cfg)
    grad, _ = dssim_mse_bwd(out, reference, stats, **cfg)
    loss, dssim, mse = stats[-3:].unbind(0)
    return loss, dssim, mse, grad


def _msssim_config(data_range, win_size, win_sigma, K, weights):
    from .utils.losses import MS_SSIM_WEIGHTS
    w = [float(v) for v in (MS_SSIM_WEIGHTS if weights is None else weights)]
    return (float(data_range), int(win_size), float(win_sigma), float(K[0]), float(K[1]), (ctypes.c_double * len(w))(*w),
            len(w))


def _msssim_workspace(x, levels, want_ref_grad):
    n, c, h, w = x.shape
    nbytes = N.lib().dr_msssim_workspace_bytes(n, c, h, w, levels, int(want_ref_grad))
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None


def msssim_mse_fwd(out, reference, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
                   weights=None):
    """Forward of nan_to_num(1 - ms_ssim(out, reference)) + mse(out, reference) (dr_msssim_mse_fwd, DESIGN.md D10;
    differender_amd.utils.ms_ssim2d's semantics). out, reference: (N, C, H, W) float32 on the GPU, min(H, W) > 16 (win_size - 1).
    Returns `stats`, float64 on the device: v[levels][N*C], ms[N*C], then loss, dms, mse."""
    x, y, strides = _loss_inputs(out, reference)
    n, c, h, w = x.shape
    cfg = _msssim_config(data_range, win_size, win_sigma, K, weights)
    stats = torch.empty((cfg[-1] + 1) * n * c + 3, dtype=torch.float64, device=x.device)
    ws = _msssim_workspace(x, cfg[-1], False)
    with torch.cuda.device(x.device):
        rc = N.lib().dr_msssim_mse_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, strides, *cfg,
                                       None if ws is None else ws.data_ptr(), stats.data_ptr(), _stream())
    N.check(rc, "dr_msssim_mse_fwd")
    return stats


def msssim_mse_bwd(out, reference, stats, upstream=None, want_ref_grad=False, data_range=1.0, win_size=11, win_sigma=1.5,
                   K=(0.01, 0.03), weights=None):
    """Gradient of msssim_mse_fwd's outputs (dr_msssim_mse_bwd): `stats` is that forward's, `upstream` the gradients of the
    caller's objective w.r.t. (loss, dms, mse), 3 float32 on the device (None = (1, 0, 0)). Returns (d out, d reference or
    None); bitwise deterministic."""
    x, y, strides = _loss_inputs(out, reference)
    n, c, h, w = x.shape
    cfg = _msssim_config(data_range, win_size, win_sigma, K, weights)
    upstream, gx, gy = _loss_bwd_buffers(x, stats, (cfg[-1] + 1) * n * c + 3,
                                         "stats must be the float64 output of msssim_mse_fwd for these images and levels",
                                         upstream, "dms", want_ref_grad)
    ws = _msssim_workspace(x, cfg[-1], want_ref_grad)
    with torch.cuda.device(x.device):
        rc = N.lib().dr_msssim_mse_bwd(x.data_ptr(), y.data_ptr(), n, c, h, w, strides, *cfg, stats.data_ptr(),
                                       None if upstream is None else upstream.data_ptr(), gx.data_ptr(),
                                       None if gy is None else gy.data_ptr(), None if ws is None else ws.data_ptr(),
                                       _stream())
    N.check(rc, "dr_msssim_mse_bwd")
    return gx, gy


def msssim_mse_loss_grad(out, reference, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
                         weights=None):
    """The MS-SSIM + MSE loss and its gradient w.r.t. `out` in one forward + backward.
    Returns (loss, dms, mse, grad_out): three 0-d float64 tensors on the device and a float32 gradient shaped like out."""
    cfg = dict(data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=K, weights=weights)
    stats = msssim_mse_fwd(out, reference, **cfg)
    grad, _ = msssim_mse_bwd(out, reference, stats, **cfg)
    loss, dms, mse = stats[-3:].unbind(0)
    return loss, dms, mse, grad


_TV_NORMS = {"l1": N.DR_TV_L1, "iso": N.DR_TV_ISO, "sq": N.DR_TV_SQ}


def _tv_config(norm, eps):
    if norm not in _TV_NORMS:
        raise ValueError(f"norm must be one of {sorted(_TV_NORMS)}, got {norm!r}")
    eps = float(eps)
    # the kernels add (float)(eps * eps): at or below 2^-150 (eps below about 2.6e-23) it rounds to 0, and a flat voxel's flux is
    # 0 * inf
    if not math.isfinite(eps) or (norm == "iso" and not (eps > 0.0 and eps * eps > 2.0 ** -150)):
        raise ValueError(f"eps must be finite (and for norm='iso' > 0 with a square that float32 holds, eps >= 3e-23), got {eps}")
    return _TV_NORMS[norm], eps


def _tv_strides(t):
    """(B, D, H, W, int64 strides[4]) of t's last three axes and its leading axes taken as one, or None when the leading axes
    do not collapse into one stride."""
    lead = [(n, s) for n, s in zip(t.shape[:-3], t.stride()[:-3]) if n > 1]
    for (n0, s0), (n1, s1) in zip(lead, lead[1:]):
        if s0 != n1 * s1:
            return None
    b = math.prod(t.shape[:-3])
    sb = lead[-1][1] if lead else 0
    return (b, *t.shape[-3:], (ctypes.c_int64 * 4)(sb, *t.stride()[-3:]))


def _tv_volume(vol):
    if vol.ndim < 3:
        raise ValueError(f"the TV regulariser expects a volume (..., D, H, W), got {vol.ndim} dimensions")
    _require_gpu(vol, "vol")
    tag = _dtype_tag(vol, "the TV regulariser reads float32 or float16 volumes")
    geo = _tv_strides(vol)
    if geo is None:   # leading axes that no single stride describes: one copy
        vol = vol.contiguous()
        geo = _tv_strides(vol)
    return vol, tag, geo


def tv3d_fwd(vol, norm="l1", eps=1e-3):
    """Sum over the voxels of the 3-D total variation of `vol` (dr_tv3d_fwd; differender_amd.utils.tv3d with
    reduction="sum"). vol: (..., D, H, W) float32 or float16 on the GPU, any strides. Returns a 0-d float64 tensor on the
    device."""
    n, e = _tv_config(norm, eps)
    vol, tag, (b, d, h, w, strides) = _tv_volume(vol)
    out = torch.empty((), dtype=torch.float64, device=vol.device)
    with torch.cuda.device(vol.device):
        rc = N.lib().dr_tv3d_fwd(vol.data_ptr(), tag, b, d, h, w, strides, n, e, out.data_ptr(), _stream())
    N.check(rc, "dr_tv3d_fwd")
    return out


def tv3d_bwd(vol, upstream=None, scale=1.0, norm="l1", eps=1e-3, out=None, accumulate=False):
    """Gradient of tv3d_fwd's sum (dr_tv3d_bwd): out = (out if accumulate else 0) + upstream * scale * dTV/dvol, float32, shaped
    like vol. `upstream`: one float32 on the device (None = 1), read there (no host synchronisation). `out` may be any
    float32 tensor of vol's shape whose elements do not overlap (e.g. the d_volume of the march; a padded or sliced view keeps
    what lies between its elements); None allocates one in vol's stride order. Bitwise deterministic. norm="iso" needs an eps
    whose square float32 holds (eps >= 3e-23): a smaller one raises ValueError."""
    n, e = _tv_config(norm, eps)
    vol, tag, (b, d, h, w, strides) = _tv_volume(vol)
    if upstream is not None:
        upstream = upstream.to(device=vol.device, dtype=torch.float32).contiguous()
        if upstream.numel() != 1:
            raise ValueError("upstream is the gradient of the scalar TV sum: 1 element")
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs `out`")
        out = torch.empty_like(vol, dtype=torch.float32)
        if not _dense(out) or _tv_strides(out) is None:
            out = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    if out.shape != vol.shape or out.dtype != torch.float32 or out.device != vol.device:
        raise ValueError("out must be a float32 tensor of vol's shape on vol's device")
    gstrides = _tv_strides(out)
    if gstrides is None or not _disjoint(out):
        raise ValueError("out must not have overlapping elements, and its leading axes must collapse into one stride")
    with torch.cuda.device(vol.device):
        rc = N.lib().dr_tv3d_bwd(vol.data_ptr(), tag, b, d, h, w, strides, n, e,
                                 None if upstream is None else upstream.data_ptr(), float(scale), out.data_ptr(),
                                 gstrides[-1], int(bool(accumulate)), _stream())
    N.check(rc, "dr_tv3d_bwd")
    return out


def tf_momentum_step(tf, d_tf, momentum, lr, gamma, max_grad):
    """In-place momentum step on the transfer function (dr_tf_momentum_step; apply_grad, EX.py:375-381):
    momentum = gamma*momentum + lr*clamp(d_tf, +-max_grad); tf = max(tf - momentum, 0)."""
    _require_gpu(tf, "tf")
    for t, name in ((tf, "tf"), (d_tf, "d_tf"), (momentum, "momentum")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != tf.shape or t.device != tf.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor of tf's shape on tf's device")
    with torch.cuda.device(tf.device):
        rc = N.lib().dr_tf_momentum_step(tf.data_ptr(), d_tf.data_ptr(), momentum.data_ptr(), tf.numel(), float(lr),
                                         float(gamma), float(max_grad), _stream())
    N.check(rc, "dr_tf_momentum_step")
    _hints.invalidate(tf)   # written through its raw pointer: torch's version counter did not see it
    return tf, momentum
