"""ctypes/numpy front-end of the CPU oracle (oracle/dr_oracle.c).

TEST INFRASTRUCTURE ONLY -- imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg, never by differender_amd. PARITY UNPINNED (the reference has no golden vectors and cannot be
imported here; see DESIGN.md section "Oracle").

Array conventions (same as the C file): volume (VX, VY, VZ) = the reference's field index (i, j, k)
(VR.py:481: (W, D, H) of the user's (1, D, H, W) tensor); tf (R, 4); image buffers (W, H[, C]).
"""
import ctypes
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libdr_oracle.so")
_lib = None


def build(force=False):
    """Compile the oracle with gcc (no GPU toolchain involved)."""
    src = [os.path.join(_HERE, f) for f in ("dr_oracle.c", "dr_oracle_impl.inc")]
    if (not force and os.path.exists(_LIB_PATH)
            and all(os.path.getmtime(_LIB_PATH) >= os.path.getmtime(s) for s in src)):
        return _LIB_PATH
    subprocess.check_call(["make", "-C", _HERE, "-B", "libdr_oracle.so"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB_PATH)
    return _lib


def _ct(dt):
    return ctypes.c_float if dt == np.float32 else ctypes.c_double


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _suffix(dt):
    return "_f32" if np.dtype(dt) == np.float32 else "_f64"


def ray_setup(cam, W, H, vol_shape, sr=1.0, fov_deg=30.0, near=0.1, jitter_seed=0, view=0, dtype=np.float32):
    """VR.py:221-259. Returns entry (W,H), exit (W,H), rays (W,H,3), n (W,H) int32."""
    dt = np.dtype(dtype)
    cam = np.ascontiguousarray(cam, dtype=dt)
    entry = np.empty((W, H), dt); exit_ = np.empty((W, H), dt)
    rays = np.empty((W, H, 3), dt); n = np.empty((W, H), np.int32)
    fn = getattr(lib(), "dro_ray_setup" + _suffix(dt))
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_double, ctypes.c_double, _ct(dt), ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rc = fn(_p(cam), W, H, *map(int, vol_shape), float(np.radians(fov_deg)), float(near), float(sr),
            int(jitter_seed), int(view), _p(entry), _p(exit_), _p(rays), _p(n))
    assert rc == 0
    return entry, exit_, rays, n


def march_fwd(vol, tf, cam, entry, exit_, rays, n, S, sr=1.0, mode=0, accum64=False):
    """mode 0: VR.py:261-306 + 363-372 (differentiable path); mode 1: VR.py:308-361 (nondiff).
    accum64 (float32 only): the same float32 samples and contributions, composited in double.
    Returns rgba (W,H,4), steps (W,H) int32."""
    dt = vol.dtype
    if accum64 and dt != np.float32:
        raise ValueError("accum64 composites the float32 march: a float32 volume is required")
    vol = np.ascontiguousarray(vol); tf = np.ascontiguousarray(tf, dtype=dt)
    cam = np.ascontiguousarray(cam, dtype=dt)
    entry = np.ascontiguousarray(entry, dtype=dt); exit_ = np.ascontiguousarray(exit_, dtype=dt)
    rays = np.ascontiguousarray(rays, dtype=dt); n = np.ascontiguousarray(n, dtype=np.int32)
    W, H = n.shape
    out = np.empty((W, H, 4), dt); steps = np.empty((W, H), np.int32)
    fn = getattr(lib(), "dro_march_fwd" + _suffix(dt) + ("_acc64" if accum64 else ""))
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_int, ctypes.c_int, ctypes.c_int, _ct(dt), ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p]
    rc = fn(_p(vol), *vol.shape, _p(tf), tf.shape[0], _p(cam), _p(entry), _p(exit_), _p(rays), _p(n),
            W, H, int(S), float(sr), int(mode), _p(out), _p(steps))
    assert rc == 0
    return out, steps


def march_bwd(vol, tf, cam, entry, exit_, rays, n, S, sr, grad_out, want_vol=True, want_tf=True):
    """Adjoint of march_fwd(mode=0) w.r.t. vol and tf (VR.py:460-461,470-471). Returns (d_vol, d_tf)."""
    dt = vol.dtype
    vol = np.ascontiguousarray(vol); tf = np.ascontiguousarray(tf, dtype=dt)
    cam = np.ascontiguousarray(cam, dtype=dt)
    entry = np.ascontiguousarray(entry, dtype=dt); exit_ = np.ascontiguousarray(exit_, dtype=dt)
    rays = np.ascontiguousarray(rays, dtype=dt); n = np.ascontiguousarray(n, dtype=np.int32)
    grad_out = np.ascontiguousarray(grad_out, dtype=dt)
    W, H = n.shape
    d_vol = np.zeros_like(vol) if want_vol else None
    d_tf = np.zeros_like(tf) if want_tf else None
    fn = getattr(lib(), "dro_march_bwd" + _suffix(dt))
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_int, ctypes.c_int, ctypes.c_int, _ct(dt), ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    rc = fn(_p(vol), *vol.shape, _p(tf), tf.shape[0], _p(cam), _p(entry), _p(exit_), _p(rays), _p(n),
            W, H, int(S), float(sr), _p(grad_out), _p(d_vol), _p(d_tf))
    assert rc == 0
    return d_vol, d_tf


def mse_loss_grad(out, ref, inv_norm=None):
    """(loss, grad) of inv_norm * sum (out-ref)^2; inv_norm defaults to 1/numel (torch mse_loss, EX.py:439-443)."""
    out = np.ascontiguousarray(out, np.float32)
    ref = np.ascontiguousarray(ref, np.float32)
    inv_norm = 1.0 / out.size if inv_norm is None else inv_norm
    grad = np.empty_like(out)
    fn = lib().dro_mse_loss_grad_f32
    fn.restype = ctypes.c_double
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]
    loss = fn(_p(out), _p(ref), out.size, np.float32(inv_norm), _p(grad))
    return loss, grad


def tf_momentum_step(tf, d_tf, momentum, lr, gamma, max_grad):
    """In-place apply_grad (EX.py:375-381) on copies; returns (tf, momentum)."""
    tf = np.array(tf, np.float32, order="C")
    mom = np.array(momentum, np.float32, order="C")
    g = np.ascontiguousarray(d_tf, np.float32)
    fn = lib().dro_tf_momentum_step_f32
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                   ctypes.c_float]
    fn(_p(tf), _p(g), _p(mom), tf.size, lr, gamma, max_grad)
    return tf, mom


def render(vol, tf, cam, out_shape, S=1 << 30, sr=1.0, mode=0, jitter_seed=0, view=0, fov_deg=30.0, near=0.1):
    """ray_setup + march_fwd in one call (the sequence of VR.py:431-438)."""
    W, H = out_shape
    S = min(S, 1 << 30)
    e, x, r, n = ray_setup(cam, W, H, vol.shape, sr, fov_deg, near, jitter_seed, view, vol.dtype)
    rgba, steps = march_fwd(vol, tf, cam, e, x, r, n, S, sr, mode)
    return rgba, steps, (e, x, r, n)


# ---- shared synthetic inputs; numpy only so tests and bench agree ----
def synth_volume(N, seed=1234, dtype=np.float32):
    """Smooth, nowhere-flat volume in [0,1]: gaussian blobs + radial falloff + linear ramp."""
    if isinstance(N, int):
        N = (N, N, N)
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-0.6, 0.6, size=(6, 3))
    sigmas = rng.uniform(0.15, 0.5, size=6)
    ax = [np.linspace(-1.0, 1.0, n, dtype=np.float64) for n in N]
    X, Y, Z = np.meshgrid(*ax, indexing="ij", sparse=True)
    acc = np.zeros(N, np.float64)
    for c, s in zip(centres, sigmas):
        acc += np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * s * s))
    v = 0.2 + 0.6 * acc / acc.max() - 0.03 * (X * X + Y * Y + Z * Z) + 0.02 * (X + 2 * Y + 3 * Z) / 6.0
    return np.clip(v, 0.0, 1.0).astype(dtype)  # stays inside (0.09, 0.83): the clip never bites


def bench_tf(R, alpha, dtype=np.float32):
    """Sinusoidal RGB, constant alpha (keeps early termination from firing when alpha = 3/n_max)."""
    i = np.arange(R, dtype=np.float64) / max(R - 1, 1)
    tf = np.empty((R, 4), np.float64)
    for k, phi in enumerate((0.0, 2.1, 4.2)):
        tf[:, k] = 0.5 + 0.5 * np.sin(2 * math.pi * i + phi)
    tf[:, 3] = alpha
    return tf.astype(dtype)


def peaks_tf(R, dtype=np.float32):
    """A 'realistic' TF with two opacity peaks (tf1-like, UT.py:9-21) so early termination fires."""
    i = np.arange(R, dtype=np.float64) / max(R - 1, 1)
    tf = np.empty((R, 4), np.float64)
    tf[:, 0] = 0.9 - 0.5 * i
    tf[:, 1] = 0.3 + 0.6 * i
    tf[:, 2] = 0.5 + 0.4 * np.sin(6.0 * i)
    tf[:, 3] = 0.35 * np.exp(-((i - 0.55) / 0.05) ** 2) + 0.08 * np.exp(-((i - 0.75) / 0.03) ** 2)
    return tf.astype(dtype)


def in_circles(i, y=0.7, dist=2.5):
    """UT.py:80-83."""
    return np.array([math.cos(i) * dist, y, math.sin(i) * dist], np.float32)


def dark_shell_scene(N, sr, body="flat", op=3e-4, c=4.7e-4, R=64, shell_vox=2.4, radius=0.75, seed=7):
    """DESIGN.md D4, the dim-behind-bright case: a ball whose bright shell (intensity 0.9, TF rgb 1, alpha 0.25) is shell_vox
    VOXELS thick -- the transmittance behind it stays near 0.75 ** shell_vox whatever N and sr are -- around a body (intensity 0.5)
    whose TF colour c is nearly black at an ORDINARY opacity: its TF alpha is 1 - (1 - op) ** sr, so every body sample has the
    per-sample opacity op (>= DR_D4_TINY_OP; the default keeps alpha above the non-differentiable march's 1e-3 cut from rate 4
    on) at sampling rate sr. Behind the shell (T <~ 0.3 with the TF ramps on either side of it) each body sample adds
    T * L * c * op to a running colour of ~0.8: with the defaults below 0.3 of an ulp, so sequential float32 compositing drops
    every one of them.
      body="flat":    constant intensity: zero gradient, ambient lighting only (L = 0.4);
      body="noisy":   the intensity jitters voxel by voxel inside the body's TF range: lit and dim samples mixed in every
                      segment (contributions from below half an ulp to a few ulps), c lowered to 0.75x;
      body="rounded": flat, with c raised 2.5x: contributions up to ~0.7 ulp on the rays that see the most of the body -- each one
                      rounded UP to a whole ulp there, dropped on the rays with less light behind the shell.
    Returns vol (N, N, N) float32 and tf (R, 4) float32."""
    ax = np.linspace(-1.0, 1.0, N, dtype=np.float32)   # (float32 throughout: 512^3 stays at a few 0.5 GB arrays)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    rad = np.sqrt(X * X + Y * Y + Z * Z)
    inner = np.float32(radius - shell_vox * 2.0 / (N - 1))
    if body == "noisy":
        fill = np.float32(0.5) + np.random.RandomState(seed).uniform(-0.08, 0.08, size=(N, N, N)).astype(np.float32)
    elif body in ("flat", "rounded"):
        fill = 0.5
    else:
        raise ValueError(f"unknown body {body!r}")
    vol = np.where(rad > np.float32(radius), np.float32(0.0), np.where(rad >= inner, np.float32(0.9), np.float32(fill)))
    i = np.arange(R, dtype=np.float64) / (R - 1)
    tf = np.zeros((R, 4), np.float64)
    in_body = (i >= 0.3) & (i < 0.7)
    tf[in_body, :3] = c * {"flat": 1.0, "noisy": 0.75, "rounded": 2.5}[body]
    tf[in_body, 3] = 1.0 - (1.0 - op) ** sr
    tf[i >= 0.7, :3] = 1.0
    tf[i >= 0.7, 3] = 0.25
    return vol.astype(np.float32), tf.astype(np.float32)
