"""What the GPU tests of the RGBA march (tests/test_gpu_rgba.py, tests/test_gpu_rgba_edges.py) share: the input recipe, and the
comparison against the float64 transliteration (tests/rgba_reference.py) by the rule of tests/test_gpu_tf2d.py (D8 / D12)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rgba_reference as RR  # noqa: E402

DEV = torch.device("cuda")
C = lambda t: t.detach().double().cpu().numpy()


def volume(shape, kind, seed=0, views=None):
    """Field-order RGBA volume ([views,] 4, VX, VY, VZ) float32 on the host: rgb uniform in [0.05, 0.95] per voxel, alpha
    "thin" = 0.01 + 0.05 b or "opaque" = 0.05 + 0.9 b^2 with b = clip(synth_volume + 0.02 noise, 0, 1)."""
    from oracle import oracle as O
    rng = np.random.RandomState(seed)
    lead = () if views is None else (views,)
    b = np.clip(O.synth_volume(shape, dtype=np.float64) + 0.02 * rng.standard_normal((*lead, *shape)), 0.0, 1.0)
    vol = rng.uniform(0.05, 0.95, size=(*lead, 4, *shape))
    vol[..., 3, :, :, :] = 0.01 + 0.05 * b if kind == "thin" else 0.05 + 0.9 * b ** 2
    return torch.from_numpy(vol.astype(np.float32))


def cams(views, first=0.9):
    from oracle import oracle as O
    return torch.from_numpy(np.stack([O.in_circles(first + 1.7 * i) for i in range(views)])).float().to(DEV)


def reference(vol4, cam, WH, S, sr, jitter=0, seed=0, rays=None):
    """The GPU forward and the f64 / f32 transliterations on the GPU's own ray buffers. Rays whose live-sample count differs
    between the GPU, the f32 and the f64 transliteration are masked (zero upstream gradient `gm`, not compared); the mask must
    keep 80 % of the rays with n > 1."""
    from differender_amd import functional as F
    V = cam.shape[0]
    e, x, r, n = rays if rays is not None else F.ray_setup(cam, WH, vol4.shape[-3:], sr, jitter_seed=jitter)
    out, steps = F.march_rgba_fwd(vol4, cam, e, x, r, n, S, sr)
    host = dict(vol=C(vol4.float()), cam=C(cam), entry=C(e), exit_=C(x), rays=C(r), n=n.cpu().numpy())
    go = torch.randn((V, *WH, 4), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()
    args = lambda g: (host["vol"], host["cam"], host["entry"], host["exit_"], host["rays"], host["n"], g, S, sr)
    ref = RR.run(*args(go), want_grad=False)
    ref32 = RR.run(*args(go), dtype=torch.float32, want_grad=False)
    mask = (steps.cpu().numpy() == ref["steps"]) & (ref32["steps"] == ref["steps"]) & (host["n"] > 1)
    assert mask.sum() >= 0.8 * (host["n"] > 1).sum(), (mask.sum(), (host["n"] > 1).sum())
    gm = go * mask[..., None]
    ref = RR.run(*args(gm), pixels=mask)
    ref32 = RR.run(*args(gm), dtype=torch.float32, pixels=mask)
    return dict(ref=ref, ref32=ref32, mask=mask, host=host, rays=(e, x, r, n), out=out, steps=steps, S=S, sr=sr, cam=cam,
                gm=torch.from_numpy(gm).float().to(DEV))


def assert_close(got, st, k, floor=1e-5):
    """got (a float64 numpy array) against st["ref"][k] ("rgba" or "dvol"): the bar is 3x the f32 transliteration's own error,
    with a floor of `floor` x the largest reference element. Prints the figures first."""
    mask = st["mask"]
    m = mask[..., None] if k == "rgba" else 1
    want = st["ref"][k] * m
    err = np.abs(got * m - want).max()
    err32 = np.abs(st["ref32"][k] * m - want).max()
    scale = np.abs(want).max()
    print(f"{k}: err {err / max(scale, 1e-300):.3e} f32 transliteration {err32 / max(scale, 1e-300):.3e} (of max |ref| {scale:.3e})")
    assert scale > 0, k
    assert err <= 3.0 * err32 + floor * scale, (k, err / scale, err32 / scale)


def backward(vol4, st):
    from differender_amd import functional as F
    return F.march_rgba_bwd(vol4, st["cam"], *st["rays"], st["S"], st["sr"], st["gm"], st["out"])


def compare(vol4, cam, WH, S, sr, jitter=0, seed=0):
    """GPU forward + backward of vol4 against the f64 transliteration; returns the state of reference()."""
    st = reference(vol4, cam, WH, S, sr, jitter, seed)
    assert_close(C(st["out"]), st, "rgba")
    d_vol = backward(vol4, st)
    assert d_vol.dtype == torch.float32 and d_vol.shape == vol4.shape
    assert_close(C(d_vol), st, "dvol")
    return st
