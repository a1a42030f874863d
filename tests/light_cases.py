"""The scenes of the lit march's tests, shared by tests/test_lighting.py (CPU: the two transliterations alone
keep enough rays in every scene) and tests/test_gpu_lighting.py (the kernels against the float64 transliteration), and D8's
masking rule for both: rays whose live count differs between the runs, or that are `near` a lighting kink in float64 or
float32, are left out, and at least 80 % of the live rays must remain.

Sizes are the smallest at which the kernels can still go wrong: volumes of 12 to 24 voxels with unequal edges, images of
16x16, 12x20 and 20x12 (a tile partly outside the image), R of 8 and 32 -- and one R at each threshold of the backward's table
tiers, on an 8x8 image.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import light_reference as LR  # noqa: E402

KEEP = 0.8

# light rows: world position (3), colour (3), ambient, diffuse, specular, shininess
SIDE = (2.4, 0.7, -1.1, 0.9, 0.6, 0.35, 0.1, 0.5, 0.3, 7.5)          # Lraw <= 0.9: nothing clamps
BRIGHT = (-1.8, 1.6, 1.2, 1.1, 0.8, 0.9, 0.55, 0.9, 0.8, 11.0)       # Lraw reaches past 1
SH32 = (1.5, -2.0, 1.0, 0.7, 1.2, 0.5, 0.2, 0.6, 0.45, 32.0)         # the five-squarings path, the other nine non-default
LC_ZERO = (2.0, 1.0, 1.5, 0.8, 0.0, 1.1, 0.15, 0.55, 0.35, 9.0)      # a channel switched off: its gradient is not zero
VIEW_B = (-2.2, 0.4, 1.9, 0.5, 0.9, 0.7, 0.2, 0.45, 0.25, 5.5)
VIEW_C = (0.3, 2.6, -0.8, 1.0, 0.4, 0.6, 0.05, 0.7, 0.5, 14.0)

CASES = {
    # name: (volume shape, image (W, H), R, TF kind, sampling rate, max_samples, jitter seed, f16 volume, light rows, seed)
    "side_colour_sh7": ((14, 12, 16), (16, 16), 8, "thin", 1.0, 4096, 0, False, (SIDE,), 1),
    "bright_clamps": ((16, 14, 12), (12, 20), 8, "thin", 1.0, 4096, 0, False, (BRIGHT,), 2),
    "sh32": ((12, 16, 14), (20, 12), 32, "thin", 1.0, 4096, 0, False, (SH32,), 3),
    "lc_zero": ((14, 12, 16), (16, 16), 8, "thin", 1.0, 4096, 4242, False, (LC_ZERO,), 4),
    "three_views": ((12, 14, 16), (12, 20), 8, "thin", 1.0, 4096, 0, False, (SIDE, VIEW_B, VIEW_C), 5),
    "ert_opaque": ((16, 12, 20), (16, 16), 32, "opaque", 2.0, 4096, 0, False, (SIDE,), 6),
    "clip_S23": ((24, 20, 22), (20, 12), 8, "thin", 1.0, 23, 0, False, (VIEW_B,), 7),
    "sr07": ((14, 16, 12), (16, 16), 32, "thin", 0.7, 4096, 0, False, (VIEW_C,), 8),
    "f16_volume": ((16, 14, 12), (12, 20), 8, "opaque", 1.0, 4096, 0, True, (SIDE,), 9),
}
# one R for each tier of the backward's tables (csrc/march_lit.hip): TF + double d_tf table in LDS (48 R bytes <= 159 KiB),
# the TF alone (16 R bytes <= 159 KiB), nothing; an 8x8 image of one view keeps the reference short
TIERS = {"both_tables": 3392, "tf_only": 3393, "none": 10177}
for _name, _R in TIERS.items():
    CASES["tier_" + _name] = ((14, 12, 16), (8, 8), _R, "thin", 1.0, 4096, 0, False, (BRIGHT,), 10)


def synth_volume(shape, seed):
    """Field-order (VX, VY, VZ) volume in [0, 1] with structure at every scale: smooth blobs plus noise (every corner weight and
    every normal direction is exercised)."""
    rng = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[np.linspace(-1.0, 1.0, s) for s in shape], indexing="ij")
    v = 0.5 + 0.3 * np.sin(3.1 * x + 1.3) * np.cos(2.3 * y - 0.4) * np.sin(1.7 * z + 0.9)
    v = v + 0.4 * np.exp(-8.0 * ((x - 0.2) ** 2 + (y + 0.1) ** 2 + z ** 2))
    return np.clip(v + 0.03 * rng.standard_normal(shape), 0.0, 1.0)


def camera(angle):
    """differender.utils.in_circles: a camera on the reference's orbit."""
    from differender.utils import in_circles
    return in_circles(angle).double().numpy()


def scene(name):
    """The host side of a case: every array holds values a float32 (the volume: float16 where the case says so) represents, so
    the kernels and the transliterations read the same numbers. -> dict(vol, tf, cam (V,3), light (V,10), sr, max_samples,
    jitter, WH, f16)."""
    vshape, WH, R, kind, sr, S, jit, f16, lights, seed = CASES[name]
    rng = np.random.RandomState(100 + seed)
    vol = synth_volume(vshape, seed).astype(np.float16 if f16 else np.float32).astype(np.float64)
    tf = rng.uniform(0.05, 0.95, size=(R, 4))
    tf[:, 3] = np.linspace(0.01, 0.06, R) if kind == "thin" else np.linspace(0.0, 0.9, R) ** 2 + 0.05
    V = len(lights)
    cam = np.stack([camera(0.7 + 0.9 * seed + 1.7 * v) for v in range(V)])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(vol=vol, tf=f32(tf), cam=f32(cam), light=f32(np.asarray(lights)), sr=sr, max_samples=S, jitter=jit, WH=WH,
                f16=f16, seed=seed)


def upstream(sc, V):
    return np.random.RandomState(200 + sc["seed"]).standard_normal((V, *sc["WH"], 4))


def inputs(sc, entry, exit_, rays, n):
    """Scene sc and ray buffers (V,W,H[,3]) as light_reference.run's input, with the scene's upstream gradient."""
    inp = dict(vol=sc["vol"], tf=sc["tf"], cam=sc["cam"], entry=np.asarray(entry, np.float64), exit=np.asarray(exit_, np.float64),
               rays=np.asarray(rays, np.float64), n=np.asarray(n), sr=sc["sr"], max_samples=sc["max_samples"])
    inp["grad_out"] = upstream(sc, inp["n"].shape[0])
    return inp


def kept_rays(sc, inp, steps=None):
    """D8's rule: a forward of the f64 and of the f32 transliteration finds the rays to keep -- equal live counts (also with
    `steps`, the kernels', when given), not `near` in either precision, n > 1 --, and KEEP of the live rays must remain.
    -> (mask (V,W,H), the f64 forward)."""
    f64 = LR.run(inp, sc["light"], want_grad=False)
    f32 = LR.run(inp, sc["light"], dtype=torch.float32, want_grad=False)
    live = inp["n"] > 1
    mask = live & (f64["steps"] == f32["steps"]) & ~f64["near"] & ~f32["near"]
    if steps is not None:
        mask &= np.asarray(steps) == f64["steps"]
    assert live.sum() > 0 and mask.sum() >= KEEP * live.sum(), (int(mask.sum()), int(live.sum()))
    return mask, f64


def reference_state(sc, entry, exit_, rays, n, steps=None):
    """The f64 and f32 transliterations of scene sc on the ray buffers given, forward + backward on the rays kept_rays keeps,
    under the upstream gradient gm = go * mask. -> dict(ref, ref32, mask, gm, inp)."""
    inp = inputs(sc, entry, exit_, rays, n)
    mask, _ = kept_rays(sc, inp, steps)
    gm = inp["grad_out"] * mask[..., None]
    inp["grad_out"] = gm
    return dict(ref=LR.run(inp, sc["light"], pixels=mask), ref32=LR.run(inp, sc["light"], dtype=torch.float32, pixels=mask),
                mask=mask, gm=gm, inp=inp)
