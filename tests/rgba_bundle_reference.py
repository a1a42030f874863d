"""Float64 / float32 reference of the RGBA march over a ray bundle: a ray is an input, with gradients to its
origin, its direction and the four channels of the volume.

A composition, nothing here is written anew: `bundle_reference.slab` supplies the rays (the slab arithmetic per ray, the t_near
clamp, the jitter), `rgba_reference.raycast_rgba` is the march (one camera row per ray), under make_autograd_golden's driver
`render_view`; all three are imported, not copied. torch.autograd differentiates the whole program; nothing is derived by hand.
A bundle is laid out as a (P, 1) image, as in bundle_reference, so the helpers written for images (camgrad_gpu.well_conditioned,
test_gpu_bundle.ray_rule, bundle_reference.keep) take its results as they are.
"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import bundle_reference as BR  # noqa: E402
import make_autograd_golden as G  # noqa: E402
import rgba_gpu as RG  # noqa: E402
import rgba_reference as RR  # noqa: E402

COLUMNS = BR.COLUMNS
F32 = BR.F32


def run(inp, dtype=torch.float64, pixels=None, grads=True):
    """inp: vol (4,VX,VY,VZ), origins, dirs (P,3), grad_out (P,4), sr, max_samples; optional t_near, jitter_seed, ray_base. The
    forward in `dtype`; pixels: mask (P,) or flat indices of the rays to march (default all with n > 1).
    -> bundle_reference.run's keys: rgba (P,1,4), steps, n (P,1), entry, exit (P,1), d_origin, d_dir (P,1,3), dray (P,1,6) = both,
    dvol (4,VX,VY,VZ) (grads=False: the forward alone, no gradients)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    P = np.asarray(inp["origins"]).shape[0]
    o, d = T(inp["origins"]).requires_grad_(grads), T(inp["dirs"]).requires_grad_(grads)
    vol = T(inp["vol"]).requires_grad_(grads)
    e, x, n = BR.slab(o, d, inp["vol"].shape[-3:], float(inp["sr"]), inp.get("t_near"), int(inp.get("jitter_seed", 0)),
                      int(inp.get("ray_base", 0)))

    def march_rays(sel):
        out, cnt, _ = RR.raycast_rgba(vol, o[sel], e[sel], x[sel], d[sel], n[sel], int(inp["max_samples"]), float(inp["sr"]))
        return out, dict(steps=cnt.int())

    with torch.set_grad_enabled(grads):
        loss, res = G.render_view((P, 1), n, pixels, T(inp["grad_out"]).reshape(P, 4) if grads else None, march_rays)
    if torch.is_tensor(loss):   # (else no ray marched)
        loss.backward()
    res.update(entry=e.detach().double().numpy().reshape(P, 1), exit=x.detach().double().numpy().reshape(P, 1),
               n=n.numpy().astype(np.int32).reshape(P, 1))
    if grads:
        d_o, d_d = G.grad_or_zero(o).reshape(P, 1, 3), G.grad_or_zero(d).reshape(P, 1, 3)
        res.update(d_origin=d_o, d_dir=d_d, dray=np.concatenate([d_o, d_d], -1), dvol=G.grad_or_zero(vol))
    return res


# ---- the cases of tests/test_gpu_rgba_bundle.py and of the conditioning test (tests/test_rgba_bundle.py) -----------------------

VOLUMES = {
    # name: (field shape (VX, VY, VZ), rgba_gpu.volume's kind, sampling rate, max_samples)
    "thin_sr1": ((14, 12, 16), "thin", 1.0, 512),
    "opaque_sr2": ((12, 14, 12), "opaque", 2.0, 512),
    # interior_bundle's lines are at least 0.8 long, 19 samples and more at this shape's diagonal of 22.7: every ray is clipped
    "thin_clip": ((14, 12, 16), "thin", 1.0, 10),
}
BUNDLES = dict(BR.BUNDLES, **{k: BR.EDGE_BUNDLES[k] for k in ("axial", "one_zero", "single_sample")})

PARITY_CASES = [("thin_sr1", b) for b in ("ortho", "random", "random_jitter", "interior", "interior_near0", "axial", "one_zero")]
PARITY_CASES += [("opaque_sr2", b) for b in ("ortho", "random", "interior_near0")] + [("thin_clip", "interior")]
RAY_CASES = [("thin_sr1", b) for b in ("random", "random_jitter", "interior_near0", "axial", "one_zero")]
RAY_CASES += [("thin_clip", "interior"), ("opaque_sr2", "random")]
SINGLE_CASE = ("thin_sr1", "single_sample")
CASES = sorted(set(PARITY_CASES + RAY_CASES + [SINGLE_CASE]))


def inputs(volume, bundle, head=None, rays=None):
    """A volume of VOLUMES under a bundle of BUNDLES, rounded to what the kernels read (the directions are unit vectors up to
    that rounding). head: the first `head` rays only; rays: (origins, dirs) in the place of the bundle's own."""
    shape, kind, sr, S = VOLUMES[volume]
    make, t_near, seed = BUNDLES[bundle]
    o, d = make() if rays is None else rays
    o, d = F32(o)[:head], F32(d)[:head]
    P = o.shape[0]
    inp = dict(vol=RG.volume(shape, kind).double().numpy(), origins=o, dirs=d,
               grad_out=F32(np.random.RandomState(P).standard_normal((P, 4))), sr=sr, max_samples=S, jitter_seed=seed,
               ray_base=BR.RAY_BASE)
    if t_near is not None:
        inp["t_near"] = t_near
    return inp


def refs(inp):
    """(float64 reference, float32 transliteration) of inp."""
    return run(inp), run(inp, torch.float32)


@functools.lru_cache(maxsize=None)
def state(volume, bundle):
    """The inputs and the two references of a case (computed once and shared; nobody writes to them)."""
    inp = inputs(volume, bundle)
    return (inp,) + refs(inp)


keep = BR.keep
