"""Float64 / float32 reference of the depth march over a ray bundle: a ray is an input, with gradients to its
origin, its direction, the volume and the table.

A composition, nothing here is derived by hand: `bundle_reference.slab` supplies the ray buffers (the slab arithmetic per ray,
the t_near clamp, the jitter), make_autograd_golden's `march` is the sample loop under its driver `render_view` on a (P, 1)
image, and the sample is depth_reference.raycast_depth's with ONE difference, which is the definition of what the kernels
compute: the distance of a sample is the march's own parameter

    t = ((pos - o) . d) / (d . d),

not the dot product (pos - o) . d. On unit directions the two are the same number. As functions of a free direction they are
not: pos - o = t d whatever |d| is, so the dot product is t |d|^2 and its derivative w.r.t. d carries the radial term 2 t e_s d
(e_s the sample's dL/dt) that the march parameter does not have. torch.autograd differentiates the whole program. A bundle is
laid out as a (P, 1) image, as in bundle_reference, so the helpers written for images (camgrad_gpu.well_conditioned,
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

COLUMNS = BR.COLUMNS
F32 = BR.F32


def raycast_depth_bundle(vol, tf, o, entry, exit_, d, n, max_samples, sampling_rate, radial=False):
    """The rays o + t d, one row per ray -> the moments (P, 4) = (M1, M2, 0, A) and the live-sample counts. radial: the sample's
    distance as the dot product (pos - o) . d instead (a mutation for the tests: the other definition)."""
    def sample(pos):
        alpha = G.apply_transfer_function(tf, G.sample_volume_trilinear(vol, pos))[:, 3]
        op = 1.0 - torch.pow(1.0 - alpha, 1.0 / sampling_rate)
        t = ((pos - o) * d).sum(1)
        if not radial:
            t = t / (d * d).sum(1)
        return torch.stack([op * t, op * t * t, torch.zeros_like(op), op], dim=1), alpha, {}

    out, _, count, _ = G.march(o, entry, exit_, d, n, max_samples, False, sample)
    return out, count


def run(inp, dtype=torch.float64, pixels=None, grads=True, radial=False):
    """inp: vol (VX,VY,VZ), tf (R,4), origins, dirs (P,3), grad_out (P,4), sr, max_samples; optional t_near, jitter_seed,
    ray_base. The forward in `dtype`; pixels: mask (P,) or flat indices of the rays to march (default all with n > 1).
    -> bundle_reference.run's keys: rgba (P,1,4) (the moments), steps, n (P,1), entry, exit (P,1), d_origin, d_dir (P,1,3), dray
    (P,1,6) = both, dvol, dtf (grads=False: the forward alone, no gradients)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    P = np.asarray(inp["origins"]).shape[0]
    o, d = T(inp["origins"]).requires_grad_(grads), T(inp["dirs"]).requires_grad_(grads)
    vol, tf = T(inp["vol"]).requires_grad_(grads), T(inp["tf"]).requires_grad_(grads)
    e, x, n = BR.slab(o, d, inp["vol"].shape, float(inp["sr"]), inp.get("t_near"), int(inp.get("jitter_seed", 0)),
                      int(inp.get("ray_base", 0)))

    def march_rays(sel):
        out, cnt = raycast_depth_bundle(vol, tf, o[sel], e[sel], x[sel], d[sel], n[sel], int(inp["max_samples"]),
                                        float(inp["sr"]), radial)
        return out, dict(steps=cnt.int())

    with torch.set_grad_enabled(grads):
        loss, res = G.render_view((P, 1), n, pixels, T(inp["grad_out"]).reshape(P, 4) if grads else None, march_rays)
    if torch.is_tensor(loss):   # (else no ray marched)
        loss.backward()
    res.update(entry=e.detach().double().numpy().reshape(P, 1), exit=x.detach().double().numpy().reshape(P, 1),
               n=n.numpy().astype(np.int32).reshape(P, 1))
    if grads:
        d_o, d_d = G.grad_or_zero(o).reshape(P, 1, 3), G.grad_or_zero(d).reshape(P, 1, 3)
        res.update(d_origin=d_o, d_dir=d_d, dray=np.concatenate([d_o, d_d], -1), dvol=G.grad_or_zero(vol), dtf=G.grad_or_zero(tf))
    return res


# ---- the cases of tests/test_gpu_depth_bundle.py and of the conditioning test (tests/test_depth_bundle.py) ----------------------

AIR_CASES = [("m_object_in_air", "ortho"), ("m_object_in_air", "random")]
GRAD_CASES = [c for c in BR.GRAD_CASES if c not in AIR_CASES] + list(BR.EDGE_CASES)
GRAD_CASES += [("j_inside", "interior"), ("j_inside", "interior_near0")]
SINGLE_CASE = ("a_orbit_sr1", "single_sample")
# rates and caps: (scene, bundle, overrides of the scene's sr / max_samples)
RATE_CASES = [("a_orbit_sr1", "random", dict(sr=0.6)), ("a_orbit_sr1", "random", dict(sr=3.0)), ("b_sr2_ert", "ortho", dict(sr=4.0)),
              ("a_orbit_sr1", "random", dict(max_samples=1)), ("a_orbit_sr1", "random", dict(max_samples=2))]
TIER_R = (3392, 3393, 10176, 10177)

inputs = BR.inputs
keep = BR.keep


def refs(inp):
    """(float64 reference, float32 transliteration) of inp."""
    return run(inp), run(inp, torch.float32)


@functools.lru_cache(maxsize=None)
def state(scene, bundle, over=()):
    """The inputs and the two references of a case (computed once and shared; nobody writes to them). over: a tuple of
    (key, value) pairs in the place of the scene's own."""
    inp = dict(inputs(scene, bundle), **dict(over))
    return (inp,) + refs(inp)


@functools.lru_cache(maxsize=None)
def tier_state(R):
    inp = BR.smooth_tier_inputs(R)
    return (inp,) + refs(inp)
