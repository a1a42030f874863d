"""Float64 / float32 reference of the ray-bundle march: a ray is an input, with gradients to its origin and
direction.

`slab` restates the slab arithmetic of pose_reference.ray_setup (its safe denominators for axial rays, its sample count and
jitter) for per-ray leaves o, d (P, 3), plus the t_near clamp; `run` feeds `raycast` of make_autograd_golden.py (imported, not
copied: it takes one camera row per ray and puts the light at cam + e_y) under that file's driver `render_view`.
torch.autograd differentiates the whole program; nothing is derived by hand. A bundle is laid out as a (P, 1) image, so the
helpers written for images (camgrad_gpu.well_conditioned, d8_rule, pose_gpu.keep) take its results as they are.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_autograd_golden as G  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402

COLUMNS = (("origin", slice(0, 3)), ("dir", slice(3, 6)))


def slab(o, d, vol_shape, sr, t_near=None, jitter_seed=0, ray_base=0):
    """entry, exit (P,), n (P,) int64 of the rays o + t d, o and d (P, 3) torch leaves; d is used as given. t_near: None = off;
    else tmin = max(tmin, t_near) before the hit test and the sample count, with no gradient where the clamp is taken."""
    dt = o.dtype
    P = o.shape[0]
    VX, VY, VZ = vol_shape
    diag = math.sqrt((VX - 1) ** 2 + (VY - 1) ** 2 + (VZ - 1) ** 2)
    axial = (d == 0).detach()
    d_safe = torch.where(axial, torch.ones_like(d), d)
    t_lo = torch.where(axial, ((-1.0 - o) / d).detach(), (-1.0 - o) / d_safe)
    t_hi = torch.where(axial, ((1.0 - o) / d).detach(), (1.0 - o) / d_safe)
    tmin = torch.minimum(t_lo, t_hi).max(dim=-1).values
    tmax = torch.maximum(t_lo, t_hi).min(dim=-1).values
    if t_near is not None:
        tmin = torch.where(tmin < t_near, torch.full_like(tmin, float(t_near)), tmin)
    hit = ~((tmax < 0) | (tmin > tmax))
    ray_len = tmax - tmin
    n = torch.where(hit, torch.floor(sr * ray_len.detach() * diag) + 1.0, torch.zeros_like(ray_len)).detach()
    entry = tmin
    if jitter_seed != 0:
        uu = torch.from_numpy(CG.jitter_u(jitter_seed, ray_base, np.arange(P))).to(dt)
        entry = tmin + uu * ray_len / torch.where(n > 0, n, torch.ones_like(n))
    return entry, tmax, n.long()


def run(inp, dtype=torch.float64, pixels=None, grads=True):
    """inp: vol (VX,VY,VZ), tf (R,4), origins, dirs (P,3), grad_out (P,4), sr, max_samples; optional t_near, jitter_seed,
    ray_base. The forward in `dtype`; pixels: mask (P,) or flat indices of the rays to march (default all with n > 1).
    -> rgba (P,1,4), steps, n (P,1), entry, exit (P,1), d_origin, d_dir (P,1,3), dray (P,1,6) = both, dvol, dtf (grads=False:
    the forward alone, no gradients)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    P = np.asarray(inp["origins"]).shape[0]
    o, d = T(inp["origins"]).requires_grad_(grads), T(inp["dirs"]).requires_grad_(grads)
    vol, tf = T(inp["vol"]).requires_grad_(grads), T(inp["tf"]).requires_grad_(grads)
    e, x, n = slab(o, d, inp["vol"].shape, float(inp["sr"]), inp.get("t_near"), int(inp.get("jitter_seed", 0)),
                   int(inp.get("ray_base", 0)))

    def march_rays(sel):
        out, cnt = G.raycast(vol, tf, o[sel], e[sel], x[sel], d[sel], n[sel], int(inp["max_samples"]), float(inp["sr"]))
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


def near_lighting_kink(vol, origins, dirs, ref):
    """camgrad_gpu.near_lighting_kink with one origin per ray (that one broadcasts a single camera): the rays with a live sample
    whose float64 shading lies within float32 rounding of a kink of D7, max(n.l, 0) or min(1, L), by the bound derived there.
    vol: the volume the kernel reads; ref: entry, exit, n, steps of the float64 reference. -> mask (P, 1)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    v, o, r = T(vol), T(origins), T(dirs)
    P = o.shape[0]
    e, x = T(ref["entry"]).reshape(-1), T(ref["exit"]).reshape(-1)
    n, steps = torch.from_numpy(ref["n"].reshape(-1)).long(), torch.from_numpy(ref["steps"].reshape(-1)).long()
    light = G.light_position(o)
    top = np.float32(max(1.0, float(np.abs(vol).max())))
    ulp = float(top - np.nextafter(top, np.float32(0.0)))
    near = torch.zeros(P, dtype=torch.bool)
    for s in range(int(steps.max()) if P else 0):
        live = (s < steps) & (n > 1)
        pos = G.sample_pos(o, e, x, r, n, s, live)
        g = torch.stack([G.sample_volume_trilinear(v, pos + ax) - G.sample_volume_trilinear(v, pos - ax)
                         for ax in 1e-3 * torch.eye(3, dtype=torch.float64)], 1)
        norm = g.norm(dim=1)
        lit = live & (norm > 0)
        safe = torch.where(lit, norm, torch.ones_like(norm))
        nrm = g / safe[:, None]
        ld = pos - light
        ld = ld / ld.norm(dim=1, keepdim=True)
        ndl = (nrm * ld).sum(1)
        rdv = ((ld - 2.0 * ndl[:, None] * nrm) * (-r)).sum(1).clamp(min=0.0)
        L = G.DIFFUSE * ndl.clamp(min=0.0) + G.SPECULAR * rdv ** G.SHININESS + G.AMBIENT
        dn = math.sqrt(3.0) * 2.0 * ulp / safe
        slope = G.DIFFUSE + G.SPECULAR * G.SHININESS * 4.0 * rdv ** (G.SHININESS - 1.0)
        near |= lit & ((ndl.abs() <= dn) | ((L - 1.0).abs() <= slope * dn))
    return near.numpy().reshape(P, 1)


def with_kinks(inp, ref):
    """ref with near_lighting_kink's mask under "near_kink", where camgrad_gpu.well_conditioned reads it."""
    return dict(ref, near_kink=near_lighting_kink(inp["vol"], inp["origins"], inp["dirs"], ref))


# ---- the bundles of the GPU tests (tests/test_gpu_bundle.py) and of the conditioning test (tests/test_bundle.py) ---------------

F32 = lambda a: np.asarray(a, np.float32).astype(np.float64)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def ortho_bundle():
    """A 12 x 12 orthographic grid, extent 2.4, viewed along (0.45, -0.35, -0.82) from 2.6 units off the centre."""
    import differender_amd.bundle as B
    view = _unit(np.array([0.45, -0.35, -0.82]))
    lf = torch.from_numpy(-2.6 * view)
    o, d = B.orthographic_rays(lf, torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), 2.4,
                               (12, 12))
    return o.reshape(-1, 3).numpy().copy(), d.reshape(-1, 3).numpy().copy()


def random_bundle(P=192):
    """Origins on radii 2.2 .. 3.5 aimed at points in [-0.8, 0.8]^3."""
    rng = np.random.RandomState(5)
    o = _unit(rng.standard_normal((P, 3))) * rng.uniform(2.2, 3.5, (P, 1))
    return o, _unit(rng.uniform(-0.8, 0.8, (P, 3)) - o)


def interior_bundle(P=128):
    """Origins uniform in [-0.6, 0.6]^3 with random directions."""
    rng = np.random.RandomState(9)
    return rng.uniform(-0.6, 0.6, (P, 3)), _unit(rng.standard_normal((P, 3)))


BUNDLES = {
    # name: (rays, t_near, jitter seed)
    "ortho": (ortho_bundle, None, 0),
    "random": (random_bundle, None, 0),
    "random_jitter": (random_bundle, None, 777),
    "interior": (interior_bundle, None, 0),
    "interior_near0": (interior_bundle, 0.0, 0),
}
GRAD_CASES = [(scene, b) for scene in ("a_orbit_sr1", "b_sr2_ert") for b in ("ortho", "random", "interior", "interior_near0")]
GRAD_CASES += [("a_orbit_sr1", "random_jitter"), ("m_object_in_air", "ortho"), ("m_object_in_air", "random")]
RAY_BASE = 3


# ---- the bundles of tests/test_gpu_bundle_edges.py: exact zeros in the direction, the t_near clamp some rays take, one sample ----
# (No origin has a coordinate of exactly +-1 on an axis whose direction component is 0: there the kernels' 0 * inf is a NaN that
# fminf / fmaxf drop and torch.minimum keeps, and the two programs define different things.)

def axial_bundle(per_axis=16):
    """16 rays along each of +-x, +-y, +-z: the direction exactly +-e_axis, the origin 2.5 off the centre on that axis and
    uniform in (-0.85, 0.85) on the two others (proj_bundle_reference.axis_inputs' rays, all six axes in one bundle)."""
    os_, ds = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            rng = np.random.RandomState(10 * axis + (sign > 0))
            o = rng.uniform(-0.85, 0.85, (per_axis, 3))
            o[:, axis] = -2.5 * sign
            d = np.zeros((per_axis, 3))
            d[:, axis] = sign
            os_.append(o)
            ds.append(d)
    return np.concatenate(os_), np.concatenate(ds)


def one_zero_bundle(P=96):
    """Rays with exactly one zero direction component, ray p's at index p % 3, aimed at points in [-0.8, 0.8]^3 from 2.2 .. 3.5
    units back along the direction: every ray hits, and its origin's coordinate on the zero axis is its target's."""
    rng = np.random.RandomState(21)
    d = rng.standard_normal((P, 3))
    d[np.arange(P), np.arange(P) % 3] = 0.0
    d = _unit(d)
    return rng.uniform(-0.8, 0.8, (P, 3)) - rng.uniform(2.2, 3.5, (P, 1)) * d, d


SINGLE = np.arange(64) % 8 == 3   # where single_sample_bundle puts its short rays: eight lanes of one wave


def single_sample_bundle():
    """random_bundle's first 56 rays with eight rays among them (SINGLE) that start inside the box 0.01 in front of the face
    x = 1 they leave through: under t_near = 0, which touches none of the 56 (their entry distances are positive), their chord
    is 0.01 < 1 / (sr diag) and n == 1."""
    o56, d56 = random_bundle(56)
    rng = np.random.RandomState(33)
    d8 = _unit(np.concatenate([rng.uniform(0.5, 1.0, (8, 1)), rng.uniform(-0.5, 0.5, (8, 2))], 1))
    o8 = np.concatenate([np.ones((8, 1)), rng.uniform(-0.6, 0.6, (8, 2))], 1) - 0.01 * d8
    o, d = np.empty((64, 3)), np.empty((64, 3))
    o[SINGLE], d[SINGLE], o[~SINGLE], d[~SINGLE] = o8, d8, o56, d56
    return o, d


EDGE_BUNDLES = {
    "axial": (axial_bundle, None, 0),
    "one_zero": (one_zero_bundle, None, 0),
    "random_near2": (random_bundle, 2.0, 0),      # some rays take the clamp, others do not
    "random_near3": (random_bundle, 3.0, 0),      # ... and some die: t_near past their exit
    "interior_near0_jitter": (interior_bundle, 0.0, 777),
    "single_sample": (single_sample_bundle, 0.0, 0),
}
EDGE_CASES = [(scene, b) for scene in ("a_orbit_sr1", "b_sr2_ert") for b in ("axial", "one_zero")]
EDGE_CASES += [("c_clip", b) for b in ("random", "ortho", "interior_near0")]   # max_samples = 23 at 24^3: the cap bites
EDGE_CASES += [("a_orbit_sr1", b) for b in ("random_near2", "random_near3", "interior_near0_jitter")]

TIER_EDGE_R = (3393, 10176, 10177)   # the table in LDS beside d_tf's global atomics; the last R in LDS; the first in global memory


def smooth_tier_inputs(R):
    """The 13 x 12 x 14 volume of tests/test_gpu_bundle.py's table tiers under scene a_orbit_sr1's own 8-texel table resampled
    linearly to R texels, and random_bundle's first 64 rays: the table is as smooth as the scene's at every R, so a sample's
    intensity adjoint (a texel slope times R - 1) is conditioned as in the scene."""
    from oracle import oracle as O
    rng = np.random.RandomState(R)
    vol = np.clip(O.synth_volume((13, 12, 14), dtype=np.float64) + 0.02 * rng.standard_normal((13, 12, 14)), 0.0, 1.0)
    tf8 = CG.make_inputs("a_orbit_sr1")["tf"]
    at = np.linspace(0.0, 1.0, R)
    tf = np.stack([np.interp(at, np.linspace(0.0, 1.0, tf8.shape[0]), tf8[:, c]) for c in range(4)], 1)
    return inputs("a_orbit_sr1", "random", vol=vol, tf=tf, head=64)


# The module's cone beam: a 12 x 10 detector behind the box, its centre off the source's axis; detector column 4 lies at
# x = 0.125 + (4 - 4.5) 0.25 = 0, the source's x, in float32 as in float64 (every term is dyadic): its rays' x component is 0.
CONE = dict(source=(0.0, 0.15, -2.6), det_center=(0.125, 0.1, 1.5), det_u=(0.25, 0.0, 0.0), det_v=(0.0, 0.2, 0.0), det=(12, 10))
CONE_ZERO_COLUMN = 4


def cone_scale():
    """The per-ray factor in [0.5, 2] the cone's unit directions are scaled by before the module sees them, (H, W, 1)."""
    return F32(np.random.RandomState(12).uniform(0.5, 2.0, (*CONE["det"], 1)))


def cone_inputs():
    """Scene a_orbit_sr1 for the cone: vol, tf, sr, max_samples, a random upstream gradient (P, 4); no jitter."""
    base = CG.make_inputs("a_orbit_sr1")
    P = CONE["det"][0] * CONE["det"][1]
    return dict(vol=F32(base["vol"]), tf=F32(base["tf"]), grad_out=F32(np.random.RandomState(P).standard_normal((P, 4))),
                sr=base["sr"], max_samples=base["max_samples"])


def cone_gradient(inp, dtype=torch.float64, pixels=None, grads=True):
    """`run`'s program behind cone_beam_rays, cone_scale and RayBundleRaycaster.forward's own normalisation, all in `dtype`,
    the source and the table the leaves -> run's rgba, steps, n (P, 1, ...) in the detector's row-major order, dirs (P, 3), and
    with grads d_source (3,) and dtf (R, 4) of sum(rgba grad_out) over the rays of `pixels`."""
    import differender_amd.bundle as B
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    src, tf, vol = T(F32(CONE["source"])).requires_grad_(grads), T(inp["tf"]).requires_grad_(grads), T(inp["vol"])
    o, d = B.cone_beam_rays(src, CONE["det_center"], CONE["det_u"], CONE["det_v"], CONE["det"])
    d = d * T(cone_scale())
    d = d / torch.sqrt((d * d).sum(-1, keepdim=True))
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    P = o.shape[0]
    e, x, n = slab(o, d, inp["vol"].shape, float(inp["sr"]))

    def march_rays(sel):
        out, cnt = G.raycast(vol, tf, o[sel], e[sel], x[sel], d[sel], n[sel], int(inp["max_samples"]), float(inp["sr"]))
        return out, dict(steps=cnt.int())

    with torch.set_grad_enabled(grads):
        loss, res = G.render_view((P, 1), n, pixels, T(inp["grad_out"]).reshape(P, 4) if grads else None, march_rays)
    if torch.is_tensor(loss):
        loss.backward()
    res.update(n=n.numpy().astype(np.int32).reshape(P, 1), dirs=d.detach().double().numpy())
    if grads:
        res.update(d_source=G.grad_or_zero(src), dtf=G.grad_or_zero(tf))
    return res


def inputs(scene, bundle, vol=None, tf=None, head=None, rays=None):
    """The scene of a camera-gradient case (make_camgrad_golden.make_inputs: volume, TF, rate, max_samples) with a bundle of
    BUNDLES or EDGE_BUNDLES in its camera's place, rounded to what the kernels read; the directions are unit vectors up to that
    rounding to float32's spacing. vol, tf: others in the scene's place; head: the first `head` rays only; rays: (origins, dirs)
    in the place of the bundle's own."""
    base = CG.make_inputs(scene)
    make, t_near, seed = (BUNDLES.get(bundle) or EDGE_BUNDLES[bundle])
    o, d = make() if rays is None else rays
    o, d = F32(o)[:head], F32(d)[:head]
    P = o.shape[0]
    inp = dict(vol=F32(base["vol"] if vol is None else vol), tf=F32(base["tf"] if tf is None else tf), origins=o, dirs=d,
               grad_out=F32(np.random.RandomState(P).standard_normal((P, 4))), sr=base["sr"], max_samples=base["max_samples"],
               jitter_seed=seed, ray_base=RAY_BASE)
    if t_near is not None:
        inp["t_near"] = t_near
    return inp


def refs(inp):
    """(float64 reference with its near-kink mask, float32 transliteration) of inp."""
    return with_kinks(inp, run(inp)), run(inp, torch.float32)


def keep(ref, ref32):
    return (ref32["steps"] == ref["steps"]) & (ref32["n"] == ref["n"])
