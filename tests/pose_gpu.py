"""What the GPU tests of the free camera share (test_gpu_pose.py, test_gpu_pose_edges.py): inputs rounded to what the kernels
read, one launch of F.march_fwd + F.march_bwd_pose on the ray buffers of the float64 reference (tests/pose_reference.py), and
D8's rule (camgrad_gpu.d8_rule) applied to the columns of each of the four pose tensors."""
import math

import numpy as np
import torch

import camgrad_gpu as K
import make_camgrad_golden as CG
import pose_reference as PR

F32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
F16 = lambda a: np.asarray(a, np.float16).astype(np.float64)
COLUMNS = (("look_from", slice(0, 3)), ("look_at", slice(3, 6)), ("up", slice(6, 9)), ("fov", slice(9, 10)))
POSE_KEYS = ("look_from", "look_at", "up", "fov_rad")


def dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"), dt)


def inputs(name, WH=None, **over):
    """The scene of a camera-gradient fixture's case (make_camgrad_golden.CASES: volume, TF, upstream gradient, rate, max_samples,
    jitter seed, view; its camera as look_from) with a pose and other settings laid over it, rounded to what the kernel reads."""
    inp = CG.make_inputs(name)
    inp["look_from"] = inp.pop("cam")
    if WH is not None:
        inp["grad_out"] = np.random.RandomState(WH[0] * 100 + WH[1]).standard_normal((*WH, 4))
    inp.update(over)
    for k in ("vol", "tf", "grad_out", *POSE_KEYS):
        if k in inp:
            inp[k] = F32(inp[k])
    return inp


def refs(inp):
    return K.with_kinks(inp, PR.run_case(inp), "look_from"), PR.run_case(inp, dtype=torch.float32)


def keep(ref, ref32):
    return (ref32["steps"] == ref["steps"]) & (ref32["n"] == ref["n"])


def well_conditioned(ref, ref32, keep_, what=None, key="dpose_ray", lit=True):
    """camgrad_gpu.well_conditioned over the four pose tensors, each judged by its own scale: the mask of the second pass."""
    return K.well_conditioned(ref, ref32, keep_, key, COLUMNS, what, lit)


def pose_rows(inps):
    """(poses (V, 9), fov_v (V,) radians or None when no view names its own fov) of the views' inputs."""
    row = lambda i: np.concatenate([np.asarray(i["look_from"]), np.asarray(i.get("look_at", PR.ORIGIN)), np.asarray(i.get("up", PR.UP_Y))])
    fov = None
    if any("fov_rad" in i for i in inps):
        fov = np.array([float(i.get("fov_rad", math.radians(PR.FOV_DEG))) for i in inps])
    return np.stack([row(i) for i in inps]), fov


def launch(vol, tf, inps, refs_, keeps, S, sr, seed=0, view_base=0, rows=None, upstream=None, grad_outs=None):
    """camgrad_gpu.launch for poses: one launch over len(inps) views on the reference's ray buffers; only the rays in `keep`
    whose march stops where the reference's does get an upstream gradient.
    -> per-ray d_pose (V, W, H, 10) float64, totals (V, 10) float64, masks (V, W, H), the upstream gradient handed in."""
    from differender_amd import functional as F
    poses, fov = pose_rows(inps)
    pose = dev(poses)
    fov_v = None if fov is None else dev(fov)
    stack = lambda k, dt=torch.float32: dev(np.stack([np.asarray(r[k]) for r in refs_]), dt)
    e, x, r, n = stack("entry"), stack("exit"), stack("rays"), stack("n", torch.int32)
    cam = pose[:, :3].contiguous()
    out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, rows=rows, pose=pose, fov_v=fov_v)
    got = steps.cpu().numpy()
    masks = np.stack([(got[v] == refs_[v]["steps"]) & (refs_[v]["n"] > 1) & keeps[v] for v in range(len(inps))])
    gos = [i["grad_out"] for i in inps] if grad_outs is None else grad_outs
    g = dev(np.stack([gos[v] * masks[v][..., None] for v in range(len(inps))]))
    if upstream is not None:
        g = upstream(g)
    d, d_ray = F.march_bwd_pose(vol, tf, pose, e, x, r, n, steps, S, sr, g, out, jitter_seed=seed, view_base=view_base, rows=rows,
                                per_ray=True, fov_v=fov_v)
    torch.cuda.synchronize()
    return d_ray.double().cpu().numpy(), d.double().cpu().numpy(), masks, g


def hip_per_ray(inp, ref, vol_dtype, keep_):
    ray, total, mask, _ = launch(dev(inp["vol"]).to(vol_dtype), dev(inp["tf"]), [inp], [ref], [keep_], int(inp["max_samples"]),
                                 float(inp["sr"]), int(inp["jitter_seed"]), int(inp["view"]))
    return ray[0], total[0], mask[0]


def both_passes(inp, ref, ref32, vol_dtype, what, run=hip_per_ray):
    """One view, one launch per pass: pose_rule over all compared rays, then over the well-conditioned ones alone.
    run(inp, ref, vol_dtype, keep) -> (ray, total, mask, ...). -> the first pass's (ray, total, mask)."""
    first = run(inp, ref, vol_dtype, keep(ref, ref32))[:3]
    pose_rule(*first[:2], ref, ref32, first[2], what)
    ray, total, mask = run(inp, ref, vol_dtype, well_conditioned(ref, ref32, keep(ref, ref32), what))[:3]
    pose_rule(ray, total, ref, ref32, mask, (what, "conditioned"))
    return first


def _three(a, sl):
    """Columns sl of the ten as the three columns camgrad_gpu's rule takes (the single fov column padded with zeros)."""
    a = a[..., sl]
    return a if a.shape[-1] == 3 else np.concatenate([a, np.zeros(a.shape[:-1] + (3 - a.shape[-1],))], -1)


def pose_rule(ray, total, ref, ref32, mask, what=None, key="dpose_ray"):
    """D8's rule, as camgrad_gpu.d8_rule states it, for the columns of each pose tensor: per ray err <= 3 err32 + 1e-4 scale (the
    scale that tensor's own largest component), the total against the rays' sum to 1e-5 and against the float64 sum by
    d8_total_rule, compared rays >= 80 % of the n > 1 rays. The tensors are judged apart: d up is typically a tenth of
    d look_at, and one scale over all ten columns would let it pass with no correct digit."""
    for name, sl in COLUMNS:
        K.d8_rule(_three(ray, sl), _three(total, sl), {"n": ref["n"], "dcam_ray": _three(ref[key], sl)},
                  {"dcam_ray": _three(ref32[key], sl)}, mask, (what, name))


def pose_total_rule(total, want_ray, ref32_ray, mask, what=None):
    for name, sl in COLUMNS:
        K.d8_total_rule(_three(total, sl), _three(want_ray, sl), _three(ref32_ray, sl), mask, (what, name))
