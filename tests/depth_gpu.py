"""What the tests of the depth march share (test_depth.py, test_gpu_depth.py): the scenes of the camera-gradient
fixture's cases (make_camgrad_golden.make_inputs, rounded to what the kernels read), one forward on the kernels' own ray buffers
with the float64 / float32 transliterations (tests/depth_reference.py) run on those buffers, the camera cases with their
references on the references' buffers, and one launch of the camera kernels. The bars are imported: light_gpu.bound,
camgrad_gpu.d8_rule, pose_gpu.pose_rule. Nothing here needs a GPU to be imported; the references are computed once per case and
shared (nobody writes to them)."""
import functools
import math

import numpy as np
import torch

import camgrad_gpu as K
import depth_reference as DR
import pose_gpu as PG
from pose_gpu import dev

KEEP = 0.8   # the share of the n > 1 rays a comparison must keep (d8_rule's own cap)
C = lambda t: t.detach().double().cpu().numpy()
POSE = dict(look_at=(0.1, -0.05, 0.08), up=(0.15, 1.0, -0.1), fov_rad=math.radians(26.0))

# forward and volume / TF backward: (case, f16 volume)
MARCH_CASES = [("a_orbit_sr1", False), ("b_sr2_ert", False), ("c_clip", False), ("d_jitter", False), ("e_nonsquare", False),
               ("j_inside", False), ("b_sr2_ert", True)]
# camera and pose: (case, posed, f16 volume); d_jitter draws its jitter as view 2 of the hash (view_base = 2)
CAMERA_CASES = [(name, posed, False) for name in ("a_orbit_sr1", "b_sr2_ert", "d_jitter", "e_nonsquare", "j_inside")
                for posed in (False, True)] + [("b_sr2_ert", True, True)]


def case_id(v):
    return v if isinstance(v, str) else ("posed" if v else "fixed")


@functools.lru_cache(maxsize=None)
def scene(name, f16=False, posed=False):
    """The inputs of depth_reference.run_case for a case: vol, tf, look_from, grad_out (W,H,4), sr, max_samples, jitter_seed,
    view, and with `posed` POSE; f16: the f16-rounded volume the kernel reads."""
    inp = PG.inputs(name, **(POSE if posed else {}))
    if f16:
        inp["vol"] = PG.F16(inp["vol"])
    return inp


def upload(inp, f16=False):
    vol = dev(inp["vol"])
    return (vol.half() if f16 else vol), dev(inp["tf"])


# ---- forward and volume / TF backward on the kernels' own ray buffers ------------------------------------------------------------

def reference_state(vol, tf, cam, e, x, r, n, grad_out, S, sr, steps=None):
    """light_cases.reference_state for the depth march: a forward of the f64 and of the f32 transliteration finds the rays to
    keep -- n > 1, equal live counts in both (and `steps`, the kernels', when given) --, then forward + backward on those rays
    under gm = grad_out * mask. Arrays: vol [V,]VX,VY,VZ, tf [V,]R,4, cam (V,3), buffers (V,W,H[,3]), grad_out (V,W,H,4)."""
    f64 = DR.run(vol, tf, cam, e, x, r, n, grad_out, S, sr, want_grad=False)
    f32 = DR.run(vol, tf, cam, e, x, r, n, grad_out, S, sr, dtype=torch.float32, want_grad=False)
    live = n > 1
    mask = live & (f64["steps"] == f32["steps"])
    if steps is not None:
        mask &= np.asarray(steps) == f64["steps"]
    print(f"kept {int(mask.sum())} of {int(live.sum())} live rays")
    assert live.sum() > 0 and mask.sum() >= KEEP * live.sum(), (int(mask.sum()), int(live.sum()))
    gm = grad_out * mask[..., None]
    return dict(ref=DR.run(vol, tf, cam, e, x, r, n, gm, S, sr, pixels=mask),
                ref32=DR.run(vol, tf, cam, e, x, r, n, gm, S, sr, dtype=torch.float32, pixels=mask), mask=mask, gm=gm)


@functools.lru_cache(maxsize=None)
def forward_state(name, f16=False):
    """Case `name` on the device: F.ray_setup's buffers, F.march_depth_fwd on them and reference_state on those buffers.
    -> dict(inp, vol, tf, cam, rays (entry, exit, rays, n), out, steps, st, S, sr)."""
    from differender_amd import functional as F
    inp = scene(name, f16)
    vol, tf = upload(inp, f16)
    cam = dev(inp["look_from"][None])
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    WH = inp["grad_out"].shape[:2]
    rays = F.ray_setup(cam, WH, vol.shape, sr, jitter_seed=int(inp["jitter_seed"]), view_base=int(inp["view"]))
    out, steps = F.march_depth_fwd(vol, tf, cam, *rays, S, sr)
    e, x, r, n = rays
    st = reference_state(inp["vol"], inp["tf"], inp["look_from"][None], C(e), C(x), C(r), n.cpu().numpy(), inp["grad_out"][None],
                         S, sr, steps.cpu().numpy())
    return dict(inp=inp, vol=vol, tf=tf, cam=cam, rays=rays, out=out, steps=steps, st=st, S=S, sr=sr)


# ---- camera and pose on the references' ray buffers ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def camera_refs(name, posed, f16=False):
    """(inputs, float64 reference, float32 reference) of a camera case."""
    inp = scene(name, f16, posed)
    return inp, DR.run_case(inp), DR.run_case(inp, dtype=torch.float32)


def look_from_columns(ref):
    """A pose reference as camgrad_gpu's rule reads the fixed camera's: under the default pose the look_from columns are the
    fixed camera's gradient."""
    return {"n": ref["n"], "dcam_ray": ref["dpose_ray"][..., :3]}


def good_rays(ref, ref32, posed, what=None):
    """The keep mask of the second, conditioned pass: the rays on which the two references agree (no lighting, no kinks)."""
    keep = PG.keep(ref, ref32)
    if posed:
        return PG.well_conditioned(ref, ref32, keep, what, lit=False)
    return K.well_conditioned(look_from_columns(ref), look_from_columns(ref32), keep, what=what, lit=False)


def rule(ray, total, ref, ref32, mask, posed, what=None):
    if posed:
        PG.pose_rule(ray, total, ref, ref32, mask, what)
    else:
        K.d8_rule(ray, total, look_from_columns(ref), look_from_columns(ref32), mask, what)


def conditioned_entries():
    """id -> (a function that returns [(float64 reference, float32 reference, keep mask, None)], the rule's key and columns):
    what camgrad_gpu.check_conditions is fed, for test_depth.py to hold every camera case to its conditions without a GPU."""
    out = {}
    for name, posed, f16 in CAMERA_CASES:
        def entries(name=name, posed=posed, f16=f16):
            _, ref, ref32 = camera_refs(name, posed, f16)
            keep = PG.keep(ref, ref32)
            return [(ref, ref32, keep, None)] if posed else [(look_from_columns(ref), look_from_columns(ref32), keep, None)]
        out["-".join((name, case_id(posed)) + (("f16",) if f16 else ()))] = (
            entries, "dpose_ray" if posed else "dcam_ray", PG.COLUMNS if posed else K.LOOK_FROM)
    return out


def launch(vol, tf, inps, refs_, keeps, seed=0, view_base=0, upstream=None, posed=True):
    """pose_gpu.launch for the depth march: one launch of F.march_depth_fwd + F.march_depth_bwd_pose (or _cam) over len(inps)
    views on the references' ray buffers; only the rays in `keep` whose march stops where the reference's does get an upstream
    gradient. -> per-ray (V, W, H, k) float64, totals (V, k) float64, masks (V, W, H), the upstream gradient handed in."""
    from differender_amd import functional as F
    poses, fov = PG.pose_rows(inps)
    pose = dev(poses)
    fov_v = None if fov is None else dev(fov)
    stack = lambda k, dt=torch.float32: dev(np.stack([np.asarray(r[k]) for r in refs_]), dt)
    e, x, r, n = stack("entry"), stack("exit"), stack("rays"), stack("n", torch.int32)
    cam = pose[:, :3].contiguous()
    S, sr = int(inps[0]["max_samples"]), float(inps[0]["sr"])
    out, steps = F.march_depth_fwd(vol, tf, cam, e, x, r, n, S, sr)
    got = steps.cpu().numpy()
    masks = np.stack([(got[v] == refs_[v]["steps"]) & (refs_[v]["n"] > 1) & keeps[v] for v in range(len(inps))])
    g = dev(np.stack([inps[v]["grad_out"] * masks[v][..., None] for v in range(len(inps))]))
    if upstream is not None:
        g = upstream(g)
    if posed:
        d, d_ray = F.march_depth_bwd_pose(vol, tf, pose, e, x, r, n, steps, S, sr, g, out, jitter_seed=seed, view_base=view_base,
                                          per_ray=True, fov_v=fov_v)
    else:
        d, d_ray = F.march_depth_bwd_cam(vol, tf, cam, e, x, r, n, steps, S, sr, g, out, jitter_seed=seed, view_base=view_base,
                                         per_ray=True)
    torch.cuda.synchronize()
    return d_ray.double().cpu().numpy(), d.double().cpu().numpy(), masks, g


def one(inp, ref, ref32, posed, f16=False, upstream=None, keep=None):
    """launch for one view -> (ray (W,H,k), total (k,), mask (W,H), the upstream gradient handed in)."""
    keep = PG.keep(ref, ref32) if keep is None else keep
    ray, total, mask, g = launch(*upload(inp, f16), [inp], [ref], [keep], int(inp["jitter_seed"]), int(inp["view"]), upstream,
                                 posed)
    return ray[0], total[0], mask[0], g
