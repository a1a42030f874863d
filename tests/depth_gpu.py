"""What the tests of the depth march share (test_depth.py, test_gpu_depth.py, test_gpu_depth_edges.py): the
scenes of the camera-gradient fixture's cases (make_camgrad_golden.make_inputs, rounded to what the kernels read), one forward
on the kernels' own ray buffers with the float64 / float32 transliterations (tests/depth_reference.py) run on those buffers,
the camera cases with their references on the references' buffers, one launch of the camera kernels over one view or several,
and the edge cases with their premises. The bars are imported: light_gpu.bound,
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
    """Case `name` on the device: forward_state_of its scene."""
    return forward_state_of(scene(name, f16), f16)


def forward_state_of(inp, f16=False):
    """A scene on the device: F.ray_setup's buffers, F.march_depth_fwd on them and reference_state on those buffers.
    -> dict(inp, vol, tf, cam, rays (entry, exit, rays, n), out, steps, st, S, sr)."""
    from differender_amd import functional as F
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


def small_scene(R=8, views=1, per_view=False, seed=0):
    """A 10x9x11 volume under a 12x10 image: numpy inputs rounded to float32 (vol [V,]VX,VY,VZ, tf [V,]R,4, cams (V,3), g)."""
    rng = np.random.RandomState(100 + seed)
    lead = (views,) if per_view else ()
    vol = PG.F32(np.clip(0.5 + 0.25 * rng.standard_normal(lead + (10, 9, 11)), 0.0, 1.0))
    tf = rng.uniform(0.05, 0.95, lead + (R, 4))
    tf[..., 3] = np.linspace(0.02, 0.3, R) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, lead + (R,)))
    cams = PG.F32(np.array([(2.2, 1.1, 1.7), (-1.6, 1.3, 2.0), (0.4, -2.1, 1.9)][:views]))
    return vol, PG.F32(tf), cams, PG.F32(rng.standard_normal((views, 12, 10, 4)))


def small_state(vol, tf, cams, g, S=512, sr=1.0, seed=0, device_vol=None):
    """forward_state for small_scene: device tensors, the kernels' buffers and forward, reference_state on them. device_vol: the
    tensor the kernels read instead of the dense upload of `vol` (a view of other strides or another dtype with vol's values)."""
    from differender_amd import functional as F
    dvol, dtf, cam = dev(vol) if device_vol is None else device_vol, dev(tf), dev(cams)
    rays = F.ray_setup(cam, (12, 10), vol.shape[-3:], sr, jitter_seed=seed)
    out, steps = F.march_depth_fwd(dvol, dtf, cam, *rays, S, sr)
    e, x, r, n = rays
    st = reference_state(vol, tf, cams, C(e), C(x), C(r), n.cpu().numpy(), g, S, sr, steps.cpu().numpy())
    return dict(vol=dvol, tf=dtf, cam=cam, rays=rays, out=out, steps=steps, st=st, S=S, sr=sr)


def raw_bwd(fs, go, d_vol, d_tf):
    """dr_march_depth_bwd on the caller's own output buffers (functional.march_depth_bwd allocates zeroed ones); shared inputs."""
    from differender_amd import _native as N
    from differender_amd import functional as F
    cam, V, W, H, rargs = F._ray_args(fs["vol"], fs["cam"], *fs["rays"])
    rc = N.lib().dr_march_depth_bwd(*F._vol_args(fs["vol"], V), *F._tf_args(fs["tf"], V), *rargs, fs["S"], fs["sr"], go.data_ptr(),
                                    fs["out"].data_ptr(), d_vol.data_ptr(), *d_vol.stride(), 0, d_tf.data_ptr(), 0,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()


# ---- the edge cases (test_gpu_depth_edges.py; their premises without a GPU: test_depth.py) ---------------------------------------
# A case is a hashable key: ("variant", name, posed, sr, S, table) -- scene(name) with the sampling rate, max_samples or the
# table replaced (None: the scene's own; table: ("ramp", R) or "opaque") --, ("tiny", volume shape, image, R, posed), or
# ("view", kind, v, posed) -- view v of a batched launch (BATCH_KINDS). edge_inputs(key) is what depth_reference.run_case reads.

LDS_BYTES, CAM_RED_BYTES = 159 * 1024, 6144                  # dr_tile.h's LDS_PER_CU, march_depth.hip's DEPTH_RED_BYTES
CAM_TABLE_R = (9792, 9793)                                   # the camera kernel's last R in LDS, its first R in global memory
FULLEST_R = (3392, 10176)                                    # the last R of the backward's tiers 2 and 1
RATES = tuple(float(np.float32(s)) for s in (0.6, 3.0, 4.0))  # (0.6 as the kernels read it)
CLIP_ERT = dict(sr=2.0, S=80)                                # c_clip at rate 2 under an opaque table: clips and terminates
FROZEN = ("m_object_in_air", "n_out_of_range", "i_on_x_axis", "g_plane_y0")
TINY = (((2, 2, 2), (8, 8), 2), ((5, 7, 3), (3, 5), 1), ((13, 12, 14), (1, 1), 4), ((10, 9, 11), (9, 17), 8))
BATCH_KINDS = ("tables", "f16vols")                          # one shared volume + per-view tables; per-view f16 volumes
BATCH_BASE, BATCH_VIEWS = 5, 3
FEW_SAMPLES = (1, 2)


def variant(name, posed=False, sr=None, S=None, table=None):
    return ("variant", name, posed, sr, S, table)


def ramp_alpha(R):
    """A smooth alpha ramp with ripple, so neighbouring texels differ."""
    x = np.linspace(0.0, 1.0, R)
    return 0.5 * (0.05 + 0.95 * x) * (1.0 + 0.3 * np.sin(37.0 * x))


def opaque_alpha(R):
    return np.linspace(0.0, 0.9, R) ** 2 + 0.05   # (make_camgrad_golden's "opaque")


def _batch_cameras():
    return PG.F32(np.array([(2.3, 1.0, 1.6), (-1.7, 1.2, 2.1), (0.5, -2.2, 1.8)]))


@functools.lru_cache(maxsize=None)
def edge_inputs(key):
    """An edge case's scene as depth_reference.run_case reads it (shared: nobody writes to it)."""
    kind = key[0]
    if kind == "variant":
        _, name, posed, sr, S, table = key
        inp = dict(scene(name, False, posed))
        if sr is not None:
            inp["sr"] = np.float64(sr)
        if S is not None:
            inp["max_samples"] = np.int32(S)
        if table is not None:
            R = table[1] if isinstance(table, tuple) else inp["tf"].shape[0]
            tf = np.random.RandomState(R).uniform(0.05, 0.95, (R, 4))
            tf[:, 3] = ramp_alpha(R) if isinstance(table, tuple) else opaque_alpha(R)
            inp["tf"] = PG.F32(tf)
        return inp
    if kind == "tiny":
        _, vshape, WH, R, posed = key
        rng = np.random.RandomState(sum(vshape) * 10 + R)
        tf = rng.uniform(0.05, 0.95, (R, 4))
        tf[:, 3] = np.linspace(0.3, 0.05, R) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, R))
        inp = dict(vol=np.clip(0.5 + 0.25 * rng.standard_normal(vshape), 0.0, 1.0), tf=tf, look_from=np.array((2.2, 1.1, 1.7)),
                   grad_out=rng.standard_normal((*WH, 4)), sr=np.float64(1.0), max_samples=np.int32(512),
                   jitter_seed=np.int64(0), view=np.int32(0), **(POSE if posed else {}))
        return {k: PG.F32(v) if k in ("vol", "tf", "grad_out", *PG.POSE_KEYS) else v for k, v in inp.items()}
    _, how, v, posed = key
    assert kind == "view" and how in BATCH_KINDS
    inp = dict(scene("d_jitter", False, posed))   # jitter on, early termination
    rng = np.random.RandomState(40 + v)
    inp.update(look_from=_batch_cameras()[v], view=np.int32(BATCH_BASE + v), grad_out=PG.F32(rng.standard_normal(inp["grad_out"].shape)))
    if how == "tables":
        tf = inp["tf"].copy()
        tf[:, 3] = opaque_alpha(len(tf)) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, len(tf)))
        inp["tf"] = PG.F32(tf)
    else:
        inp["vol"] = PG.F16(np.clip(inp["vol"] + 0.05 * rng.standard_normal(inp["vol"].shape), 0.0, 1.0))
    return inp


@functools.lru_cache(maxsize=None)
def edge_refs(key):
    """(inputs, float64 reference, float32 reference) of an edge case, on the references' own ray buffers."""
    inp = edge_inputs(key)
    return inp, DR.run_case(inp), DR.run_case(inp, dtype=torch.float32)


def edge_id(key):
    return "-".join(case_id(k) if isinstance(k, (str, bool)) else "x".join(map(str, k)) if isinstance(k, tuple) else format(k, "g")
                    for k in key[1:] if k is not None)


def is_posed(key):
    return key[{"variant": 2, "tiny": 4, "view": 3}[key[0]]]


def batch_keys(how, posed):
    return [("view", how, v, posed) for v in range(BATCH_VIEWS)]


def edge_camera_keys():
    """Every camera case of test_gpu_depth_edges.py, fixed and posed."""
    keys = []
    for posed in (False, True):
        keys += [variant("d_jitter", posed, table=("ramp", R)) for R in CAM_TABLE_R]
        keys += [variant("c_clip", posed), variant("c_clip", posed, table="opaque", **CLIP_ERT)]
        keys += [variant(name, posed, sr=sr) for name in ("b_sr2_ert", "d_jitter") for sr in RATES]
        keys += [variant(name, posed) for name in FROZEN]
        keys += [k for how in BATCH_KINDS for k in batch_keys(how, posed)]
        keys += [("tiny", vshape, WH, R, posed) for vshape, WH, R in TINY]
        keys += [variant("b_sr2_ert", posed, S=S) for S in FEW_SAMPLES]
    return keys


def edge_forward_keys():
    """Every scene test_gpu_depth_edges.py runs forward + volume / TF backward on the kernels' own buffers (forward_state_of
    sets the fixed camera's rays up: the keys are the unposed ones)."""
    keys = [variant("d_jitter", table=("ramp", R)) for R in CAM_TABLE_R] + [variant("c_clip", table="opaque", **CLIP_ERT)]
    keys += [variant(name, sr=sr) for name in ("b_sr2_ert", "d_jitter") for sr in RATES] + [variant(name) for name in FROZEN]
    return keys + [("tiny", vshape, WH, R, False) for vshape, WH, R in TINY] + [variant("b_sr2_ert", S=S) for S in FEW_SAMPLES]


def table_tiers():
    """The arithmetic of dr_tile.h's table_tier that the R of the edge cases stand on: if a constant moves, a test says so
    instead of running one tier twice."""
    lo, hi = CAM_TABLE_R
    assert hi == lo + 1 and 16 * lo + CAM_RED_BYTES <= LDS_BYTES < 16 * hi + CAM_RED_BYTES   # camera: the table beside 6 KiB
    assert 48 * FULLEST_R[0] <= LDS_BYTES < 48 * (FULLEST_R[0] + 1)                          # backward: table + double table
    assert 16 * FULLEST_R[1] <= LDS_BYTES < 16 * (FULLEST_R[1] + 1)                          # backward and forward: the table
    assert FULLEST_R[1] > hi                                                                  # (the camera's boundary is its own)


def axial_rays(ref):
    """The n > 1 rays of a reference with a direction component of exactly 0."""
    return (ref["rays"] == 0).any(-1) & (ref["n"] > 1)


def check_premise(key, inp, e, x, r, n, steps):
    """What an edge scene is there for, asserted on one view's ray buffers ((W,H[,3]) arrays) and live counts -- the kernels'
    on the GPU, the references' without one. -> march_counts."""
    S = int(inp["max_samples"])
    c = march_counts(n, steps, S)
    live = n > 1
    assert c["live"] > 0
    if key[0] == "tiny":
        assert inp["vol"].shape == key[1] and n.shape == key[2] and inp["tf"].shape == (key[3], 4)
        return c
    _, name, _, sr, few, table = key
    if isinstance(table, tuple):    # the camera kernel's boundary: jitter as view 2, early termination, a table of distinct texels
        assert inp["tf"].shape == (table[1], 4) and (np.diff(inp["tf"][:, 3]) != 0).mean() > 0.99   # (all but a ripple's crests)
        assert int(inp["jitter_seed"]) != 0 and int(inp["view"]) == 2 and c["early"] > 100
    if name == "c_clip":
        assert c["clipped"] > 20 and (c["early"] > 20 if table == "opaque" else c["early"] == 0), c
    if sr is not None and table is None:
        assert sr in RATES and c["live"] > 100 and (c["early"] > 20 or sr < 1), c
    if few is not None and table is None:
        assert (steps[live] == few).all() and (n[live] > 2).sum() > 100   # (S = 2: the second sample is not at the exit)
    if name in ("m_object_in_air", "n_out_of_range"):
        I, on, cell = sample_values(inp["vol"], inp["look_from"], e, x, r, n, steps)
        if name == "m_object_in_air":
            zero = on & (I == 0)
            assert zero.any(0).sum() > 20 and deep_air(inp["vol"], cell, zero).sum() > 20
        else:
            print("samples below 0:", int((on & (I < 0)).sum()), "above 1:", int((on & (I > 1)).sum()))
            assert (on & ((I < 0) | (I > 1))).any()   # the lookup clamps them
    return c


def march_counts(n, steps, S):
    """Of the n > 1 rays: how many there are, how many stop at the max_samples clip and how many terminate early."""
    live = n > 1
    return dict(live=int(live.sum()), clipped=int((live & (n > S) & (steps == S)).sum()),
                early=int((live & (steps < np.minimum(n, S))).sum()))


def sample_values(vol, look_from, e, x, r, n, steps):
    """The float64 intensity of every live sample of a view's march on the given ray buffers ((W,H[,3]) arrays) and the low
    corner of its cell: I (S, P), live (S, P), cell (S, P, 3) -- make_autograd_golden's positions and tap."""
    import make_autograd_golden as G
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    v, cam = T(vol), T(look_from)
    e, x, r = T(e).reshape(-1), T(x).reshape(-1), T(r).reshape(-1, 3)
    n, steps = torch.from_numpy(np.asarray(n).reshape(-1)).long(), torch.from_numpy(np.asarray(steps).reshape(-1)).long()
    shape = torch.tensor(v.shape, dtype=torch.float64)
    I, live, cell = [], [], []
    for s in range(int(steps.max())):
        on = (s < steps) & (n > 1)
        pos = G.sample_pos(cam, e, x, r, n, s, on)
        I.append(G.sample_volume_trilinear(v, pos))
        live.append(on)
        cell.append(torch.floor(torch.clamp(0.5 * pos + 0.5, 0.0, 1.0) * (shape - 1.0 - 1e-4)).long())
    return torch.stack(I).numpy(), torch.stack(live).numpy(), torch.stack(cell).numpy()


def deep_air(vol, cell, on):
    """The voxels that are corners of a cell of `cell[on]` and have nothing but exact zeros around them (themselves and their 26
    neighbours): whichever cell a float32 program puts a sample in, a sample that scatters to such a voxel read eight zeros."""
    vol = np.asarray(vol)
    pad = np.pad(vol != 0, 1, mode="edge")
    X, Y, Z = vol.shape
    busy = np.zeros(vol.shape, bool)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                busy |= pad[dx:dx + X, dy:dy + Y, dz:dz + Z]
    touched = np.zeros(vol.shape, bool)
    c = cell[on]
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                touched[np.minimum(c[:, 0] + dx, X - 1), np.minimum(c[:, 1] + dy, Y - 1), np.minimum(c[:, 2] + dz, Z - 1)] = True
    return touched & ~busy


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
    cases = [("-".join((name, case_id(posed)) + (("f16",) if f16 else ())), posed, functools.partial(camera_refs, name, posed, f16))
             for name, posed, f16 in CAMERA_CASES]
    cases += [("edge-" + edge_id(key), is_posed(key), functools.partial(edge_refs, key)) for key in edge_camera_keys()]
    for cid, posed, refs_ in cases:
        def entries(posed=posed, refs_=refs_):
            _, ref, ref32 = refs_()
            keep = PG.keep(ref, ref32)
            return [(ref, ref32, keep, None)] if posed else [(look_from_columns(ref), look_from_columns(ref32), keep, None)]
        assert cid not in out, cid
        out[cid] = (entries, "dpose_ray" if posed else "dcam_ray", PG.COLUMNS if posed else K.LOOK_FROM)
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


def many(vol, tf, inps, refs_, refs32, posed, keeps=None):
    """launch for the views of one batched launch: view v's jitter is drawn as view inps[0]["view"] + v of the hash, so its
    reference is the case with that view. vol, tf: the device tensors, shared or one item per view.
    -> (ray (V,W,H,k), total (V,k), mask (V,W,H))."""
    base = int(inps[0]["view"])
    assert all(int(i["view"]) == base + v and int(i["jitter_seed"]) == int(inps[0]["jitter_seed"]) for v, i in enumerate(inps))
    keeps = [PG.keep(r, r32) for r, r32 in zip(refs_, refs32)] if keeps is None else keeps
    return launch(vol, tf, inps, refs_, keeps, int(inps[0]["jitter_seed"]), base, None, posed)[:3]


def both_passes(key, f16=False, columns_nonzero=False):
    """An edge case's camera (or pose) gradient by its rule over the kept rays, then over good_rays. -> the first pass's
    (ray, total, mask)."""
    inp, ref, ref32 = edge_refs(key)
    posed, what = is_posed(key), edge_id(key)
    first = one(inp, ref, ref32, posed, f16)[:3]
    rule(*first[:2], ref, ref32, first[2], posed, what)
    if columns_nonzero:
        for name, sl in (PG.COLUMNS if posed else K.LOOK_FROM):
            assert np.abs(first[0][..., sl]).max() > 0, (what, name)
    ray, total, mask, _ = one(inp, ref, ref32, posed, f16, keep=good_rays(ref, ref32, posed, what))
    rule(ray, total, ref, ref32, mask, posed, (what, "conditioned"))
    return first
