"""Depth moments, DESIGN.md D18, without a GPU: the C ABI and its argument checks, the float64 transliteration
(tests/depth_reference.py) against central differences, the conditions every camera case of the GPU files owes the conditioned
pass, the premises of the edge scenes (test_gpu_depth_edges.py) and three mutations their rules must reject, the two torch
helpers, and the module's argument checks."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import camgrad_gpu as K  # noqa: E402
import depth_gpu as DG  # noqa: E402
import depth_reference as DR  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_march_depth_fwd", "dr_march_depth_bwd", "dr_march_depth_bwd_cam", "dr_march_depth_bwd_pose")


# --- 1. the C ABI -----------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    assert N.lib().dr_abi_version() == 9   # the entries are additive
    for name in ENTRIES:
        params = _header_params(name)
        assert hasattr(raw, name)
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
                    ctypes.c_float if p.startswith("float") else ctypes.c_double if p.startswith("double") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)
    # dr_march_fwd's volume, TF and ray arguments (everything up to sampling_rate), then out, steps, stream / the tails of the
    # RGBA camera entries (which have the channel stride where these have the table's three arguments)
    march, cam, pose = (_header_params(n) for n in ("dr_march_fwd", "dr_march_rgba_bwd_cam", "dr_march_rgba_bwd_pose"))
    head = march[:march.index("float sampling_rate") + 1]
    fwd, bwd, dcam, dpose = (_header_params(n) for n in ENTRIES)
    assert fwd[:len(head)] == head and len(fwd) == len(head) + 3 == len(march) - 6
    assert bwd[:len(head)] == head and bwd[-1] == "void *stream"
    rename = lambda ps: [p.replace("out_rgba", "out_moments") for p in ps]   # (the forward's image is not a colour here)
    assert dcam == head + rename(cam[cam.index("float sampling_rate") + 1:]) and len(dcam) == len(cam) + 2
    assert dpose == head + rename(pose[pose.index("float sampling_rate") + 1:]) and len(dpose) == len(pose) + 2


def _args(b, which, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, tf=b.p[1], R=8, tvs=0, cam=b.p[2], entry=b.p[3],
             exit=b.p[4], rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0)
    if which == "fwd":
        a.update(out=b.p[7], steps=None)
    elif which == "bwd":
        a.update(go=b.p[7], out=b.p[7], dvol=None, dsx=0, dsy=0, dsz=0, dvs=0, dtf=None, dtvs=0)
    else:
        a.update(fov=math.radians(30.0), near=0.1, seed=0, base=0, steps=b.p[6], go=b.p[7], out=b.p[7])
        if which == "pose":
            a.update(pose=b.p[2], fov_v=None)
        a.update(d=b.p[1], d_ray=None)
    a.update(stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null tf": dict(tf=None), "null cam": dict(cam=None), "null entry": dict(entry=None),
    "null exit": dict(exit=None), "null rays": dict(rays=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7),
    "views 0": dict(V=0), "W 0": dict(W=0), "H -1": dict(H=-1), "VX 1": dict(VX=1), "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0),
    "R 0": dict(R=0), "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0),
    "sampling rate < 0": dict(sr=-1.0), "sampling rate inf": dict(sr=float("inf")), "sampling rate nan": dict(sr=float("nan")),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    bad = INVALID[case]
    assert hiplib.dr_march_depth_fwd(*_args(b, "fwd", **bad)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd", dvol=b.p[0], dtf=b.p[1], **bad)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd", **bad)) == -1   # (checked before "nothing requested")
    assert hiplib.dr_march_depth_bwd_cam(*_args(b, "cam", **bad)) == -1
    assert hiplib.dr_march_depth_bwd_pose(*_args(b, "pose", **bad)) == -1


def test_missing_outputs_return_einval_and_nothing_requested_returns_0(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_depth_fwd(*_args(b, "fwd", out=None)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd", dvol=b.p[0], go=None)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd", dtf=b.p[1], out=None)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd", dtf=b.p[1], dtvs=6)) == -1
    assert hiplib.dr_march_depth_bwd(*_args(b, "bwd")) == 0   # d_vol == NULL && d_tf == NULL: nothing to do, no HIP call
    for entry in ("cam", "pose"):
        fn = getattr(hiplib, "dr_march_depth_bwd_" + entry)
        for bad in (dict(steps=None), dict(go=None), dict(out=None), dict(d=None), dict(near=0.0), dict(fov=0.0)):
            assert fn(*_args(b, entry, **bad)) == -1, (entry, bad)
    assert hiplib.dr_march_depth_bwd_pose(*_args(b, "pose", pose=None)) == -1


# --- 2. the reference checks itself -------------------------------------------------------------------------------------------

POSE10 = ("look_from", "look_at", "up", "fov_rad")


def _small_case():
    inp = DG.PG.inputs("a_orbit_sr1", WH=(6, 5), **DG.POSE)
    rng = np.random.RandomState(5)
    inp["vol"] = np.clip(rng.uniform(0.0, 1.0, (10, 9, 11)), 0.0, 1.0)
    inp["tf"] = rng.uniform(0.05, 0.95, (6, 4))
    inp["tf"][:, 3] = np.linspace(0.02, 0.2, 6)
    return inp


def test_transliteration_autograd_meets_central_differences():
    """One 10x9x11 case in float64: autograd equals central differences (step 1e-6, relative tolerance 1e-6 of the largest
    entry) for a handful of d_vol entries, every d_tf alpha entry and the ten pose columns; the d_tf colour columns are
    exactly 0."""
    inp = _small_case()
    ref = DR.run_case(inp)
    n = ref["n"]
    assert (n > 1).sum() > 15
    bufs = [ref[k][None] for k in ("entry", "exit", "rays")] + [n[None]]
    cam, g = inp["look_from"][None], inp["grad_out"][None]
    S, sr = int(inp["max_samples"]), float(inp["sr"])
    res = DR.run(inp["vol"], inp["tf"], cam, *bufs, g, S, sr)
    assert np.abs(res["moments"][0] - ref["rgba"]).max() <= 1e-12 and (res["moments"][..., 2] == 0).all()
    loss = lambda vol, tf: float((DR.run(vol, tf, cam, *bufs, g, S, sr, want_grad=False)["moments"] * g).sum())
    h = 1e-6
    dvol, dtf = res["dvol"], res["dtf"]
    assert (dtf[:, :3] == 0).all() and np.abs(dtf[:, 3]).min() > 0
    big = np.abs(dvol).max()
    for k in np.argsort(-np.abs(dvol).ravel())[:5]:
        idx = np.unravel_index(k, dvol.shape)
        vp, vm = inp["vol"].copy(), inp["vol"].copy()
        vp[idx] += h; vm[idx] -= h
        fd = (loss(vp, inp["tf"]) - loss(vm, inp["tf"])) / (2 * h)
        assert abs(fd - dvol[idx]) <= 1e-6 * big, (idx, fd, dvol[idx])
    big = np.abs(dtf).max()
    for k in range(dtf.shape[0]):
        tp, tm = inp["tf"].copy(), inp["tf"].copy()
        tp[k, 3] += h; tm[k, 3] -= h
        fd = (loss(inp["vol"], tp) - loss(inp["vol"], tm)) / (2 * h)
        assert abs(fd - dtf[k, 3]) <= 1e-6 * big, (k, fd, dtf[k, 3])

    # the ten pose columns: the objective with n and the live counts frozen by the references' own predicates
    def pose_loss(**over):
        r = DR.run_case(dict(inp, **over))
        assert np.array_equal(r["n"], n) and np.array_equal(r["steps"], ref["steps"])
        return float((r["rgba"] * inp["grad_out"]).sum())

    d, col = ref["dpose"], 0
    for key in POSE10:
        base = np.atleast_1d(np.asarray(inp[key], np.float64))
        for k in range(base.size):
            p, m = base.copy(), base.copy()
            p[k] += h; m[k] -= h
            sh = (lambda a: a) if key != "fov_rad" else (lambda a: a[0])
            fd = (pose_loss(**{key: sh(p)}) - pose_loss(**{key: sh(m)})) / (2 * h)
            scale = np.abs(d[PG_SLICES[key]]).max()
            assert abs(fd - d[col]) <= 1e-6 * scale, (key, k, fd, d[col])
            col += 1
    assert col == 10


PG_SLICES = {"look_from": slice(0, 3), "look_at": slice(3, 6), "up": slice(6, 9), "fov_rad": slice(9, 10)}


# --- 3. the conditions of the GPU file's camera cases -----------------------------------------------------------------------------

CONDITIONED = DG.conditioned_entries()


@pytest.mark.parametrize("case", sorted(CONDITIONED))
def test_camera_cases_meet_the_conditions_of_the_conditioned_pass(case):
    """Every camera case of test_gpu_depth.py and (edge-...) of test_gpu_depth_edges.py keeps 80 % of its n > 1 rays in the conditioned pass, and the float32
    transliteration's error over them is within the rule's floor: from the references alone."""
    entries, key, columns = CONDITIONED[case]
    K.check_conditions(entries(), key, columns, lit=False)


EDGE_FORWARD = DG.edge_forward_keys()


@pytest.mark.parametrize("key", EDGE_FORWARD, ids=[DG.edge_id(k) for k in EDGE_FORWARD])
def test_edge_scenes_keep_their_premises(key):
    """Every forward scene of test_gpu_depth_edges.py on the references' own ray buffers: the two transliterations agree on
    KEEP of the n > 1 rays (reference_state's mask), and the scene still exercises what it is there for (check_premise: the
    clip and termination counts, zero and out-of-range samples, the sample counts). The planes' scenes have axial rays."""
    inp, ref, ref32 = DG.edge_refs(key)
    live = ref["n"] > 1
    assert (DG.PG.keep(ref, ref32) & live).sum() >= DG.KEEP * live.sum() > 0
    DG.check_premise(key, inp, ref["entry"], ref["exit"], ref["rays"], ref["n"], ref["steps"])
    if key[1] in ("i_on_x_axis", "g_plane_y0"):
        assert DG.axial_rays(ref).sum() > 0
    if key[0] == "tiny":   # live rays and non-zero gradients in every one
        assert np.abs(ref["dpose_ray"][..., :3]).max() > 0


def test_edge_cases_stand_on_the_table_tiers_they_name():
    DG.table_tiers()
    for how in DG.BATCH_KINDS:   # a batched launch: three views, jitter on, view_base 5, tables or volumes of their own
        inps = [DG.edge_inputs(k) for k in DG.batch_keys(how, True)]
        assert [int(i["view"]) for i in inps] == [5, 6, 7] and all(int(i["jitter_seed"]) != 0 for i in inps)
        own = "tf" if how == "tables" else "vol"
        assert all(np.abs(inps[a][own] - inps[b][own]).max() > 0.01 for a in range(3) for b in range(a))
        assert all(np.array_equal(inps[0][k], i[k]) for i in inps for k in ("vol", "tf") if k != own)


def test_the_edge_rules_reject_plausible_mutations():
    """Arrays in the kernel's place, as test_the_conditioned_rule_rejects_a_one_percent_error feeds them: the float32
    transliteration passes each rule and a plausible mistake does not. A camera gradient 1 % too large under the max_samples
    clip; d_tf shifted by one texel at R = 9793; view 1's pose gradient computed with view 0's table."""
    from light_gpu import bound
    for posed in (False, True):
        _, ref, ref32 = DG.edge_refs(DG.variant("c_clip", posed))
        key = "dpose_ray" if posed else "dcam_ray"
        r64, r32 = (ref, ref32) if posed else (DG.look_from_columns(ref), DG.look_from_columns(ref32))
        for mask in (DG.PG.keep(ref, ref32) & (ref["n"] > 1), DG.good_rays(ref, ref32, posed)):
            m = mask[..., None]
            DG.rule(r32[key] * m, (r32[key] * m).sum((0, 1)), ref, ref32, mask, posed)
            wrong = 1.01 * r64[key] * m
            with pytest.raises(AssertionError):
                DG.rule(wrong, wrong.sum((0, 1)), ref, ref32, mask, posed)

    inp, ref, _ = DG.edge_refs(DG.variant("d_jitter", table=("ramp", DG.CAM_TABLE_R[1])))
    args = (inp["vol"], inp["tf"], inp["look_from"][None], *(ref[k][None] for k in ("entry", "exit", "rays", "n")),
            inp["grad_out"][None], int(inp["max_samples"]), float(inp["sr"]))
    d64, d32 = DR.run(*args)["dtf"][:, 3], DR.run(*args, dtype=torch.float32)["dtf"][:, 3]
    bound(d32, d64, d32, "dtf alpha, the float32 transliteration")
    with pytest.raises(AssertionError):
        bound(np.roll(d64, 1), d64, d32, "dtf alpha, one texel on")

    keys = DG.batch_keys("tables", True)
    inp1, ref, ref32 = DG.edge_refs(keys[1])
    wrong = DR.run_case(dict(inp1, tf=DG.edge_inputs(keys[0])["tf"]))["dpose_ray"]
    for mask in (DG.PG.keep(ref, ref32) & (ref["n"] > 1), DG.good_rays(ref, ref32, True)):
        m = mask[..., None]
        with pytest.raises(AssertionError):
            DG.rule(wrong * m, (wrong * m).sum((0, 1)), ref, ref32, mask, True)


# --- 4. expected_depth and depth_variance -----------------------------------------------------------------------------------------

def test_expected_depth_and_variance_are_the_closed_forms():
    from differender_amd.depth import depth_variance, expected_depth
    g = torch.Generator().manual_seed(1)
    w = torch.rand((2, 5, 4, 3), generator=g, dtype=torch.float64) * 0.3      # per-sample weights T op
    t = 1.0 + 2.0 * torch.rand((2, 5, 4, 3), generator=g, dtype=torch.float64)   # per-sample distances
    w[:, :, 0, 0] = 0.0   # a ray that collected nothing
    m = torch.stack([(w * t).sum(1), (w * t * t).sum(1), w.sum(1)], 1)       # (2, 3, 4, 3)
    a = w.sum(1)
    hit = a > 1e-6
    mean = (w * t).sum(1)[hit] / a[hit]
    var = (w * (t - ((w * t).sum(1) / a.clamp(min=1e-30))[:, None]) ** 2).sum(1)[hit] / a[hit]
    d, v = expected_depth(m, background=7.5), depth_variance(m)
    assert d.shape == v.shape == (2, 4, 3)
    assert torch.allclose(d[hit], mean, rtol=1e-12, atol=0) and bool((d[~hit] == 7.5).all()) and int((~hit).sum()) == 2
    assert torch.allclose(v[hit], var, rtol=1e-9, atol=1e-12) and bool((v[~hit] == 0).all()) and bool((v >= 0).all())
    assert bool((expected_depth(m)[~hit] == 0).all())
    # A <= eps is background, whatever M1 holds; un-batched moments work alike
    m1 = torch.tensor([[[3.0, 1e-7]], [[10.0, 1e-7]], [[1.0, 1e-6]]], dtype=torch.float64)
    assert expected_depth(m1, background=-1.0).tolist() == [[3.0, -1.0]]
    assert expected_depth(m1, eps=1e-7).tolist() == [[3.0, pytest.approx(0.1)]]
    assert depth_variance(m1).tolist() == [[1.0, 0.0]]
    with pytest.raises(ValueError):
        expected_depth(torch.zeros(4, 5, 5))
    with pytest.raises(ValueError):
        depth_variance(torch.zeros(5, 5))


def test_expected_depth_and_variance_pass_gradcheck():
    from differender_amd.depth import depth_variance, expected_depth
    g = torch.Generator().manual_seed(2)
    w = torch.rand((6, 3, 2), generator=g, dtype=torch.float64) * 0.3
    t = 1.0 + 2.0 * torch.rand((6, 3, 2), generator=g, dtype=torch.float64)
    w[:, 0, 0] = 0.0   # background: a zero gradient, not a NaN
    m = torch.stack([(w * t).sum(0), (w * t * t).sum(0), w.sum(0)], 0).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: expected_depth(x, background=2.0), (m,))
    assert torch.autograd.gradcheck(depth_variance, (m,))
    (expected_depth(m).sum() + depth_variance(m).sum()).backward()
    assert bool(torch.isfinite(m.grad).all()) and bool((m.grad[:, 0, 0] == 0).all()) and float(m.grad.abs().max()) > 0


# --- 5. the module ----------------------------------------------------------------------------------------------------------------

def test_depth_raycaster_rejects_malformed_inputs(hiplib):
    from differender_amd.depth import DepthRaycaster
    for bad in (((8, 8), (16, 16), 8), ((8, 8, 8), (16,), 8), ((8, 8, 8), (16, 16), 0)):
        with pytest.raises(ValueError):
            DepthRaycaster(*bad)
    with pytest.raises(ValueError):
        DepthRaycaster((8, 8, 8), (16, 16), 8, max_samples=0)
    rc = DepthRaycaster((8, 9, 10), (16, 16), 8, jitter=False)
    vol, tf, lf = torch.zeros(1, 8, 9, 10), torch.zeros(4, 8), torch.tensor([0.0, 0.0, 3.0])
    for bad in ((torch.zeros(8, 9, 10), tf, lf), (torch.zeros(4, 8, 9, 10), tf, lf), (torch.zeros(1, 10, 9, 8), tf, lf),
                (vol, torch.zeros(8, 4), lf), (vol, torch.zeros(4, 9), lf), (vol, torch.zeros(8), lf),
                (vol, tf, torch.zeros(2)), (vol, tf, torch.zeros(1, 1, 3)),
                (torch.zeros(2, 1, 8, 9, 10), tf, torch.zeros(3, 3)), (vol, torch.zeros(2, 4, 8), torch.zeros(3, 3))):
        with pytest.raises(ValueError):
            rc(*bad)
    with pytest.raises(ValueError, match="built for"):
        rc(torch.zeros(1, 8, 9, 11), tf, lf)
    with pytest.raises(ValueError):
        rc(vol, tf, lf, look_at=torch.zeros(2))
    # camera tensors that require grad are refused without camera_grad=True
    for name in ("look_from", "look_at", "up", "fov"):
        cam = dict(look_from=lf.clone(), look_at=torch.zeros(3), up=torch.tensor([0.0, 1.0, 0.0]), fov=torch.tensor(30.0))
        cam[name].requires_grad_(True)
        with pytest.raises(ValueError, match=name):
            rc(vol, tf, cam.pop("look_from"), **cam)
