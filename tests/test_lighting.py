"""The differentiable light and Phong material, DESIGN.md D17, without a GPU: the float64 transliteration
(tests/light_reference.py) against the reference program at the reference's lighting and against central differences, the
masking rule on every scene of the GPU tests (and what each edge scene is for), the non-differentiable transliteration against
make_setup_nondiff_golden.raycast_nondiff, per-view inputs of the transliteration, RaycasterLit's argument checks, and the C
ABI's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import light_cases as LC  # noqa: E402
import light_reference as LR  # noqa: E402

G = LR.G
ENTRIES = ("dr_march_lit_fwd", "dr_march_lit_bwd")


# --- 1. at the reference's lighting the transliteration is make_autograd_golden.raycast ------------------------------------------

@pytest.mark.parametrize("name", ["a_sr1", "b_sr2_ert"])
def test_reference_lighting_reproduces_the_golden_raycast(name):
    z = np.load(os.path.join(HERE, "golden", f"autograd_{name}.npz"))
    inp = {k: z[k] for k in ("vol", "tf", "cam", "entry", "exit", "rays", "n", "grad_out", "sr", "max_samples")}
    want = G.run_case(inp)
    one = dict(inp, cam=inp["cam"][None], entry=inp["entry"][None], exit=inp["exit"][None], rays=inp["rays"][None], n=inp["n"][None],
               grad_out=inp["grad_out"][None])
    got = LR.run(one, LR.reference_light(inp["cam"]))
    assert (got["steps"][0] == want["steps"]).all()
    assert np.abs(got["rgba"][0] - want["rgba"]).max() <= 1e-14
    if name == "b_sr2_ert":
        assert (want["steps"] < np.minimum(inp["n"], int(inp["max_samples"])))[inp["n"] > 1].any()
    for k in ("dvol", "dtf"):
        big = np.abs(want[k]).max()
        assert big > 0 and np.abs(got[k] - want[k]).max() <= 1e-12 * big, k


# --- 2. autograd's d_light against central differences, per ray -------------------------------------------------------------------

def _small_scene(light, opaque=False, sr=1.0):
    from oracle import oracle as O
    vshape, WH = (10, 9, 11), (6, 5)
    rng = np.random.RandomState(3)
    vol = LC.synth_volume(vshape, 11)
    tf = rng.uniform(0.05, 0.95, size=(8, 4))
    tf[:, 3] = np.linspace(0.0, 0.9, 8) ** 2 + 0.05 if opaque else np.linspace(0.01, 0.06, 8)
    cam = O.in_circles(1.1).astype(np.float64)
    e, x, r, n = O.ray_setup(cam, *WH, vshape, sr=sr, dtype=np.float64)
    g = rng.standard_normal((1, *WH, 4))
    inp = dict(vol=vol, tf=tf, cam=cam[None], entry=e[None], exit=x[None], rays=r[None], n=n[None], grad_out=g, sr=sr,
               max_samples=4096)
    return inp, np.asarray(light, np.float64)[None]


@pytest.mark.parametrize("light,opaque,sr", [(LC.SIDE, False, 1.0), (LC.BRIGHT, True, 2.0), (LC.SH32, False, 1.0)],
                         ids=["side_sh7.5", "bright_opaque_sr2", "sh32"])
def test_transliteration_dlight_meets_central_differences(oracle, light, opaque, sr):
    """Per ray, every one of the ten components: |fd - autograd| <= 1e-8 of the largest per-ray gradient element, at h = 1e-6
    (the bar and the step of tests/test_rgba.py's central-difference check). Rays `near` a kink are excluded, and so are rays
    whose live count moves under the perturbation (the frozen termination). The difference between the steps h and h/2, which
    bounds the truncation error of the difference quotient, is asserted to be below the same bar, so the bar stands as it is."""
    inp, L = _small_scene(light, opaque, sr)
    res = LR.run(inp, L)
    d = res["dlight_ray"][0]
    big = np.abs(d).max()
    live = (inp["n"][0] > 1) & ~res["near"][0]
    assert live.sum() >= 0.8 * (inp["n"][0] > 1).sum() and big > 0
    assert all(np.abs(d[live][:, k]).max() > 0 for k in range(10))   # every component receives a gradient
    if opaque:
        assert (res["steps"][0] < inp["n"][0])[live].any()            # the frozen live count is exercised

    def per_ray_loss(Lp):
        r = LR.run(inp, Lp, want_grad=False)
        return (r["rgba"][0] * inp["grad_out"][0]).sum(-1), r["steps"][0]

    def quotient(k, h):
        Lp, Lm = L.copy(), L.copy()
        Lp[0, k] += h; Lm[0, k] -= h
        (fp, sp), (fm, sm) = per_ray_loss(Lp), per_ray_loss(Lm)
        return (fp - fm) / (2 * h), (sp == res["steps"][0]) & (sm == res["steps"][0])

    h = 1e-6
    for k in range(10):
        fd, same = quotient(k, h)
        fd2, same2 = quotient(k, h / 2)
        ok = live & same & same2
        assert ok.sum() >= 0.8 * (inp["n"][0] > 1).sum()
        assert np.abs(fd - fd2)[ok].max() <= 1e-8 * big, (k, np.abs(fd - fd2)[ok].max() / big)
        assert np.abs(fd - d[..., k])[ok].max() <= 1e-8 * big, (k, np.abs(fd - d[..., k])[ok].max() / big)
    assert np.abs(res["dlight"][0] - d.reshape(-1, 10).sum(0)).max() == 0


# --- 3. the masking rule keeps enough rays in every scene of the GPU tests ---------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_both_transliterations_keep_enough_rays(oracle, name):
    """tests/test_gpu_lighting.py compares on the rays light_cases.kept_rays keeps (at least 80 % of the live ones, asserted
    there): here on the oracle's float64 ray buffers, there on the kernels' float32 ones. Also what each scene is for."""
    sc = LC.scene(name)
    inp = LC.oracle_inputs(sc, oracle)
    mask, f64, _ = LC.kept_rays(sc, inp)
    n, S = inp["n"], sc["max_samples"]
    if name == "ert_opaque":
        assert (f64["steps"] < np.minimum(n, S))[mask].any()
    if name == "clip_S23":
        assert (n > S)[mask].any() and (f64["steps"][mask] <= S).all()
    assert (f64["rgba"][mask][:, 3] > 0).all()


# what each edge scene is for, asserted on the float64 transliteration so that a scene cannot quietly stop exercising its path
EARLY = {"sh_half_opaque_sr2", "nd_opaque0_sr4", "nd_overexposed"}            # kept rays stop before their last sample
BRIGHT = {"nd_thin0_no_clip", "nd_opaque0_sr4", "nd_overexposed", "nd_sh32"}  # kept rays composite samples with Lraw > 1
WITH_GRADIENTS = {"light_far", "kd_zero"}                                     # (besides the zero-column and per-view scenes)


@pytest.mark.parametrize("name", list(LC.EDGE_CASES) + list(LC.NONDIFF_CASES))
def test_edge_scenes_keep_enough_rays_and_reach_their_paths(oracle, name):
    """test_both_transliterations_keep_enough_rays for the scenes of tests/test_gpu_lighting_edges.py, the non-differentiable
    ones through the non-differentiable transliteration and its `near` (the skip threshold's band)."""
    sc = LC.scene(name)
    inp = LC.oracle_inputs(sc, oracle)
    mask, f64, f32 = LC.kept_rays(sc, inp)
    n, S, light = inp["n"], sc["max_samples"], sc["light"]
    assert (f64["rgba"][mask][:, 3] > 0).any()
    if name in EARLY:
        assert (f64["steps"] < (n if sc["nondiff"] else np.minimum(n, S)))[mask].any()
    if sc["nondiff"]:
        assert (f64["rgba"] <= 1.0).all() and (f32["rgba"] <= 1.0).all()
        # a kept ray skips a sample (alpha <= 1e-3) and composites another
        assert ((f64["skipped"] > 0) & (f64["skipped"] < f64["steps"]) & (f64["rgba"][..., 3] > 0))[mask].sum() >= 10
        if name in BRIGHT:
            assert (f64["bright"] > 0)[mask].any()                 # composited with L = Lraw > 1: nothing clamps the lighting
        if name == "nd_thin0_no_clip":
            assert (f64["steps"] > S)[mask].any() and S == 23      # no max_samples clip
        if name == "nd_overexposed":
            over = (f64["raw"][..., :3] > 1.0).any(-1) & mask
            assert over.sum() >= 10 and (f64["rgba"][over][:, :3].max(-1) == 1.0).all()   # only the final min(1, .) holds them
        if name == "nd_sh32":
            assert light[0, 9] == 32.0 and (light[0, :9] != LR.reference_light(sc["cam"])[0, :9]).all()
        if name == "nd_f16_volume":
            assert sc["f16"] and np.array_equal(sc["vol"], sc["vol"].astype(np.float16).astype(np.float64))
        if name == "nd_per_view":
            assert sc["vol"].ndim == 4 and sc["tf"].ndim == 3 and len(light) == 3
        return
    if name == "light_inside":
        assert (np.abs(light[0, :3]) < 1.0).all()                  # inside the box [-1, 1]^3 that ray_setup intersects
    if name.startswith("sh_"):
        assert light[0, 9] == {"sh_half": 0.5, "sh_half_opaque_sr2": 0.5, "sh_one": 1.0, "sh_zero": 0.0, "sh_200": 200.0}[name]
    if name in ("R2", "R6_three_views"):
        assert 48 * sc["tf"].shape[0] < 320                         # TF + double d_tf table: shorter than the reduction's scratch
    if name.startswith("image_"):
        assert mask.all() and mask.size < 64                        # every pixel is live and kept; less than one wave of them
    if not (sc["zero"] or sc["per_view"] or name in WITH_GRADIENTS):
        return
    st = LC.reference_state(sc, inp["entry"], inp["exit"], inp["rays"], n)
    ref, ref32 = st["ref"], st["ref32"]
    cols = np.abs(ref["dlight_ray"]).sum((0, 1, 2))
    for r in (ref, ref32):
        assert np.isfinite(r["dlight_ray"]).all()
        for k in range(10):
            if k in sc["zero"]:
                assert (r["dlight_ray"][..., k] == 0).all() and (r["dlight"][:, k] == 0).all(), k   # exactly, ray by ray
            else:
                assert np.abs(r["dlight_ray"][..., k]).sum() > 0, k
    if name == "light_far":
        assert cols[:3].max() < 1e-3 * cols[3:8].min()              # d p: three orders below d lc, d ka and d kd
        assert cols[:3].max() < cols[3:].min()                      # ... and the smallest column of all
    if sc["per_view"]:
        V = len(light)
        assert ref["dvol"].shape == sc["vol"].shape and ref["dtf"].shape == sc["tf"].shape
        for k in ("dvol", "dtf"):
            big = np.abs(ref[k]).max()
            assert all(np.abs(ref[k][a] - ref[k][b]).max() > 1e-3 * big for a in range(V) for b in range(a))


# --- 3b. the non-differentiable transliteration and the per-view inputs of `run` ----------------------------------------------------

def _golden_nondiff(name):
    """A committed setup_nondiff_* fixture -> (the fixture, the non-differentiable transliteration at the reference's lighting on
    the fixture's ray buffers, the rays both march). make_setup_nondiff_golden.raycast_nondiff (numpy, its own helpers)
    reproduces the fixture's image exactly. Single-sample rays are left out (H6: `run` does not march them)."""
    import make_setup_nondiff_golden as NG
    z = np.load(os.path.join(HERE, "golden", f"setup_nondiff_{name}.npz"))
    W, H = z["n"].shape
    want, live, _ = NG.raycast_nondiff(z["vol"], z["tf"], z["cam"], z["entry"].reshape(-1), z["exit"].reshape(-1),
                                       z["rays"].reshape(-1, 3), z["n"].reshape(-1).astype(np.int64), float(z["sr"]))
    assert np.array_equal(want.reshape(W, H, 4), z["rgba"]) and np.array_equal(live.reshape(W, H), z["live"])
    inp = dict(vol=z["vol"], tf=z["tf"], cam=z["cam"][None], entry=np.nan_to_num(z["entry"])[None], exit=np.nan_to_num(z["exit"])[None],
               rays=z["rays"][None], n=z["n"][None], sr=float(z["sr"]), max_samples=1)   # (max_samples is not read: no clip)
    got = LR.run(inp, LR.reference_light(z["cam"]), mode="nondiff")
    ok = z["n"] > 1
    assert ok.sum() > 100 and (got["steps"][0] == z["live"])[ok].all() and (z["live"] > 1)[ok].any()
    assert (got["raw"][0][ok] >= got["rgba"][0][ok]).all()
    return z, got, ok


def test_reference_lighting_reproduces_the_golden_raycast_nondiff():
    """At the reference's lighting the non-differentiable transliteration is make_setup_nondiff_golden.raycast_nondiff to 1e-14,
    on the fixture at rate 8 whose rays terminate early."""
    z, got, ok = _golden_nondiff("e_sr8_ert")
    assert (z["live"] < z["n"])[ok].any() and z["rgba"][ok].max() > 0.9
    assert np.abs(got["rgba"][0] - z["rgba"])[ok].max() <= 1e-14


def test_reference_lighting_skips_the_samples_the_golden_raycast_nondiff_skips():
    """The fixture whose TF has stretches of alpha 0 (none of the others skips a sample): equal live counts, and the alpha
    channel -- which holds every skip decision and nothing of the lighting -- to 1e-14. The colours are printed, not asserted
    at that bar: the two float64 programs normalise the normal and the light direction in different operation orders, r.v differs
    by an ulp or two, r.v^32 multiplies that by 32 per sample, and the colours of this fixture end 1.6e-14 apart (1.3e-14 on
    c_far_sr03, 3.0e-14 on b_aniso_sr4, 5e-15 on the other two)."""
    z, got, ok = _golden_nondiff("a_orbit_sr1")
    assert ((got["skipped"][0] > 0) & (got["skipped"][0] < got["steps"][0]))[ok].sum() > 50
    print("colour difference", np.abs(got["rgba"][0] - z["rgba"])[ok][:, :3].max())
    assert np.abs(got["rgba"][0] - z["rgba"])[ok][:, 3].max() <= 1e-14 and z["rgba"][ok][:, 3].max() > 0.5


def test_per_view_copies_of_shared_inputs_are_the_shared_run(oracle):
    """`run` with V copies of one volume and TF as per-view inputs: every view's image and per-ray d_light are the shared run's
    to the bit, each view's d_vol / d_tf is the shared run of that view alone, and they sum to the shared run's."""
    inp, L = _small_scene(LC.SIDE)
    cam2 = oracle.in_circles(2.9).astype(np.float64)
    e, x, r, n = oracle.ray_setup(cam2, 6, 5, inp["vol"].shape, sr=1.0, dtype=np.float64)
    two = lambda a, b: np.concatenate([a, b[None]])
    inp = dict(inp, cam=two(inp["cam"], cam2), entry=two(inp["entry"], e), exit=two(inp["exit"], x), rays=two(inp["rays"], r),
               n=two(inp["n"], n), grad_out=np.random.RandomState(8).standard_normal((2, 6, 5, 4)))
    L = np.stack([L[0], np.asarray(LC.VIEW_B, np.float64)])
    shared = LR.run(inp, L)
    per = LR.run(dict(inp, vol=np.stack([inp["vol"]] * 2), tf=np.stack([inp["tf"]] * 2)), L)
    assert per["dvol"].shape == (2, *inp["vol"].shape) and per["dtf"].shape == (2, 8, 4)
    for k in ("rgba", "steps", "near", "clamped", "dlight_ray", "dlight"):
        assert np.array_equal(per[k], shared[k]), k
    only = lambda v: np.arange(2)[:, None, None] == v + np.zeros((2, 6, 5), int)
    for k in ("dvol", "dtf"):
        big = np.abs(shared[k]).max()
        assert big > 0 and np.abs(per[k].sum(0) - shared[k]).max() <= 1e-13 * big, k
        for v in range(2):
            alone = LR.run(inp, L, pixels=only(v))[k]
            assert np.abs(per[k][v]).max() > 0 and np.abs(per[k][v] - alone).max() <= 1e-13 * big, (k, v)
    for mode in ("diff", "nondiff"):
        a = LR.run(inp, L, want_grad=False, mode=mode)
        b = LR.run(dict(inp, vol=np.stack([inp["vol"]] * 2), tf=np.stack([inp["tf"]] * 2)), L, want_grad=False, mode=mode)
        assert all(np.array_equal(a[k], b[k]) for k in a), mode


# --- 4. the module's argument checks, before any device call ----------------------------------------------------------------------

def test_raycaster_lit_rejects_malformed_inputs(hiplib):
    from differender_amd.lighting import RaycasterLit
    with pytest.raises(ValueError):
        RaycasterLit((8, 8), (16, 16), 8)
    with pytest.raises(ValueError):
        RaycasterLit((8, 8, 8), (16,), 8)
    with pytest.raises(ValueError):
        RaycasterLit((8, 8, 8), (16, 16), 0)
    rc = RaycasterLit((8, 9, 10), (16, 16), 8, jitter=False)
    vol, tf, lf = torch.zeros(1, 8, 9, 10), torch.zeros(4, 8), torch.tensor([0.0, 0.0, 3.0])
    shapes = ((torch.zeros(8, 9, 10), tf, lf), (torch.zeros(2, 8, 9, 10), tf, lf), (torch.zeros(1, 10, 9, 8), tf, lf),
              (vol, torch.zeros(3, 8), lf), (vol, torch.zeros(4, 9), lf), (vol, tf, torch.zeros(2)), (vol, tf, torch.zeros(1, 1, 3)),
              (torch.zeros(2, 1, 8, 9, 10), tf, torch.zeros(3, 3)))   # batch sizes 2 and 3
    for bad in shapes:
        with pytest.raises(ValueError):
            rc(*bad)
        with pytest.raises(ValueError):
            rc.raycast_nondiff(*bad)
    lighting = (dict(light_pos=torch.zeros(4)), dict(light_pos=torch.zeros(2, 2)), dict(light_color=torch.zeros(1, 1, 3)),
                dict(light_color=(1.0, 2.0)), dict(ambient=torch.zeros(2, 2)), dict(specular=torch.zeros(1, 1, 1)),
                dict(light_color=torch.zeros(2, 3), diffuse=torch.zeros(3, 1)),          # the batch rule: 2 and 3
                dict(shininess=torch.full((3,), 4.0), light_pos=torch.zeros(2, 3)),       # ... a (BS,) scalar joins it
                dict(shininess=0.0), dict(shininess=-2.0), dict(shininess=float("nan")), dict(shininess=float("inf")),
                dict(ambient=float("nan")), dict(diffuse=float("inf")), dict(specular=float("-inf")),
                dict(light_pos=(0.0, float("nan"), 1.0)), dict(light_color=float("inf")))
    for bad in lighting:
        with pytest.raises(ValueError):
            rc(vol, tf, lf, **bad)
        with pytest.raises(ValueError):
            rc.raycast_nondiff(vol, tf, lf, **bad)
    for name, kw in (("look_from", {}), ("look_at", dict(look_at=torch.zeros(3, requires_grad=True))),
                     ("up", dict(up=torch.tensor([0.0, 1.0, 0.0], requires_grad=True))),
                     ("fov", dict(fov=torch.tensor(30.0, requires_grad=True)))):
        cam = lf.clone().requires_grad_(True) if name == "look_from" else lf
        with pytest.raises(ValueError, match=r"%s.*volume_raycaster\.Raycaster" % name):
            rc(vol, tf, cam, **kw)
    # what is well-formed passes every check and stops at the first device call: there is no CPU path
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rc(vol, tf, lf, light_pos=torch.zeros(3), light_color=0.5, ambient=torch.tensor(0.2), shininess=torch.tensor([7.0]))


# --- 5. the C ABI -----------------------------------------------------------------------------------------------------------------

def _header_params(name):
    text = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


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
                    ctypes.c_float if p.startswith("float") else ctypes.c_int)
            assert a is want, (name, p, a)


class _Bufs:
    """Host memory standing in for the device buffers: the argument checks run before any HIP call."""

    def __init__(self):
        self.keep = [(ctypes.c_float * 4096)() for _ in range(10)]
        self.p = [ctypes.addressof(b) for b in self.keep]


def _fwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, tf=b.p[1], R=8, tfvs=0, cam=b.p[2], entry=b.p[3],
             exit=b.p[4], rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, light=b.p[8], mode=0, out=b.p[7], steps=None,
             stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, tf=b.p[1], R=8, tfvs=0, cam=b.p[2], entry=b.p[3],
             exit=b.p[4], rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, light=b.p[8], mode=0, go=b.p[7], out=b.p[7],
             dvol=None, dsx=0, dsy=0, dsz=0, dvs=0, dtf=None, dtfvs=0, dlight=None, dray=None, stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null tf": dict(tf=None), "null cam": dict(cam=None), "null entry": dict(entry=None),
    "null exit": dict(exit=None), "null rays": dict(rays=None), "null n": dict(n=None), "null light": dict(light=None),
    "unknown dtype": dict(dtype=7), "views 0": dict(V=0), "W 0": dict(W=0), "H -1": dict(H=-1), "VX 0": dict(VX=0),
    "VY -3": dict(VY=-3), "VZ 1": dict(VZ=1), "R 0": dict(R=0), "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0),
    "sampling rate < 0": dict(sr=-1.0), "sampling rate nan": dict(sr=float("nan")), "mode 2": dict(mode=2),
    "mode -1": dict(mode=-1),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    assert hiplib.dr_march_lit_fwd(*_fwd_args(b, **INVALID[case])) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, dlight=b.p[9], **INVALID[case])) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, **INVALID[case])) == -1   # (checked before "nothing requested")


def test_invalid_outputs_and_backward_mode_return_einval(hiplib):
    from differender_amd import _native as N
    b = _Bufs()
    assert hiplib.dr_march_lit_fwd(*_fwd_args(b, out=None)) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, dlight=b.p[9], mode=N.DR_MODE_NONDIFF)) == -1   # the backward is DIFF's
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, dlight=b.p[9], go=None)) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, dlight=b.p[9], out=None)) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b, dtf=b.p[9], dtfvs=2)) == -1
    assert hiplib.dr_march_lit_bwd(*_bwd_args(b)) == 0   # all four outputs NULL: nothing to do, no HIP call
