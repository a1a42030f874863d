"""The differentiable light and Phong material, DESIGN.md D17, without a GPU: the float64 transliteration
(tests/light_reference.py) against the reference program at the reference's lighting and against central differences, the
masking rule on every scene of the GPU tests, RaycasterLit's argument checks, and the C ABI's."""
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
    W, H = sc["WH"]
    bufs = [oracle.ray_setup(c, W, H, sc["vol"].shape, sr=sc["sr"], jitter_seed=sc["jitter"], view=v, dtype=np.float64)
            for v, c in enumerate(sc["cam"])]
    inp = LC.inputs(sc, *(np.stack([b[k] for b in bufs]) for k in range(4)))
    mask, f64 = LC.kept_rays(sc, inp)
    n, S = inp["n"], sc["max_samples"]
    if name == "ert_opaque":
        assert (f64["steps"] < np.minimum(n, S))[mask].any()
    if name == "clip_S23":
        assert (n > S)[mask].any() and (f64["steps"][mask] <= S).all()
    assert (f64["rgba"][mask][:, 3] > 0).all()


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
