"""Pre-classified RGBA volumes, DESIGN.md D14, without a GPU: the float64 transliteration (tests/rgba_reference.py) against
finite differences and against the closed form of a constant volume, the C ABI and its argument checks, the module's shape
checks, and interleaved()."""
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

import rgba_reference as RR  # noqa: E402

ENTRIES = ("dr_march_rgba_fwd", "dr_march_rgba_bwd")


def _scene(vshape=(10, 9, 11), WH=(6, 5), seed=0, opaque=False, sr=1.0, angle=1.1):
    from oracle import oracle as O
    rng = np.random.RandomState(seed)
    b = np.clip(O.synth_volume(vshape, dtype=np.float64) + 0.02 * rng.standard_normal(vshape), 0.0, 1.0)
    vol = rng.uniform(0.05, 0.95, size=(4, *vshape))
    vol[3] = 0.05 + 0.9 * b ** 2 if opaque else 0.01 + 0.05 * b
    cam = O.in_circles(angle).astype(np.float64)
    e, x, r, n = O.ray_setup(cam, *WH, vshape, sr=sr, dtype=np.float64)
    g = rng.standard_normal((*WH, 4))
    return dict(vol=vol, cam=cam[None], entry=e[None], exit=x[None], rays=r[None], n=n[None], grad_out=g[None], sr=sr)


def _run(s, vol=None, S=4096, **kw):
    return RR.run(s["vol"] if vol is None else vol, s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], S, s["sr"],
                  **kw)


# --- 1. the transliteration's autograd against central differences ------------------------------------------------------------

@pytest.mark.parametrize("opaque,sr", [(False, 1.0), (True, 2.0)], ids=["thin_sr1", "opaque_sr2"])
def test_transliteration_gradient_meets_central_differences(opaque, sr):
    s = _scene(seed=3, opaque=opaque, sr=sr)
    res = _run(s)
    if opaque:
        assert (res["steps"] < s["n"])[s["n"] > 1].any()   # some rays terminate early: the frozen live count is exercised
    dvol = res["dvol"]
    big = np.abs(dvol).max()
    assert big > 0 and all(np.abs(dvol[k]).max() > 0 for k in range(4))   # every channel receives a gradient
    loss = lambda v: float((_run(s, vol=v, want_grad=False)["rgba"] * s["grad_out"]).sum())
    h = 1e-6
    # the voxels of largest gradient overall, and of each channel
    picks = np.argsort(-np.abs(dvol).ravel())[:6].tolist()
    for k in range(4):
        picks += (np.argsort(-np.abs(dvol[k]).ravel())[:2] + k * dvol[k].size).tolist()
    for k in picks:
        idx = np.unravel_index(k, dvol.shape)
        vp, vm = s["vol"].copy(), s["vol"].copy()
        vp[idx] += h; vm[idx] -= h
        fd = (loss(vp) - loss(vm)) / (2 * h)
        assert abs(fd - dvol[idx]) <= 1e-8 * big, (idx, fd, dvol[idx])


# --- 2. a constant volume ---------------------------------------------------------------------------------------------------

def test_constant_volume_has_the_closed_form():
    s = _scene(vshape=(8, 8, 8), WH=(6, 6), sr=2.0)
    c = np.array([0.7, 0.2, 0.45, 0.3])
    vol = np.broadcast_to(c[:, None, None, None], (4, 8, 8, 8)).copy()
    res = _run(s, vol=vol, want_grad=False)
    op = 1.0 - np.sqrt(1.0 - c[3])
    live = s["n"][0] > 1
    steps = res["steps"][0][live]
    assert live.sum() > 8 and steps.min() >= 2 and len(set(steps.tolist())) > 1
    assert (steps < s["n"][0][live]).any()   # A = 1 - (1 - op)^k crosses 0.99 on the long rays
    A = 1.0 - (1.0 - op) ** steps
    got = res["rgba"][0][live]
    assert np.abs(got[:, 3] - A).max() <= 1e-14
    for k in range(3):
        assert np.abs(got[:, k] - c[k] * A).max() <= 1e-14
    assert (res["rgba"][0][~live] == 0).all()


# --- 3. the C ABI -----------------------------------------------------------------------------------------------------------

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
        self.keep = [(ctypes.c_float * 4096)() for _ in range(8)]
        self.p = [ctypes.addressof(b) for b in self.keep]


def _fwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, sc=512, vs=0, cam=b.p[2], entry=b.p[3], exit=b.p[4],
             rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, mode=0, out=b.p[7], steps=None, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, sc=512, vs=0, cam=b.p[2], entry=b.p[3], exit=b.p[4],
             rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, go=b.p[7], out=b.p[7], dvol=None, dsx=0, dsy=0, dsz=0, dsc=0,
             dvs=0, stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null cam": dict(cam=None), "null entry": dict(entry=None), "null exit": dict(exit=None),
    "null rays": dict(rays=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7), "views 0": dict(V=0), "W 0": dict(W=0),
    "H -1": dict(H=-1), "VX 0": dict(VX=0), "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0), "max_samples 0": dict(S=0),
    "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0), "sampling rate < 0": dict(sr=-1.0),
    "sampling rate inf": dict(sr=float("inf")), "sampling rate nan": dict(sr=float("nan")),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    assert hiplib.dr_march_rgba_fwd(*_fwd_args(b, **INVALID[case])) == -1
    assert hiplib.dr_march_rgba_bwd(*_bwd_args(b, dvol=b.p[1], **INVALID[case])) == -1
    assert hiplib.dr_march_rgba_bwd(*_bwd_args(b, **INVALID[case])) == -1   # (checked before "nothing requested")


def test_invalid_mode_and_outputs_return_einval(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_rgba_fwd(*_fwd_args(b, mode=2)) == -1
    assert hiplib.dr_march_rgba_fwd(*_fwd_args(b, mode=-1)) == -1
    assert hiplib.dr_march_rgba_fwd(*_fwd_args(b, out=None)) == -1
    assert hiplib.dr_march_rgba_bwd(*_bwd_args(b, dvol=b.p[1], go=None)) == -1
    assert hiplib.dr_march_rgba_bwd(*_bwd_args(b, dvol=b.p[1], out=None)) == -1
    assert hiplib.dr_march_rgba_bwd(*_bwd_args(b)) == 0   # d_vol == NULL: nothing to do, no HIP call


# --- 4. the module ----------------------------------------------------------------------------------------------------------

def test_raycaster_rgba_rejects_malformed_inputs(hiplib):
    from differender_amd.rgba import RaycasterRGBA
    with pytest.raises(ValueError):
        RaycasterRGBA((8, 8), (16, 16))
    with pytest.raises(ValueError):
        RaycasterRGBA((8, 8, 8), (16,))
    with pytest.raises(ValueError):
        RaycasterRGBA((8, 8, 8), (16, 16), max_samples=0)
    rc = RaycasterRGBA((8, 9, 10), (16, 16), jitter=False)
    vol, lf = torch.zeros(4, 8, 9, 10), torch.tensor([0.0, 0.0, 3.0])
    for bad in ((torch.zeros(8, 9, 10), lf), (torch.zeros(1, 8, 9, 10), lf), (torch.zeros(3, 8, 9, 10), lf),
                (torch.zeros(4, 10, 9, 8), lf), (torch.zeros(2, 3, 8, 9, 10), lf), (torch.zeros(1, 2, 4, 8, 9, 10), lf),
                (vol, torch.zeros(2)), (vol, torch.zeros(1, 1, 3)),
                (torch.zeros(2, 4, 8, 9, 10), torch.zeros(3, 3))):   # batch sizes 2 and 3
        with pytest.raises(ValueError):
            rc(*bad)
        with pytest.raises(ValueError):
            rc.raycast_nondiff(*bad)
    with pytest.raises(ValueError, match="look_from"):
        rc(vol, lf.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="look_from"):
        rc(torch.zeros(2, 4, 8, 9, 10), torch.zeros(2, 3, requires_grad=True))


# --- 5. interleaved() -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("lead", [(), (3,)], ids=["single", "batch"])
def test_interleaved_puts_the_channel_axis_at_stride_one(lead, dtype):
    from differender_amd.rgba import interleaved
    v = torch.rand((*lead, 4, 5, 6, 7)).to(dtype)
    w = interleaved(v)
    assert w.shape == v.shape and w.dtype == v.dtype and torch.equal(w, v)
    assert w.stride(-4) == 1 and all(s % 4 == 0 for k, s in enumerate(w.stride()) if k != w.ndim - 4)
    assert interleaved(w).data_ptr() == w.data_ptr()   # already interleaved: no copy
    with pytest.raises(ValueError):
        interleaved(torch.zeros(3, 5, 6, 7))
