"""X-ray line-integral and maximum intensity projections without a GPU: the float64 transliteration against
central differences and the chord length, the C ABI's argument checks, Projector's shape checks."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proj_reference as PR  # noqa: E402

ENTRIES = ("dr_project_fwd", "dr_project_bwd", "dr_project_bwd_cam")
F64 = torch.float64


def _volume(shape, seed, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + torch.rand(shape, generator=g, dtype=F64)).requires_grad_(True)


def _cam(theta, phi, r):
    return torch.tensor([r * math.cos(phi) * math.sin(theta), r * math.sin(phi), r * math.cos(phi) * math.cos(theta)], dtype=F64)


# name: volume shape, image, sampling rate, max_samples, jitter seed, camera
CASES = {
    "orbit": ((7, 6, 8), (5, 4), 1.0, None, 0, (0.7, 0.3, 2.6)),
    "jitter_sr2": ((6, 7, 5), (4, 5), 2.0, None, 977, (2.1, -0.4, 3.1)),
    "clipped": ((8, 8, 8), (4, 4), 1.3, 9, 0, (4.0, 0.2, 2.4)),
}


def _objective(vol, cam, case, mode, grad):
    vshape, (W, H), sr, S, seed, _ = CASES[case]
    out, _, _ = PR.project_camera(vol, cam, W, H, sr, S, mode, jitter_seed=seed, view=1)
    return (out * grad).sum()


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_transliteration_gradients_match_central_differences(case, mode):
    vshape, (W, H), sr, S, seed, cp = CASES[case]
    vol = _volume(vshape, 3 + sorted(CASES).index(case))
    cam = _cam(*cp).requires_grad_(True)
    grad = torch.randn(W * H, generator=torch.Generator().manual_seed(5), dtype=F64)
    _objective(vol, cam, case, mode, grad).backward()
    h = 1e-6
    rng = np.random.RandomState(0)
    with torch.no_grad():
        flat = vol.view(-1)
        for k in rng.choice(flat.numel(), 12, replace=False):
            old = float(flat[k])
            flat[k] = old + h; fp = float(_objective(vol, cam, case, mode, grad))
            flat[k] = old - h; fm = float(_objective(vol, cam, case, mode, grad))
            flat[k] = old
            assert abs((fp - fm) / (2 * h) - float(vol.grad.view(-1)[k])) <= 1e-6 * (1 + abs(fp - fm) / (2 * h)), (k,)
        for a in range(3):
            e = torch.zeros(3, dtype=F64); e[a] = h
            fp = float(_objective(vol, cam + e, case, mode, grad))
            fm = float(_objective(vol, cam - e, case, mode, grad))
            fd = (fp - fm) / (2 * h)
            assert abs(fd - float(cam.grad[a])) <= 1e-5 * (1 + abs(fd)), (a, fd, float(cam.grad[a]))


@pytest.mark.parametrize("seed", [0, 1234])
def test_constant_volume_gives_the_chord_length(seed):
    c = 0.37
    vol = torch.full((9, 7, 8), c, dtype=F64)
    for cp in ((0.3, 0.2, 2.7), (1.9, -0.5, 0.4)):   # the second camera sits inside the box
        out, _, (e, x, r, n) = PR.project_camera(vol, _cam(*cp), 6, 5, 1.0, None, "sum", jitter_seed=seed)
        ok = n >= 2
        assert ok.any()
        torch.testing.assert_close(out[ok], c * (x - e)[ok], rtol=1e-12, atol=1e-12)
        assert (out[~ok] == 0).all()


def test_max_takes_the_first_maximum_and_gives_zero_without_samples():
    vol = torch.full((6, 6, 6), -0.25, dtype=F64)
    e = torch.tensor([-1.0, 0.0, -1.0]); x = torch.tensor([1.0, 1.0, 1.0])
    r = torch.tensor([[0.0, 0.0, 1.0]] * 3, dtype=F64); n = torch.tensor([5, 0, 1])
    cam = torch.tensor([0.1, 0.2, 0.0], dtype=F64)
    out, arg = PR.project(vol, cam, e.double(), x.double(), r, n, None, "max")
    assert out.tolist() == [-0.25, 0.0, 0.0] and arg.tolist() == [0, -1, -1]   # all equal: the first sample wins


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_library_and_signatures_agree(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        params = _header_params(name)
        assert hasattr(raw, name)
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
                    ctypes.c_double if p.startswith("double") else ctypes.c_float if p.startswith("float") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)


class _Bufs:
    """Host memory standing in for the device buffers: the argument checks run before any HIP call."""

    def __init__(self):
        self.keep = [(ctypes.c_float * 4096)() for _ in range(10)]
        self.p = [ctypes.addressof(b) for b in self.keep]


def _common(b):
    return dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, cam=b.p[2], entry=b.p[3], exit=b.p[4],
                rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, mode=0)


def _fwd_args(b, **kw):
    a = _common(b); a.update(out=b.p[7], arg=b.p[8], stream=None); a.update(kw)
    return list(a.values())


def _bwd_args(b, **kw):
    a = _common(b)
    a.update(go=b.p[7], arg=b.p[8], dvol=b.p[9], dsx=64, dsy=8, dsz=1, dvs=0, variant=0, stream=None); a.update(kw)
    return list(a.values())


def _cam_args(b, **kw):
    a = _common(b)
    a.update(fov=0.5, near=0.1, seed=0, vbase=0, go=b.p[7], arg=b.p[8], dcam=b.p[9], dray=None, stream=None); a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null cam": dict(cam=None), "null entry": dict(entry=None), "null exit": dict(exit=None),
    "null rays": dict(rays=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7), "views 0": dict(V=0),
    "views 65536": dict(V=65536), "W 0": dict(W=0), "H -1": dict(H=-1), "VX 1": dict(VX=1), "VZ 0": dict(VZ=0),
    "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-3), "mode 2": dict(mode=2), "mode -1": dict(mode=-1),
    "max without arg_max": dict(mode=1, arg=None),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    assert hiplib.dr_project_fwd(*_fwd_args(b, **INVALID[case])) == -1
    assert hiplib.dr_project_bwd(*_bwd_args(b, **INVALID[case])) == -1
    assert hiplib.dr_project_bwd_cam(*_cam_args(b, **INVALID[case])) == -1


def test_invalid_outputs_variants_and_camera_return_einval(hiplib):
    b = _Bufs()
    assert hiplib.dr_project_fwd(*_fwd_args(b, out=None)) == -1
    assert hiplib.dr_project_bwd(*_bwd_args(b, go=None)) == -1
    for v in (2, -1, 0x100):
        assert hiplib.dr_project_bwd(*_bwd_args(b, variant=v)) == -1
    assert hiplib.dr_project_bwd_cam(*_cam_args(b, go=None)) == -1
    assert hiplib.dr_project_bwd_cam(*_cam_args(b, dcam=None)) == -1
    assert hiplib.dr_project_bwd_cam(*_cam_args(b, fov=0.0)) == -1
    assert hiplib.dr_project_bwd_cam(*_cam_args(b, near=-1.0)) == -1
    # nothing requested: nothing to do, no HIP call
    assert hiplib.dr_project_bwd(*_bwd_args(b, dvol=None)) == 0
    assert hiplib.dr_project_bwd(*_bwd_args(b, dvol=None, mode=1, variant=1)) == 0


def test_projector_rejects_malformed_arguments(hiplib):
    from differender_amd.projection import Projector
    for bad in (dict(volume_shape=(8, 8)), dict(output_shape=(16,)), dict(mode="mean"), dict(max_samples=0),
                dict(sampling_rate=0.0), dict(volume_shape=(8, 1, 8)), dict(output_shape=(0, 4))):
        kw = dict(volume_shape=(8, 8, 8), output_shape=(16, 16)); kw.update(bad)
        with pytest.raises(ValueError):
            Projector(**kw)
    pj = Projector((8, 6, 7), (16, 12), jitter=False)
    vol, lf = torch.zeros(1, 8, 6, 7), torch.tensor([0.0, 0.0, 3.0])
    for v, c in ((torch.zeros(8, 6, 7), lf), (torch.zeros(2, 8, 6, 7), lf), (torch.zeros(1, 7, 6, 8), lf),
                 (torch.zeros(2, 1, 8, 6, 7), torch.zeros(3, 3)), (vol, torch.zeros(2)), (vol, torch.zeros(1, 1, 3)),
                 (torch.zeros(1, 2, 8, 6, 7), lf)):
        with pytest.raises(ValueError):
            pj(v, c)
