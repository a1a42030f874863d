"""X-ray line-integral and maximum intensity projections without a GPU: the float64 transliteration against
central differences and the chord length, the C ABI's argument checks, Projector's shape checks; the reference's helpers for
tests/test_gpu_projection_edges.py (sample_at, window_plan, layout_volume) and that file's case tables: the window paths, the
clipping and the compared shares each case is there for."""
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


# ---- the reference's helpers for tests/test_gpu_projection_edges.py and that file's choice of cases ----------------------------

CG = PR.CG   # tests/golden/make_camgrad_golden.py: the transliterated ray setup


@pytest.mark.parametrize("case", sorted(CASES))
def test_sample_at_the_argmax_is_the_maximum(case):
    vshape, (W, H), sr, S, seed, cp = CASES[case]
    vol = _volume(vshape, 21, lo=-0.4).detach()
    cam = _cam(*cp)
    out, arg, (e, x, r, n) = PR.project_camera(vol, cam, W, H, sr, S, "max", jitter_seed=seed, view=1)
    assert (arg >= 0).any()
    assert torch.equal(PR.sample_at(vol, cam, e, x, r, n, arg), out)
    # any other sample of a ray is no larger, an earlier one is smaller; the gap of project_top2 is that to the runner-up
    best, arg2, gap = PR.project_top2(vol, cam, e, x, r, n, S)
    assert torch.equal(best, out) and torch.equal(arg2, arg)
    m = torch.where(n > 1, torch.clamp(n, max=S if S is not None else 1 << 30), torch.zeros_like(n))
    runner_up = torch.full_like(out, -math.inf)
    for s in range(int(m.max())):
        v = PR.sample_at(vol, cam, e, x, r, n, torch.full_like(n, s))
        live = s < m
        assert (v[live] <= out[live]).all() and (v[live & (s < arg)] < out[live & (s < arg)]).all()
        runner_up = torch.where(live & (s != arg), torch.maximum(runner_up, v), runner_up)
    assert torch.equal(gap, out - runner_up) and (gap[arg >= 0] >= 0).all()
    # differentiable in the volume: the 8 trilinear weights of one sample sum to 1 per live ray
    v = vol.clone().requires_grad_(True)
    PR.sample_at(v, cam, e, x, r, n, arg).sum().backward()
    assert abs(float(v.grad.sum()) - int((arg >= 0).sum())) <= 1e-9 * W * H


def test_window_constants_are_read_from_the_kernel_source():
    K = PR.window_constants()
    assert set(K) == {"PW_TILE", "PW_BOX", "PW_WIN_VOX", "PW_MIN_VOX"}
    assert K["PW_TILE"] == 16 and K["PW_BOX"] * 4 <= 64 * 1024 and K["PW_WIN_VOX"] > K["PW_MIN_VOX"] >= 1


def _plan(case):
    """window_plan over the case's views on float32 rays of the transliterated ray setup, and the clipped share of live rays."""
    W, H = case["WH"]
    total, clipped = np.zeros(5, dtype=np.int64), []
    for v, c in enumerate(case["cams"]):
        e, x, r, n = CG.ray_setup(torch.tensor(c, dtype=torch.float32), W, H, case["vshape"], case["sr"], case["fov"], 0.1,
                                  case["seed"], v)
        total += np.array(PR.window_plan(c, e, x, r, n, case["vshape"], case["S"], W, H))
        if case["S"] is not None:
            clipped.append(float((n[n > 1] > case["S"]).float().mean()))
    return PR.WindowPlan(*(int(t) for t in total)), clipped


def test_edge_cases_reach_the_window_paths_they_claim():
    claimed = {}
    for name, case in PR.EDGE_CASES.items():
        plan, clipped = _plan(case)
        windows = plan.lds_full + plan.lds_halved + plan.fallback
        for path in case["paths"]:
            count = getattr(plan, path)
            assert count >= 3 and count >= 0.05 * windows, (name, path, plan)
            claimed.setdefault(path, set()).add(case["dtype"])
        if case.get("dead_tiles"):
            assert plan.dead_tiles >= 1 and plan.live_tiles >= 1, (name, plan)
        assert all(c > 1 / 3 for c in clipped), (name, clipped)
        W, H = case["WH"]
        assert W % 16 and H % 16 and W > 32 and H > 32, name   # 3 x 3 tiles or more, the last ones partly filled
    for path in ("lds_full", "lds_halved", "fallback"):
        assert claimed.get(path) == {torch.float32, torch.float16}, (path, claimed.get(path))
    cases = PR.EDGE_CASES.values()
    assert {c["layout"] for c in cases} == {"x", "y", "z", "strided"}
    assert sum(c["S"] is not None for c in cases) >= 2 and sum(c["dtype"] == torch.float16 for c in cases) >= 2
    assert any(c["S"] is not None and c["dtype"] == torch.float16 for c in cases)
    assert any(c["S"] is not None and "lds_halved" in c["paths"] for c in cases)
    assert any(c["own"] and len(c["cams"]) == 3 and c["seed"] for c in cases)
    assert any(max(c["vshape"]) >= 3 * min(c["vshape"]) for c in cases)
    assert any(max(abs(v) for v in c["cams"][0]) < 1 for c in cases)   # a camera inside the box


def test_window_plan_counts_a_single_tile_by_hand():
    # one ray along z through the middle of a 40^3 volume: 39 voxels of depth in windows of 16 -> 3 windows, a 2x2xN box each
    vs = (40, 40, 40)
    e, x = np.full((1, 1), 1.0, np.float32), np.full((1, 1), 3.0, np.float32)
    r = np.array([[[0.0, 0.0, -1.0]]], np.float32)
    plan = PR.window_plan([0.01, 0.01, 2.0], e, x, r, np.array([[40]]), vs, None, 1, 1)
    assert plan == PR.WindowPlan(3, 0, 0, 0, 1), plan
    assert PR.window_plan([0.01, 0.01, 2.0], e, x, r, np.array([[1]]), vs, None, 1, 1) == PR.WindowPlan(0, 0, 0, 1, 0)
    # clipped to 10 samples: the walk still covers the depth range, only the first window has samples
    assert PR.window_plan([0.01, 0.01, 2.0], e, x, r, np.array([[40]]), vs, 10, 1, 1) == PR.WindowPlan(1, 0, 0, 0, 1)


def test_layout_volume_keeps_values_and_gives_the_strides():
    vals = torch.rand(2, 5, 6, 7)
    for v in (vals, vals[0]):
        for layout, unit in (("z", -1), ("x", -3), ("y", -2), ("strided", None)):
            t = PR.layout_volume(v, layout)
            assert t.shape == v.shape and torch.equal(t, v), layout
            assert all(s != 1 for s in t.stride()) if unit is None else t.stride(unit) == 1
    t = PR.layout_volume(vals[0], "strided")
    assert torch.zeros_like(t, memory_format=torch.preserve_format).stride() != t.stride()


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("name", sorted(PR.CAM_CASES))
def test_camera_cases_keep_nine_rays_in_ten(name, mode):
    """The share of rays on which the GPU test compares d look_from per ray: those whose sample count (and argmax) the float64
    and the float32 program agree on. Also the clipping the "clipped" case is there for."""
    case = PR.CAM_CASES[name]
    W, H = case["WH"]
    for v, c in enumerate(case["cams"]):
        vol = PR.case_values(case, 8, lo=-0.3 if mode == "max" else 0.0)
        res = {}
        for dt in (F64, torch.float32):
            _, a, (_, _, _, n) = PR.project_camera(vol.to(dt), torch.tensor(c, dtype=dt), W, H, case["sr"], case["S"], mode,
                                                   fov_deg=case["fov"], jitter_seed=case["seed"], view=case["view_base"] + v)
            res[dt] = (n, a)
        same = res[F64][0] == res[torch.float32][0]
        if mode == "max":
            same &= res[F64][1] == res[torch.float32][1]
        assert same.float().mean() >= 0.9, (name, v, float(same.float().mean()))
        n = res[F64][0]
        assert (n > 1).any()
        if case["S"] is not None:
            assert (n[n > 1] > case["S"]).float().mean() > 1 / 3
    if name == "odd_missed":
        assert W % 8 and H % 8 and (n == 0).any()


@pytest.mark.parametrize("name", sorted(PR.MIP_CASES))
def test_mip_cases_have_a_clear_maximum_on_most_rays(name):
    """The share of live rays whose float64 top-two gap exceeds 1e-4 of the image's scale: where the GPU test asks the
    kernel's arg_max to equal the reference's exactly."""
    case = PR.MIP_CASES[name]
    W, H = case["WH"]
    V = len(case["cams"])
    vols = PR.case_values(case, 11, V if case["own"] else None, lo=-0.3).double()
    for v, c in enumerate(case["cams"]):
        cam = torch.tensor(c, dtype=F64)
        e, x, r, n = CG.ray_setup(cam, W, H, case["vshape"], case["sr"], case["fov"], 0.1, case["seed"], v)
        best, arg, gap = PR.project_top2(vols[v] if case["own"] else vols, cam, e, x, r, n, case["S"])
        live = arg >= 0
        assert live.sum() >= 50
        assert (gap[live] > 1e-4 * float(best.abs().max())).float().mean() >= 0.95, (name, v)
        if case["S"] is not None:
            assert (n[live] > case["S"]).float().mean() > 1 / 3
