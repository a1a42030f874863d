"""2-D (value, gradient-magnitude) transfer functions, DESIGN.md D12, without a GPU: the C ABI and its argument checks, the
module's shape checks, the float64 transliteration (tests/tf2d_reference.py) against the 1-D one and against finite
differences, and gradient_scale."""
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
sys.path.insert(0, os.path.join(HERE, "golden"))

import tf2d_reference as R2  # noqa: E402

ENTRIES = ("dr_march_tf2d_fwd", "dr_march_tf2d_bwd")


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
                    ctypes.c_float if p.startswith("float") else ctypes.c_int)
            assert a is want, (name, p, a)


class _Bufs:
    """Host memory standing in for the device buffers: the argument checks run before any HIP call."""

    def __init__(self):
        self.keep = [(ctypes.c_float * 4096)() for _ in range(8)]
        self.p = [ctypes.addressof(b) for b in self.keep]


def _fwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, tf=b.p[1], RV=4, RG=3, tvs=0, g=1.0,
             cam=b.p[2], entry=b.p[3], exit=b.p[4], rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0, mode=0,
             out=b.p[7], steps=None, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(b, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, vs=0, tf=b.p[1], RV=4, RG=3, tvs=0, g=1.0,
             cam=b.p[2], entry=b.p[3], exit=b.p[4], rays=b.p[5], n=b.p[6], V=1, W=4, H=4, S=64, sr=1.0,
             go=b.p[7], out=b.p[7], dvol=None, dsx=0, dsy=0, dsz=0, dvs=0, dtf=None, dtvs=0, stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null tf2d": dict(tf=None), "null cam": dict(cam=None), "null entry": dict(entry=None),
    "null exit": dict(exit=None), "null rays": dict(rays=None), "null n": dict(n=None),
    "unknown dtype": dict(dtype=7), "views 0": dict(V=0), "W 0": dict(W=0), "H -1": dict(H=-1), "VX 1": dict(VX=1),
    "RV 0": dict(RV=0), "RG 0": dict(RG=0), "RV*RG 2^31": dict(RV=1 << 16, RG=1 << 15), "g_scale 0": dict(g=0.0),
    "g_scale < 0": dict(g=-1.0), "g_scale inf": dict(g=float("inf")), "g_scale nan": dict(g=float("nan")),
    "max_samples < 0": dict(S=-1), "sampling rate 0": dict(sr=0.0), "tf view stride": dict(tvs=3),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    assert hiplib.dr_march_tf2d_fwd(*_fwd_args(b, **INVALID[case])) == -1
    assert hiplib.dr_march_tf2d_bwd(*_bwd_args(b, dtf=b.p[1], **INVALID[case])) == -1


def test_invalid_mode_and_outputs_return_einval(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_tf2d_fwd(*_fwd_args(b, mode=2)) == -1
    assert hiplib.dr_march_tf2d_fwd(*_fwd_args(b, out=None)) == -1
    assert hiplib.dr_march_tf2d_bwd(*_bwd_args(b, dtf=b.p[1], go=None)) == -1
    assert hiplib.dr_march_tf2d_bwd(*_bwd_args(b, dtf=b.p[1], out=None)) == -1
    assert hiplib.dr_march_tf2d_bwd(*_bwd_args(b, dtf=b.p[1], dtvs=6)) == -1
    assert hiplib.dr_march_tf2d_bwd(*_bwd_args(b)) == 0   # nothing requested: nothing to do, no HIP call


def test_raycaster2d_rejects_malformed_shapes(hiplib):
    from differender_amd.tf2d import Raycaster2D
    with pytest.raises(ValueError):
        Raycaster2D((8, 8, 8), (16, 16), (8,), g_scale=1.0)
    with pytest.raises(ValueError):
        Raycaster2D((8, 8, 8), (16, 16), (8, 0), g_scale=1.0)
    for g in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Raycaster2D((8, 8, 8), (16, 16), (8, 4), g_scale=g)
    rc = Raycaster2D((8, 8, 8), (16, 16), (8, 4), g_scale=1.0, jitter=False)
    vol, tf, lf = torch.zeros(1, 8, 8, 8), torch.zeros(4, 8, 4), torch.tensor([0.0, 0.0, 3.0])
    for bad in ((torch.zeros(8, 8, 8), tf, lf), (torch.zeros(2, 8, 8, 8), tf, lf), (vol, torch.zeros(4, 8), lf),
                (vol, torch.zeros(3, 8, 4), lf), (vol, torch.zeros(4, 4, 8), lf), (vol, tf, torch.zeros(2)),
                (torch.zeros(2, 1, 8, 8, 8), torch.zeros(3, 4, 8, 4), lf)):
        with pytest.raises(ValueError):
            rc(*bad)
    with pytest.raises(ValueError, match="Raycaster"):
        rc(vol, tf, lf.clone().requires_grad_(True))


# --- the transliteration ----------------------------------------------------------------------------------------------------

def _scene(vshape=(10, 9, 11), WH=(5, 4), RV=6, RG=5, seed=0, thin=True, sr=1.0, g_target=1.3):
    from oracle import oracle as O
    rng = np.random.RandomState(seed)
    vol = np.clip(O.synth_volume(vshape, dtype=np.float64) + 0.05 * rng.standard_normal(vshape), 0.0, 1.0)
    tf = rng.uniform(0.05, 0.95, size=(RV, RG, 4))
    tf[..., 3] = rng.uniform(0.01, 0.08, size=(RV, RG)) if thin else rng.uniform(0.2, 0.9, size=(RV, RG))
    cam = O.in_circles(1.1).astype(np.float64)
    e, x, r, n = O.ray_setup(cam, *WH, vshape, sr=sr, dtype=np.float64)
    g = rng.standard_normal((*WH, 4))
    # g_scale: the 80th percentile of the tap length over the volume lands at u = g_target (beyond 1: samples on the clamp)
    pos = torch.from_numpy(np.random.RandomState(seed + 100).uniform(-0.9, 0.9, size=(2000, 3)))
    q = float(np.quantile(R2.taps(torch.from_numpy(vol), pos).norm(dim=1).numpy(), 0.8))
    return dict(vol=vol, tf=tf, cam=cam[None], entry=e[None], exit=x[None], rays=r[None], n=n[None], grad_out=g[None],
                g_scale=g_target / q, sr=sr)


def test_transliteration_with_one_gradient_column_is_the_1d_one():
    import make_autograd_golden as G
    s = _scene(RG=1, thin=False, sr=2.0)
    res = R2.run(s["vol"], s["tf"], s["g_scale"], s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], 4096, 2.0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    vol = T(s["vol"]).requires_grad_(True)
    tf = T(s["tf"][:, 0]).requires_grad_(True)
    live = s["n"][0].reshape(-1) > 1
    sel = torch.from_numpy(np.nonzero(live)[0])
    out, cnt = G.raycast(vol, tf, T(s["cam"][0]), T(s["entry"][0]).reshape(-1)[sel], T(s["exit"][0]).reshape(-1)[sel],
                         T(s["rays"][0]).reshape(-1, 3)[sel], T(s["n"][0].astype(np.int64)).reshape(-1)[sel], 4096, 2.0)
    (out * T(s["grad_out"][0]).reshape(-1, 4)[sel]).sum().backward()
    assert (res["steps"][0].reshape(-1)[live] == cnt.numpy()).all()
    assert cnt.sum() > 50 and (cnt.numpy() < s["n"][0].reshape(-1)[live]).any()   # some rays terminate early
    assert np.abs(res["rgba"][0].reshape(-1, 4)[live] - out.detach().numpy()).max() <= 1e-12
    assert np.abs(res["dvol"] - vol.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(vol.grad.numpy()).max())
    assert np.abs(res["dtf"][:, 0] - tf.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(tf.grad.numpy()).max())


def _loss(s, vol, tf):
    r = R2.run(vol, tf, s["g_scale"], s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], 4096, s["sr"],
               want_grad=False)
    return float((r["rgba"] * s["grad_out"]).sum())


def test_transliteration_gradients_match_finite_differences():
    s = _scene(seed=3, g_target=1.0)
    res = R2.run(s["vol"], s["tf"], s["g_scale"], s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], 4096, 1.0)
    # the march visits both sides of the gradient-axis clamp: u spread over the table and beyond its last column
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    pos = T(np.random.RandomState(0).uniform(-0.9, 0.9, size=(4000, 3)))
    u = R2.taps(T(s["vol"]), pos).norm(dim=1).numpy() * s["g_scale"]
    assert (u > 1.0).mean() > 0.01 and ((u > 0.1) & (u < 0.9)).mean() > 0.3
    dvol, dtf = res["dvol"], res["dtf"]
    assert np.abs(dtf[:, 1:]).max() > 0 and np.abs(dtf[:, -1]).max() > 0   # texels reached through u, the last column too
    # the u path of d_vol is live: the same volume gradient with a table flat along the gradient axis differs
    flat_tf = np.repeat(s["tf"][:, :1], s["tf"].shape[1], axis=1)
    res_flat = R2.run(s["vol"], flat_tf, s["g_scale"], s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], 4096,
                      1.0)
    res_flat_img = R2.run(s["vol"], flat_tf, s["g_scale"] * 0.5, s["cam"], s["entry"], s["exit"], s["rays"], s["n"],
                          s["grad_out"], 4096, 1.0, want_grad=False)
    assert np.abs(res_flat["rgba"] - res_flat_img["rgba"]).max() <= 1e-12   # (flat along u: g_scale does not matter)
    rng = np.random.RandomState(1)
    eps = 1e-6
    # voxels with the largest gradients, and random ones
    flat_idx = np.argsort(-np.abs(dvol).ravel())[:6].tolist() + rng.choice(dvol.size, 6, replace=False).tolist()
    for k in flat_idx:
        idx = np.unravel_index(k, dvol.shape)
        vp, vm = s["vol"].copy(), s["vol"].copy()
        vp[idx] += eps; vm[idx] -= eps
        fd = (_loss(s, vp, s["tf"]) - _loss(s, vm, s["tf"])) / (2 * eps)
        assert abs(fd - dvol[idx]) <= 1e-5 * max(1.0, abs(dvol[idx])), (idx, fd, dvol[idx])
    tidx = np.argsort(-np.abs(dtf).ravel())[:6].tolist() + rng.choice(dtf.size, 6, replace=False).tolist()
    for k in tidx:
        idx = np.unravel_index(k, dtf.shape)
        tp, tm = s["tf"].copy(), s["tf"].copy()
        tp[idx] += eps; tm[idx] -= eps
        fd = (_loss(s, s["vol"], tp) - _loss(s, s["vol"], tm)) / (2 * eps)
        assert abs(fd - dtf[idx]) <= 1e-5 * max(1.0, abs(dtf[idx])), (idx, fd, dtf[idx])
    assert np.abs(dvol - res_flat["dvol"]).max() > 1e-3 * np.abs(dvol).max()


def test_gradient_scale_on_a_linear_ramp():
    from differender_amd.tf2d import gradient_scale
    D, H, W = 12, 10, 17
    a = 0.05
    vol = (a * torch.arange(W, dtype=torch.float64)).expand(D, H, W)[None]   # (1, D, H, W): a ramp along x (W)
    want = 1.0 / (a * 1e-3 * (W - 1 - 1e-4))
    assert abs(gradient_scale(vol) - want) <= 1e-9 * want
    assert abs(gradient_scale(vol[0], q=0.5) - want) <= 1e-9 * want
    # along y (H) the span is that axis's
    vol_y = (a * torch.arange(H, dtype=torch.float64))[:, None].expand(D, H, W)
    assert abs(gradient_scale(vol_y) - 1.0 / (a * 1e-3 * (H - 1 - 1e-4))) <= 1e-9 / (a * 1e-3 * (H - 1))
    with pytest.raises(ValueError):
        gradient_scale(torch.zeros(4, 4, 4))
    # a batch ([BS,]1,D,H,W): each volume differenced on its own, the quantile over all of them
    for bs in (2, 3):
        assert abs(gradient_scale(vol[None].expand(bs, 1, D, H, W)) - want) <= 1e-9 * want
    vol_d = (a * torch.arange(D, dtype=torch.float64))[:, None, None].expand(D, H, W)   # a ramp along D
    want_d = 1.0 / (a * 1e-3 * (D - 1 - 1e-4))
    assert abs(gradient_scale(vol_d[None, None].expand(3, 1, D, H, W)) - want_d) <= 1e-9 * want_d
    with pytest.raises(ValueError):
        gradient_scale(torch.zeros(2, 2, 4, 4, 4))   # ([BS,]C,D,H,W) with C != 1


def test_nondiff_transliteration_with_one_gradient_column_is_the_oracle(oracle):
    """The transliteration's non-differentiable march (no max_samples clip, alpha <= 1e-3 counted but not composited,
    unclamped lighting, min(1, .) at the end) with RG = 1 against the f64 oracle's mode 1 (VR.py:308-361)."""
    s = _scene(RG=1, thin=False, sr=2.0, seed=5)
    tf = s["tf"].copy()
    tf[::3, 0, 3] = 0.0          # rows of zero alpha: samples lerp between them and live rows, across the threshold
    res = R2.run(s["vol"], tf, s["g_scale"], s["cam"], s["entry"], s["exit"], s["rays"], s["n"], s["grad_out"], 4, 2.0,
                 want_grad=False, nondiff=True)
    rgba, steps = oracle.march_fwd(s["vol"], np.ascontiguousarray(tf[:, 0]), s["cam"][0], s["entry"][0], s["exit"][0],
                                   s["rays"][0], s["n"][0], 4, 2.0, mode=1)
    live = (s["n"][0] > 1) & ~res["near"][0]
    assert live.sum() > 10 and (steps[live] > 4).any()
    assert (res["steps"][0][live] == steps[live]).all()
    assert np.abs(res["rgba"][0][live] - rgba[live]).max() <= 1e-10


def test_power_of_two_plateaus_are_flat_in_both_precisions():
    """The premise of the GPU plateau test (tests/test_gpu_tf2d_edges.py): in tf2d_reference.plateau_volume the air (0), the
    plateaus (0.25, 0.5) and the out-of-range blocks (-0.25, 2.0) give samples whose six taps cancel exactly, in float64 and in
    float32 alike, and nothing else does; a march through it meets the same flat samples in both precisions."""
    from oracle import oracle as O
    vol = R2.plateau_volume((24, 24, 24), seed=1)
    pos = np.random.RandomState(0).uniform(-1.0, 1.0, size=(20000, 3))
    flats = {}
    for dt in (torch.float64, torch.float32):
        v, p = torch.from_numpy(vol).to(dt), torch.from_numpy(pos).to(dt)
        I = R2.G.sample_volume_trilinear(v, p)
        g = R2.taps(v, p)
        flat = ((g * g).sum(1) == 0).numpy()
        I = I.double().numpy()
        on = np.zeros(len(pos), bool)
        for level, least in ((0.0, 5000), (0.25, 500), (0.5, 100), (2.0, 100), (-0.25, 100)):
            at = I == level
            on |= at
            assert (at & flat).sum() >= least, (dt, level, (at & flat).sum())
        assert not (flat & ~on).any(), dt
        flats[dt] = flat
    assert (flats[torch.float64] == flats[torch.float32]).all()
    cam = O.in_circles(0.9).astype(np.float64)
    e, x, r, n = O.ray_setup(cam, 12, 12, vol.shape, sr=1.0, dtype=np.float64)
    tf = np.random.RandomState(2).uniform(0.05, 0.95, size=(12, 7, 4))
    tf[..., 3] = 0.03
    args = (vol.astype(np.float64), tf, 40.0, cam[None], e[None], x[None], r[None], n[None], np.zeros((1, 12, 12, 4)), 4096,
            1.0)
    r64 = R2.run(*args, want_grad=False, count_flat=True)
    r32 = R2.run(*args, dtype=torch.float32, want_grad=False, count_flat=True)
    assert (r64["flat"] == r32["flat"]).all() and (r64["steps"] == r32["steps"]).all()
    live = n > 1
    assert r64["flat"][0][live].sum() >= 0.3 * r64["steps"][0][live].sum()
    assert (r64["flat"][0][live] < r64["steps"][0][live]).mean() > 0.5   # and most rays meet structure as well
