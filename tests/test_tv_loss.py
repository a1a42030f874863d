"""The 3-D total-variation regulariser without a GPU: tv3d against a float64 NumPy loop for every norm; a float64
restatement of the gather-form gradient the backward kernel implements against torch.autograd of tv3d; the C ABI declares,
exports and signs the entry points and rejects bad arguments before any HIP call; fused_tv3d_loss has no CPU path."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from differender_amd.utils import fused_tv3d_loss, tv3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dr_tv3d_fwd", "dr_tv3d_bwd")
NORMS = [("l1", 1e-3), ("iso", 1e-3), ("iso", 1e-1), ("sq", 1e-3)]
SHAPES = [(1, 1, 1, 1), (1, 1, 2, 3), (3, 1, 4), (1, 5, 1, 7), (2, 1, 3, 4, 5), (1, 6, 5, 4), (2, 3, 1, 1)]


def _np_tv(v, norm, eps):
    """Sum of the per-voxel terms, one voxel at a time (float64)."""
    v = np.asarray(v, dtype=np.float64)
    *lead, D, H, W = v.shape
    flat = v.reshape(-1, D, H, W)
    total = 0.0
    for b, z, y, x in itertools.product(range(flat.shape[0]), range(D), range(H), range(W)):
        c = flat[b, z, y, x]
        dz = flat[b, min(z + 1, D - 1), y, x] - c
        dy = flat[b, z, min(y + 1, H - 1), x] - c
        dx = flat[b, z, y, min(x + 1, W - 1)] - c
        if norm == "l1":
            total += abs(dz) + abs(dy) + abs(dx)
        elif norm == "sq":
            total += dz * dz + dy * dy + dx * dx
        else:
            total += np.sqrt(dz * dz + dy * dy + dx * dx + eps * eps)
    return total


def _volume(shape, seed=0, flat=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g, dtype=torch.float64)
    if flat:   # constant regions and exact ties: "l1" meets sign(0)
        v = (v * 3).floor() / 3
    return v


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("norm,eps", NORMS)
def test_tv3d_matches_a_numpy_loop(shape, norm, eps):
    v = _volume(shape, seed=len(shape))
    want = _np_tv(v.numpy(), norm, eps)
    got_sum = float(tv3d(v, norm, eps, reduction="sum"))
    got_mean = float(tv3d(v, norm, eps))
    assert got_sum == pytest.approx(want, rel=1e-12, abs=1e-14)
    assert got_mean == pytest.approx(want / v.numel(), rel=1e-12, abs=1e-16)


def test_tv3d_leading_axes_are_separate_volumes():
    a, b = _volume((1, 4, 5, 6), 1), _volume((1, 4, 5, 6), 2)
    both = torch.stack([a, b])   # (2, 1, 4, 5, 6)
    for norm in ("l1", "iso", "sq"):
        s = tv3d(both, norm, reduction="sum")
        assert float(s) == pytest.approx(float(tv3d(a, norm, reduction="sum") + tv3d(b, norm, reduction="sum")), rel=1e-13)


def test_tv3d_float32_and_errors():
    v = _volume((1, 5, 6, 7), 3)
    assert float(tv3d(v.float(), "iso")) == pytest.approx(float(tv3d(v, "iso")), rel=1e-5)
    with pytest.raises(ValueError):
        tv3d(v[0, 0], "l1")
    with pytest.raises(ValueError):
        tv3d(v, "l2")
    with pytest.raises(ValueError):
        tv3d(v, "iso", eps=0.0)
    with pytest.raises(ValueError):
        tv3d(v, "l1", reduction="max")


def _flux(v, norm, eps):
    """f_a of every voxel (float64): sign(d_a), d_a / r or 2 d_a, for the axes (D, H, W)."""
    d = [torch.diff(v, dim=a, append=v.narrow(a, v.shape[a] - 1, 1)) for a in (-3, -2, -1)]
    if norm == "l1":
        return [torch.sign(t) for t in d]
    if norm == "sq":
        return [2 * t for t in d]
    r = torch.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2 + eps * eps)
    return [t / r for t in d]


def _gather_grad(v, norm, eps, scale):
    """g(p) = scale * (sum_a f_a(p - e_a) - sum_a f_a(p)); f_a(p - e_a) left out at the first voxel along a. This is the
    formula of tv3d_bwd_kernel, restated voxel-parallel."""
    f = _flux(v, norm, eps)
    g = -(f[0] + f[1] + f[2])
    for k, a in enumerate((-3, -2, -1)):
        n = v.shape[a]
        if n > 1:
            g.narrow(a, 1, n - 1).add_(f[k].narrow(a, 0, n - 1))
    return scale * g


@pytest.mark.parametrize("shape", SHAPES + [(1, 9, 8, 7)])
@pytest.mark.parametrize("norm,eps", NORMS)
@pytest.mark.parametrize("flat", [False, True])
def test_gather_gradient_matches_autograd(shape, norm, eps, flat):
    v = _volume(shape, seed=7, flat=flat).requires_grad_(True)
    for reduction in ("sum", "mean"):
        v.grad = None
        (2.5 * tv3d(v, norm, eps, reduction)).backward()
        scale = 2.5 / (v.numel() if reduction == "mean" else 1)
        want = _gather_grad(v.detach(), norm, eps, scale)
        assert float((v.grad - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_header_declares_the_tv_entry_points():
    text = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", text), name
    assert re.search(r"DR_TV_L1\s*=\s*0,\s*DR_TV_ISO\s*=\s*1,\s*DR_TV_SQ\s*=\s*2", text)


def test_library_exports_and_native_signs_the_tv_entry_points(hiplib):
    from differender_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES, name
    assert len(N.SIGNATURES["dr_tv3d_fwd"][1]) == 11 and len(N.SIGNATURES["dr_tv3d_bwd"][1]) == 15
    assert (N.DR_TV_L1, N.DR_TV_ISO, N.DR_TV_SQ) == (0, 1, 2)
    assert hiplib.dr_abi_version() == 9


def test_exports():
    import differender_amd.utils as U
    from differender_amd import functional as F
    assert U.tv3d is tv3d and U.fused_tv3d_loss is fused_tv3d_loss
    assert "tv3d_fwd" in F.__all__ and "tv3d_bwd" in F.__all__


def _call(lib, bwd, **kw):
    strides = (ctypes.c_int64 * 4)(8 * 8 * 8, 64, 8, 1)
    a = dict(vol=16, dtype=0, B=1, D=8, H=8, W=8, strides=strides, norm=0, eps=1e-3, sum=16, scale=1.0, grad=16,
             gstrides=strides)
    a.update(kw)
    head = (a["vol"], a["dtype"], a["B"], a["D"], a["H"], a["W"], a["strides"], a["norm"], a["eps"])
    if bwd:
        return lib.dr_tv3d_bwd(*head, None, a["scale"], a["grad"], a["gstrides"], 0, None)
    return lib.dr_tv3d_fwd(*head, a["sum"], None)


BAD = [dict(vol=None), dict(strides=None), dict(B=0), dict(D=0), dict(H=-1), dict(W=0), dict(dtype=2), dict(dtype=-1),
       dict(norm=3), dict(norm=-1), dict(eps=float("nan")), dict(eps=float("inf")), dict(norm=1, eps=0.0),
       dict(norm=1, eps=-1e-3), dict(norm=1, eps=1e-30), dict(norm=1, eps=2.0 ** -75)]   # (the last two: eps^2 is 0 in float32)


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_return_einval(hiplib, bad, bwd):
    assert _call(hiplib, bwd, **bad) == -1


@pytest.mark.parametrize("bad", [dict(sum=None)])
def test_bad_forward_arguments(hiplib, bad):
    assert _call(hiplib, False, **bad) == -1


@pytest.mark.parametrize("bad", [dict(grad=None), dict(gstrides=None), dict(scale=float("nan")), dict(scale=float("inf"))])
def test_bad_backward_arguments(hiplib, bad):
    assert _call(hiplib, True, **bad) == -1


def test_iso_eps_whose_square_float32_drops_and_gradient_buffer_layouts():
    """The argument rules that need no GPU: "iso" turns down an eps whose square is 0 in float32 (2^-75 squared is the tie that
    rounds to 0) and takes one whose square is subnormal; `out` may have gaps but no two voxels on one element."""
    from differender_amd import functional as F
    v = torch.rand(1, 4, 5, 6)
    for eps in (0.0, -1e-3, 1e-30, 2.0 ** -75):
        with pytest.raises(ValueError):
            F.tv3d_fwd(v, "iso", eps)
        with pytest.raises(ValueError):
            F.tv3d_bwd(v, norm="iso", eps=eps)
    for norm, eps in (("iso", 1e-20), ("iso", 2.7e-23), ("l1", 0.0), ("sq", 1e-30)):
        assert F._tv_config(norm, eps)[1] == eps
    buf = torch.zeros(4, 5, 8)
    for ok in (buf[..., :6], buf[:, ::2], buf.permute(2, 0, 1), buf[..., 1:7].permute(1, 2, 0)):
        assert F._disjoint(ok)
    for bad in (buf[:1].expand(3, 5, 8), buf.as_strided((4, 5, 6), (6, 1, 1)), buf.as_strided((4, 5, 6), (29, 6, 1))):
        assert not F._disjoint(bad)


def test_restated_plan_stands_on_the_kernels_constants():
    """tests/tv_gpu.py restates tv_loss.hip's launch plan for test_gpu_tv_edges.py to assert its premises against: the constants
    are read from the source here, so one that moves fails this test instead of leaving the edge cases on another path; and the
    chunk cases' premises hold without a GPU."""
    import test_gpu_tv_edges as E
    import tv_gpu as T
    src = open(os.path.join(ROOT, "differender_amd", "csrc", "tv_loss.hip")).read()
    got = {k: int(v) for k, v in re.findall(r"\b(NT|VX|TX|TY|TARGET_BLOCKS|ZMIN) = (\d+)", src)}
    assert got == dict(NT=T.NT, VX=T.VX, TX=T.TX, TY=T.TY, TARGET_BLOCKS=T.TARGET_BLOCKS, ZMIN=T.ZMIN)
    for shape, want in E.CHUNKS.items():
        p = T.plan_of(torch.empty(shape))
        assert (p.tiles, p.want, p.zc, p.chunks) == want, shape
    # the alignment rule: x of stride 1, the other strides multiples of 4 unless the axis has extent 1, the pointer on 4 elements
    assert T.aligned4(16, 4, (0, 1, 72, 1296), (1, 61, 18, 20)) and not T.aligned4(16, 4, (0, 1, 70, 1260), (1, 68, 18, 20))
    assert T.aligned4(8, 2, (0, 1, 72, 1296), (1, 61, 18, 20)) and not T.aligned4(4, 2, (0, 1, 72, 1296), (1, 61, 18, 20))
    assert T.aligned4(16, 4, (0, 1, 70, -1296), (1, 3, 1, 20)) and not T.aligned4(16, 4, (0, -1, 72, 1296), (1, 61, 18, 20))


def test_fused_loss_has_no_cpu_path():
    v = torch.rand(1, 4, 5, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_tv3d_loss(v)
    with pytest.raises(TypeError):
        fused_tv3d_loss(v.double())
    with pytest.raises(ValueError):
        fused_tv3d_loss(torch.rand(4, 5))
