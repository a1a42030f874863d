"""The RGBA march over ray bundles, DESIGN.md D21, without a GPU: the three C entries and their argument checks, the float64
reference (tests/rgba_bundle_reference.py) against central finite differences of itself, the conditions every case of the GPU
file (tests/test_gpu_rgba_bundle.py) owes its comparisons, from the references alone, and the module's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import bundle_reference as BR  # noqa: E402
import camgrad_gpu as K  # noqa: E402
import rgba_bundle_reference as RB  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_march_rgba_bundle_fwd", "dr_march_rgba_bundle_bwd", "dr_march_rgba_bundle_bwd_rays")
INF = float("inf")


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
                    ctypes.c_float if p.startswith("float") else ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)
    # the three marches share their head, up to sampling_rate: the D19 entries' with the RGBA volume's sc in the table's place
    fwd, bwd, rays = (_header_params(n) for n in ENTRIES)
    head = fwd[:fwd.index("float sampling_rate") + 1]
    assert bwd[:len(head)] == head and rays[:len(head)] == head
    d19 = _header_params("dr_march_bundle_fwd")
    assert [p for p in head if p != "int64_t sc"] == [p for p in d19[:len(head) + 1] if p not in ("const float *tf", "int R")]
    assert all(ps[-1] == "void *stream" for ps in (fwd, bwd, rays))
    assert rays[len(head):] == _header_params("dr_march_bundle_bwd_rays")[len(head) + 1:]


def _args(b, which, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, sc=512, origins=b.p[2], dirs=b.p[5], entry=b.p[3],
             exit=b.p[4], n=b.p[6], N=16, S=64, sr=1.0)
    if which == "fwd":
        a.update(out=b.p[7], steps=None)
    elif which == "bwd":
        a.update(go=b.p[7], out=b.p[7], dvol=None, dsx=0, dsy=0, dsz=0, dsc=0)
    else:
        a.update(steps=b.p[6], t_near=-INF, seed=0, base=0, go=b.p[7], out=b.p[7], d_o=b.p[0], d_d=b.p[1])
    a.update(stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null origins": dict(origins=None), "null dirs": dict(dirs=None),
    "null entry": dict(entry=None), "null exit": dict(exit=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7),
    "N 0": dict(N=0), "N -5": dict(N=-5), "N 2^31": dict(N=2 ** 31), "N 2^40": dict(N=2 ** 40), "VX 1": dict(VX=1),
    "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0), "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-1),
    "sampling rate 0": dict(sr=0.0), "sampling rate nan": dict(sr=float("nan")), "sampling rate inf": dict(sr=INF),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    """The D19 entries' return codes, before any HIP call (the buffers are host memory)."""
    b = _Bufs()
    bad = INVALID[case]
    assert hiplib.dr_march_rgba_bundle_fwd(*_args(b, "fwd", **bad)) == -1
    assert hiplib.dr_march_rgba_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], **bad)) == -1
    assert hiplib.dr_march_rgba_bundle_bwd(*_args(b, "bwd", **bad)) == -1   # (checked before "nothing requested")
    assert hiplib.dr_march_rgba_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1


def test_nan_t_near_missing_outputs_and_nothing_requested(hiplib):
    b = _Bufs()
    assert hiplib.dr_march_rgba_bundle_bwd_rays(*_args(b, "rays", t_near=float("nan"))) == -1
    assert hiplib.dr_march_rgba_bundle_fwd(*_args(b, "fwd", out=None)) == -1
    assert hiplib.dr_march_rgba_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], go=None)) == -1
    assert hiplib.dr_march_rgba_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], out=None)) == -1
    assert hiplib.dr_march_rgba_bundle_bwd(*_args(b, "bwd")) == 0   # d_vol == NULL: nothing to do, no HIP call
    for bad in (dict(steps=None), dict(go=None), dict(out=None), dict(d_o=None), dict(d_d=None)):
        assert hiplib.dr_march_rgba_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1, bad


# --- 2. the float64 reference against central differences of itself -------------------------------------------------------------

FD_RAYS = (3, 40, 77, 150)
FD_STEP = 1e-6   # moves a sample by less than 3e-5 of a cell: none of these rays' samples lies that close to a face of its cell
#                  (one that did would put the jump of the trilinear slope into the difference, 1e-2 of the scale, not 1e-6)


def _objective(inp):
    res = RB.run(inp, grads=False)
    return float((res["rgba"][:, 0] * inp["grad_out"]).sum()), res


@pytest.mark.parametrize("volume,bundle", [("thin_sr1", "random_jitter"), ("opaque_sr2", "random")], ids=str)
def test_the_f64_reference_is_the_central_difference_of_its_own_forward(volume, bundle):
    """Four rays of a case (their origins and directions as free 3-vectors: dray's 24 numbers) and six voxel channels, each
    against (L(+h) - L(-h)) / 2h of the float64 forward with n, steps and the cells unchanged by the step."""
    full = RB.inputs(volume, bundle)
    idx = np.array(FD_RAYS)
    inp = dict(full, origins=full["origins"][idx], dirs=full["dirs"][idx], grad_out=full["grad_out"][idx])
    ref = RB.run(inp)   # (a jitter draw is per ray index: rays 0..3 of the sub-bundle draw their own, the same in every run)
    assert (ref["n"] > 1).all()
    scale = np.abs(ref["dray"]).max()
    for key, col in (("origins", 0), ("dirs", 3)):
        for p in range(len(idx)):
            for a in range(3):
                lo, hi = (dict(inp, **{key: inp[key].copy()}) for _ in range(2))
                lo[key][p, a] -= FD_STEP
                hi[key][p, a] += FD_STEP
                (Ll, rl), (Lh, rh) = _objective(lo), _objective(hi)
                assert (rl["n"] == ref["n"]).all() and (rh["n"] == ref["n"]).all()
                assert (rl["steps"] == ref["steps"]).all() and (rh["steps"] == ref["steps"]).all()
                fd = (Lh - Ll) / (2 * FD_STEP)
                assert abs(fd - ref["dray"][p, 0, col + a]) <= 1e-6 * scale, (key, p, a, fd, ref["dray"][p, 0, col + a])
    dv = ref["dvol"]
    top = np.argsort(np.abs(dv).reshape(-1))[::-1][:5]   # the five largest entries, and the largest of each colour's and alpha's
    for k in list(top) + [int(np.argmax(np.abs(dv[c]).reshape(-1))) + c * dv[0].size for c in (0, 3)]:
        at = np.unravel_index(int(k), dv.shape)
        lo, hi = (dict(inp, vol=inp["vol"].copy()) for _ in range(2))
        lo["vol"][at] -= FD_STEP
        hi["vol"][at] += FD_STEP
        fd = (_objective(hi)[0] - _objective(lo)[0]) / (2 * FD_STEP)
        assert abs(fd - dv[at]) <= 1e-6 * np.abs(dv).max(), (at, fd, dv[at])


# --- 3. conditioning, from the references alone -----------------------------------------------------------------------------------

@pytest.mark.parametrize("volume,bundle", RB.CASES, ids=lambda v: str(v))
def test_every_case_keeps_more_than_ninety_percent_of_its_rays(volume, bundle):
    """For every (volume, bundle) the GPU tests use: on bundle_reference.keep's rays the float32 and float64 references agree on n
    and steps, camgrad_gpu.well_conditioned (the columns origin and dir, no lighting) is applied on top, and what is left is
    more than 90 % of the n > 1 rays -- so the GPU tests' own cap of 80 % is met with room by the references alone. And the
    structure each case is there for."""
    inp, ref, ref32 = RB.state(volume, bundle)
    keep = RB.keep(ref, ref32)
    live = ref["n"] > 1
    assert (ref32["n"][keep] == ref["n"][keep]).all() and (ref32["steps"][keep] == ref["steps"][keep]).all()
    good = K.well_conditioned(ref, ref32, keep, "dray", RB.COLUMNS, (volume, bundle), lit=False)
    assert not (good & ~(keep & live)).any()
    assert good.sum() > 0.9 * live.sum(), (volume, bundle, good.sum(), live.sum())
    for _, sl in RB.COLUMNS:
        assert K.conditioned_err32(ref, ref32, keep, good, "dray", sl) <= K.FLOOR
    S = int(inp["max_samples"])
    d = inp["dirs"]
    if bundle == "ortho":
        assert (ref["n"] == 0).sum() == 4 and (ref["dray"][ref["n"][..., 0] == 0] == 0).all()
    if bundle == "interior_near0":
        assert (ref["entry"] == 0).all()   # every interior origin takes the clamp
    if bundle == "axial":
        assert ((d == 0).sum(1) == 2).all() and live.all()
    if bundle == "one_zero":
        assert ((d == 0).sum(1) == 1).all() and live.all()
    if volume == "thin_clip":
        assert live.all() and S < ref["n"].min() and (ref["steps"] == S).all()   # the clip lies below the shortest n
        unclipped = RB.run(dict(inp, max_samples=512))
        assert np.abs(unclipped["dray"] - ref["dray"]).max() > 1e-2 * np.abs(ref["dray"]).max()
    else:
        assert ref["n"].max() <= S
    if volume == "opaque_sr2":   # early termination: rays that stop before their last sample, frozen by steps in the ray gradient
        assert (ref["steps"][live] < ref["n"][live]).sum() > 0.2 * live.sum()
    if volume == "thin_sr1":
        assert (ref["steps"][live] == ref["n"][live]).all()
    if bundle == "random_jitter":
        plain = RB.state(volume, "random")[1]
        assert np.abs(plain["dray"] - ref["dray"]).max() > 1e-2 * np.abs(ref["dray"]).max()
    if bundle == "single_sample":
        one = BR.SINGLE
        assert (ref["n"][one] == 1).all() and (ref32["n"][one] == 1).all() and (ref["n"][~one] > 1).all()
        assert (ref["dray"][one] == 0).all() and (ref["rgba"][one] == 0).all()   # H6: the reference marches no such ray


# --- 4. the module's argument checks ------------------------------------------------------------------------------------------------

def test_module_argument_checks(hiplib):
    from differender_amd.rgba import RayBundleRaycasterRGBA
    with pytest.raises(ValueError):
        RayBundleRaycasterRGBA((8, 8))
    with pytest.raises(ValueError):
        RayBundleRaycasterRGBA((8, 8, 8), max_samples=0)
    with pytest.raises(ValueError):
        RayBundleRaycasterRGBA((8, 8, 8), t_near=float("nan"))
    rc = RayBundleRaycasterRGBA((8, 9, 10))
    vol, o, d = torch.rand(4, 8, 9, 10), torch.zeros(5, 7, 3), torch.ones(5, 7, 3)
    for bad in ((vol[0], o, d), (vol[:3], o, d), (torch.rand(4, 8, 9, 11), o, d), (vol[None], o, d), (vol, o[0], d),
                (vol, o[..., :2], d[..., :2]), (vol, o[:0], d[:0])):
        with pytest.raises(ValueError):
            rc(*bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # shapes fine, tensors on the CPU: there is no CPU path
        rc(vol, o, d)
    assert "ray_grad = False" in repr(rc)


def test_ray_tensors_that_require_grad_need_ray_grad(hiplib):
    from differender_amd.rgba import RayBundleRaycasterRGBA
    rc = RayBundleRaycasterRGBA((8, 8, 8))
    vol = torch.rand(4, 8, 8, 8)
    for name in ("origins", "directions"):
        rays = dict(origins=torch.zeros(6, 3), directions=torch.ones(6, 3))
        rays[name].requires_grad_(True)
        with pytest.raises(ValueError, match=f"no gradient w.r.t. {name}.*ray_grad=True"):
            rc(vol, **rays)
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):   # (nothing to refuse without autograd)
            rc(vol, **rays)


def test_a_zero_length_direction_raises(hiplib):
    from differender_amd.rgba import RayBundleRaycasterRGBA
    rc = RayBundleRaycasterRGBA((8, 8, 8), ray_grad=True)
    d = torch.ones(6, 3)
    d[4] = 0.0
    with pytest.raises(ValueError, match="zero length"):
        rc(torch.rand(4, 8, 8, 8), torch.zeros(6, 3), d)
