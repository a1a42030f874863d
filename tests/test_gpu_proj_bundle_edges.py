"""The backwards of the bundle projections past one ray group, against float64: the windowed SUM backward on
the paths its first tests only held to the plain kernel -- LDS windows at the first and at halved depths, the fall-through
after samples were taken (a cone beam that spreads), max_samples inside the window walk, lanes at staggered depths, ragged and
dead groups, the three volume layouts -- and the MIP's under the clip; the SUM adjoint identity under the clip; the ray
gradients under max_samples, of axis-parallel rays and of an f16 volume; a cone beam's source gradient through the module.
Every windowed case asserts the paths it is there for on the kernel's own buffers (proj_bundle_reference.group_trace) before
it compares anything. One tolerance: D8's rule with the float32 transliteration's own error (proj_bundle_reference.d8_check),
and the windowed-against-plain bound of tests/test_gpu_proj_bundle.py beside it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import proj_bundle_reference as PB  # noqa: E402
import proj_reference as PR  # noqa: E402
from bundle_reference import BUNDLES  # noqa: E402
from test_gpu_proj_bundle import AUTO, BASELINE, MODES, C, _F, _forward, _opts, bits, dev  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- 1. d_vol of the windowed, the plain and the MIP backward on the declared paths ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    """The rays and the upstream gradient of an edge case (made once and shared; nobody writes to them)."""
    return PB.edge_case(name)


def _volume(case, seed=6):
    """Random values in [0, 1) in the case's layout on the device, with the strides the case says -> values (numpy), volume."""
    vals = torch.rand(case["vshape"], generator=torch.Generator().manual_seed(seed))
    vol = PR.layout_volume(vals.cuda(), case["layout"])
    assert PB.LAYOUT_STRIDES[case["layout"]](tuple(vol.stride()), case["vshape"]), (case["layout"], vol.stride())
    return vals.double().numpy(), vol


def _setup(case):
    F = _F()
    o, d = dev(case["origins"]), dev(case["dirs"])
    e, x, n = F.bundle_setup(o, d, case["vshape"], case["sr"], case["t_near"], case["seed"], PB.RAY_BASE)
    return o, d, e, x, n, [C(e), C(x), n.cpu().numpy()]


SUM_RUNS = [(name, S) for name in sorted(PB.EDGE_CASES) for S in PB.EDGE_CASES[name]["clips"]]


@pytest.mark.parametrize("name,S", SUM_RUNS, ids=["%s-%s" % r for r in SUM_RUNS])
def test_sum_d_vol_on_every_declared_path_matches_f64(hiplib, name, S):
    F = _F()
    case = _case(name)
    vals, vol = _volume(case)
    o, d, e, x, n, own = _setup(case)
    PB.check_paths(case, S, PB.group_trace(case["origins"], own[0], own[1], case["dirs"], own[2], case["vshape"], S, case["live"]))
    g = dev(case["grad_out"])
    g_ref = np.where(np.isfinite(case["grad_out"]), case["grad_out"], 0.0)   # a NaN lane adds nothing (D5)
    ref = [PB.on_buffers(vals, case["origins"], case["dirs"], *own, g_ref, S, "sum", dt)[1] for dt in (torch.float64, torch.float32)]
    assert (ref[0] != 0).any()
    got = {}
    for variant in (AUTO, BASELINE):
        got[variant] = F.project_bundle_bwd(vol, o, d, e, x, n, g, S, "sum", None, variant=variant)
        assert got[variant].stride() == vol.stride() and got[variant].dtype == torch.float32
        PB.d8_check(C(got[variant]), *ref, (name, S, "d_vol", "AUTO" if variant == AUTO else "BASELINE"))
    scale = float(got[BASELINE].abs().max())
    assert scale > 0 and float((got[AUTO] - got[BASELINE]).abs().max()) <= 1e-5 * scale, (name, S)


@pytest.mark.parametrize("name,S", PB.MAX_CASES, ids=["%s-%s" % r for r in PB.MAX_CASES])
def test_max_d_vol_under_the_clip_matches_f64_at_the_kernels_argmax(hiplib, name, S):
    F = _F()
    case = _case(name)
    vals, vol = _volume(case)
    o, d, e, x, n, own = _setup(case)
    out, arg = F.project_bundle_fwd(vol, o, d, e, x, n, S, "max")
    a, nn = arg.cpu().numpy(), own[2]
    live = nn > 1
    assert live.sum() > 0.9 * live.size and (nn > S).any()
    assert (a[live] >= 0).all() and (a[live] < np.minimum(nn, S)[live]).all() and (a[~live] == -1).all()
    g = dev(case["grad_out"])
    g_ref = np.where(np.isfinite(case["grad_out"]), case["grad_out"], 0.0)
    ref = [PB.on_buffers(vals, case["origins"], case["dirs"], *own, g_ref, S, "max", dt, a)[1] for dt in (torch.float64, torch.float32)]
    assert (ref[0] != 0).any()
    d_vol = F.project_bundle_bwd(vol, o, d, e, x, n, g, S, "max", arg)
    PB.d8_check(C(d_vol), *ref, (name, S, "max d_vol"))


# ---- 2. the SUM adjoint identity under the clip: the clipped backward tied to the clipped forward -----------------------------------

@pytest.mark.parametrize("variant", [AUTO, BASELINE])
@pytest.mark.parametrize("S", [None, 150])
def test_sum_adjoint_identity_on_the_spreading_cone(hiplib, S, variant):
    F = _F()
    case = _case("cone_spreading")
    _, vol = _volume(case, seed=2)
    o, d, e, x, n, own = _setup(case)
    PB.check_paths(case, S, PB.group_trace(case["origins"], own[0], own[1], case["dirs"], own[2], case["vshape"], S))
    out, _ = F.project_bundle_fwd(vol, o, d, e, x, n, S, "sum")
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    dv = F.project_bundle_bwd(vol, o, d, e, x, n, g, S, "sum", None, variant=variant)
    lhs = float((out.double() * g.double()).sum())
    rhs = float((vol.double() * dv.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((out.double().abs() * g.double().abs()).sum()), (S, lhs, rhs)


# ---- 3. the ray gradients under max_samples ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clip_state(bundle, shape, mode, S):
    inp = PB.inputs(bundle, *PB.SHAPES[shape], max_samples=S)
    return inp, PB.run(inp, mode), PB.run(inp, mode, torch.float32)


def _check_ray_gradients(inp, ref, ref32, mode, what, vol=None):
    """The kernel's d_origin and d_dir of inp against the two references by D8's rule on the rays all three agree on -> the raw
    results, n and the forward's arg_max."""
    F = _F()
    vol, o, d, e, x, n, out, arg = _forward(inp, mode, vol)
    d_o, d_d = F.project_bundle_bwd_rays(vol, o, d, e, x, n, dev(inp["grad_out"]), inp.get("max_samples"), mode, arg, **_opts(inp))
    assert bool(torch.isfinite(d_o).all()) and bool(torch.isfinite(d_d).all()), what   # (the raw result, before any comparison)
    nk = n.cpu().numpy()
    same, live = PB.agree(ref, ref32, mode, nk, None if arg is None else arg.cpu().numpy())
    keep = same & live
    assert keep.sum() >= 0.9 * live.sum(), (what, keep.sum(), live.sum())
    assert (C(d_o)[nk <= 1] == 0).all() and (C(d_d)[nk <= 1] == 0).all()
    PB.d8_check(C(d_o)[keep], ref["d_origin"][keep], ref32["d_origin"][keep], (*what, mode, "d_origin"))
    PB.d8_check(C(d_d)[keep], ref["d_dir"][keep], ref32["d_dir"][keep], (*what, mode, "d_dir"))
    return d_o, d_d, n, arg


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(PB.SHAPES))
@pytest.mark.parametrize("bundle", sorted(BUNDLES))
def test_ray_gradients_under_max_samples_match_autograd_of_the_reference(hiplib, bundle, shape, mode):
    unclipped = _clip_state(bundle, shape, mode, None)
    free = _check_ray_gradients(*unclipped, mode, (bundle, shape, None))
    for S in PB.CLIPS:
        S = PB.clip(S, free[2].cpu().numpy(), unclipped[1]["n"])
        inp, ref, ref32 = _clip_state(bundle, shape, mode, S)
        got = _check_ray_gradients(inp, ref, ref32, mode, (bundle, shape, S))
        if S > 5:   # a max_samples no ray reaches reproduces the unclipped result, bit for bit
            assert bool((got[2] <= S).all())
            assert torch.equal(bits(got[0]), bits(free[0])) and torch.equal(bits(got[1]), bits(free[1]))
        else:
            assert int((got[2] > S).sum()) >= 0.9 * int((got[2] > 1).sum())   # the clip clips
            assert not torch.equal(got[0], free[0])


# ---- 4. axis-parallel rays: a direction component that is exactly 0 ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _axis_state(axis, sign, S, mode):
    inp = PB.axis_inputs(axis, sign, S)
    return inp, PB.run(inp, mode), PB.run(inp, mode, torch.float32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("axis,sign", PB.AXES, ids=["%s%s" % ("+" if s > 0 else "-", "xyz"[a]) for a, s in PB.AXES])
def test_axis_parallel_ray_gradients_are_finite_nonzero_and_match(hiplib, axis, sign, mode):
    for S in PB.AXIS_CLIPS:
        inp, ref, ref32 = _axis_state(axis, sign, S, mode)
        d_o, d_d, n, _ = _check_ray_gradients(inp, ref, ref32, mode, ("axis", axis, sign, S))
        assert bool((n > 9).all())   # every ray is live, and the clip clips it
        # no ray's six floats are all zero: finite_or_zero did not swallow a NaN of the 1 / 0 in the slab test
        assert bool((torch.cat([d_o, d_d], 1) != 0).any(1).all()), (axis, sign, S)


# ---- 5. a cone beam's source gradient, end to end through the module ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_cone_beam_source_gradient_through_the_module(hiplib, mode):
    """RayBundleProjector(ray_grad=True, jitter on) on cone_beam_rays of the spreading cone at 24^3 under a 16 x 16 detector:
    source.grad of sum(out g) against autograd through cone_beam_rays and the reference program in float64 on the CPU, by D8's
    rule; g is zero off the rays whose n (and argmax) float64, float32 and the kernel agree on."""
    from differender_amd.projection import RayBundleProjector
    F = _F()
    cone, V = PB.CONE_SMALL, 24
    vals = torch.rand((V, V, V), generator=torch.Generator().manual_seed(9))
    user = vals.permute(1, 2, 0).contiguous()[None].cuda()   # (1, D, H, W), whose field (W, D, H) is vals
    field = user[0].permute(2, 0, 1)
    assert np.array_equal(C(field), vals.double().numpy())
    seed = PB.module_jitter_seed()
    source = dev(cone["source"]).requires_grad_(True)
    pj = RayBundleProjector((V, V, V), mode=mode, jitter=True, ray_grad=True)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(PB.SOURCE_TORCH_SEED)
        out = pj(user, *PB.cone_rays(cone, source, normalise=False))
    # the buffers the module's kernels saw: its own statements on the same rays, the seed it drew
    ok, dk = (t.detach() for t in PB.cone_rays(cone, source))
    e, x, n = F.bundle_setup(ok, dk, field.shape, 1.0, None, seed)
    out_k, arg_k = F.project_bundle_fwd(field, ok, dk, e, x, n, None, mode)
    assert torch.equal(bits(out.detach()), bits(out_k))
    inp = dict(vol=vals.double().numpy(), sr=1.0, max_samples=None, jitter_seed=seed, ray_base=0)
    refs = [PB.source_gradient(cone, inp, mode, dt) for dt in (torch.float64, torch.float32)]
    same, live = PB.agree(*refs, mode, n.cpu().numpy(), None if arg_k is None else arg_k.cpu().numpy())
    keep = same & live
    assert live.sum() > 200 and keep.sum() >= 0.9 * live.sum(), (keep.sum(), live.sum())
    g = np.random.RandomState(5).standard_normal(keep.size) * keep
    want = [PB.source_gradient(cone, inp, mode, dt, PB.F32(g))["d_source"] for dt in (torch.float64, torch.float32)]
    (out * dev(g)).sum().backward()
    assert np.abs(want[0]).max() > 0
    PB.d8_check(C(source.grad), *want, (mode, "cone source"))


# ---- 6. an f16 volume -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _f16_state(mode):
    inp = PB.inputs("random", *PB.SHAPES["sr1"], dtype=torch.float16)
    return inp, PB.run(inp, mode), PB.run(inp, mode, torch.float32)


@pytest.mark.parametrize("mode", MODES)
def test_f16_volume_max_d_vol_and_ray_gradients(hiplib, mode):
    """The references on the volume rounded to f16. d_vol of an f16 volume is float32 in the volume's layout (functional._d_vol)."""
    F = _F()
    inp, ref, ref32 = _f16_state(mode)
    vol = PR.layout_volume(dev(inp["vol"]).half(), "x")
    assert vol.dtype == torch.float16 and vol.stride(0) == 1 and np.array_equal(C(vol), inp["vol"])
    _check_ray_gradients(inp, ref, ref32, mode, ("f16",), vol=vol)
    if mode == "max":
        vol, o, d, e, x, n, out, arg = _forward(inp, mode, vol)
        own = [C(e), C(x), n.cpu().numpy(), inp["grad_out"], None, mode]
        dv = [PB.on_buffers(inp["vol"], inp["origins"], inp["dirs"], *own, dt, arg.cpu().numpy())[1] for dt in (torch.float64, torch.float32)]
        d_vol = F.project_bundle_bwd(vol, o, d, e, x, n, dev(inp["grad_out"]), None, mode, arg)
        assert d_vol.dtype == torch.float32 and d_vol.stride() == vol.stride() and d_vol.shape == vol.shape
        PB.d8_check(C(d_vol), *dv, ("f16", "max d_vol"))
