"""Projections of ray bundles, DESIGN.md D20, without a GPU: the C ABI and its argument checks, cone_beam_rays and tile_order,
the reference (tests/proj_bundle_reference.py) pinned to proj_reference.project_camera on a pinhole's rays, what the float64
comparisons of the GPU file owe their own rule (rays kept, a mutated tail coefficient refused), the windowed cases held to the
plan model, the cases of tests/test_gpu_proj_bundle_edges.py held to their declared paths and to the conditions their
comparisons rest on, and the module's argument checks."""
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

import bundle_reference as BR  # noqa: E402
import proj_bundle_reference as PB  # noqa: E402
import proj_reference as PR  # noqa: E402
from test_bundle import CAM, POSE  # noqa: E402
from test_rgba import _Bufs, _header_params  # noqa: E402

ENTRIES = ("dr_project_bundle_fwd", "dr_project_bundle_bwd", "dr_project_bundle_bwd_rays")
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
                    ctypes.c_float if p.startswith("float") else ctypes.c_double if p.startswith("double") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (name, p, a)
    # the three entries share their head, up to the mode: dr_march_bundle_fwd's without the table and the sampling rate
    fwd, bwd, rays = (_header_params(n) for n in ENTRIES)
    head = fwd[:fwd.index("int mode") + 1]
    assert bwd[:len(head)] == head and rays[:len(head)] == head
    march = [p for p in _header_params("dr_march_bundle_fwd") if p not in ("const float *tf", "int R", "float sampling_rate")]
    assert head[:-1] == march[:len(head) - 1]
    assert all(ps[-1] == "void *stream" for ps in (fwd, bwd, rays))
    from differender_amd import functional as F
    assert all(n in F.__all__ for n in ("project_bundle_fwd", "project_bundle_bwd", "project_bundle_bwd_rays"))


def _args(b, which, **kw):
    a = dict(vol=b.p[0], dtype=0, VX=8, VY=8, VZ=8, sx=64, sy=8, sz=1, origins=b.p[2], dirs=b.p[5], entry=b.p[3], exit=b.p[4],
             n=b.p[6], N=16, S=64, mode=0)
    if which == "fwd":
        a.update(out=b.p[7], arg=b.p[1])
    elif which == "bwd":
        a.update(go=b.p[7], arg=b.p[1], dvol=None, dsx=0, dsy=0, dsz=0, variant=0)
    else:
        a.update(t_near=-INF, seed=0, base=0, go=b.p[7], arg=b.p[1], d_o=b.p[0], d_d=b.p[1])
    a.update(stream=None)
    a.update(kw)
    return list(a.values())


INVALID = {
    "null volume": dict(vol=None), "null origins": dict(origins=None), "null dirs": dict(dirs=None),
    "null entry": dict(entry=None), "null exit": dict(exit=None), "null n": dict(n=None), "unknown dtype": dict(dtype=7),
    "N 0": dict(N=0), "N -5": dict(N=-5), "N 2^31": dict(N=2 ** 31), "N 2^40": dict(N=2 ** 40), "VX 1": dict(VX=1),
    "VY -3": dict(VY=-3), "VZ 0": dict(VZ=0), "max_samples 0": dict(S=0), "max_samples < 0": dict(S=-1),
    "mode 2": dict(mode=2), "mode -1": dict(mode=-1), "max without arg_max": dict(mode=1, arg=None),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_return_einval_without_a_gpu(hiplib, case):
    b = _Bufs()
    bad = INVALID[case]
    assert hiplib.dr_project_bundle_fwd(*_args(b, "fwd", **bad)) == -1
    assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], **bad)) == -1
    assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", **bad)) == -1   # (checked before "nothing requested")
    assert hiplib.dr_project_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1


def test_nan_t_near_variant_missing_outputs_and_nothing_requested(hiplib):
    b = _Bufs()
    assert hiplib.dr_project_bundle_bwd_rays(*_args(b, "rays", t_near=float("nan"))) == -1
    assert hiplib.dr_project_bundle_fwd(*_args(b, "fwd", out=None)) == -1
    assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], go=None)) == -1
    for variant in (-1, 2, 7):
        assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", dvol=b.p[0], variant=variant)) == -1
        assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", variant=variant)) == -1
    for mode in (0, 1):
        for variant in (0, 1):
            assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", mode=mode, variant=variant)) == 0   # d_vol NULL: no HIP call
    for bad in (dict(go=None), dict(d_o=None), dict(d_d=None)):
        assert hiplib.dr_project_bundle_bwd_rays(*_args(b, "rays", **bad)) == -1, bad
    # arg_max is not read for DR_PROJ_SUM: NULL is fine up to the first HIP call (d_vol NULL stops short of it)
    assert hiplib.dr_project_bundle_bwd(*_args(b, "bwd", arg=None)) == 0


# --- 2. the helpers -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("WH", [(16, 16), (14, 9)], ids=str)
def test_cone_beam_rays_with_the_near_plane_as_detector_are_pinhole_rays(WH):
    """det_center = look_from + near view_dir, det_u = (near_w / W) right, det_v = -(near_h / H) up'."""
    from differender_amd.bundle import _camera_basis, cone_beam_rays, pinhole_rays
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    lf, la, up = T(CAM), T(POSE["look_at"]), T(POSE["up"])
    fov_deg, near, (W, H) = 27.0, 0.1, WH
    want_o, want_d = pinhole_rays(lf, la, up, fov_deg, WH, near)
    vd, right, upp = _camera_basis(lf, la, up)
    near_h = 2.0 * math.tan(math.radians(fov_deg)) * near
    near_w = near_h * (W / H)
    o, d = cone_beam_rays(lf, lf + near * vd, (near_w / W) * right, -(near_h / H) * upp, (H, W))
    assert o.shape == d.shape == (H, W, 3) and o.dtype == torch.float64
    assert float((d - want_d).abs().max()) <= 1e-12 and bool((o == want_o).all())


def test_cone_beam_rays_detector_offset_pitch_and_gradients():
    from differender_amd.bundle import cone_beam_rays
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    src = T([0.0, 0.0, 3.0]).requires_grad_(True)
    centre, u, v = T([0.25, -0.1, -2.0]), T([0.05, 0.0, 0.0]), T([0.0, -0.03, 0.0])
    o, d = cone_beam_rays(src, centre, u, v, (5, 8))
    assert o.shape == d.shape == (5, 8, 3)
    assert float((d.detach().norm(dim=-1) - 1.0).abs().max()) <= 1e-15
    # pixel (r, c) lies on its ray, at centre + (c - 3.5) u + (r - 2) v
    for r, c in ((0, 0), (4, 7), (2, 3)):
        pix = centre + (c - 3.5) * u + (r - 2.0) * v
        t = (pix - src).norm()
        assert float((src + t * d[r, c] - pix).detach().abs().max()) <= 1e-14
    (d[..., 0].sum()).backward()
    assert src.grad is not None and float(src.grad.abs().max()) > 0


@pytest.mark.parametrize("HW", [(32, 48), (16, 16), (64, 32)], ids=str)
def test_tile_order_is_a_permutation_in_runs_of_tiles_and_blocks(HW):
    from differender_amd.bundle import tile_order
    H, W = HW
    perm = tile_order(HW)
    assert perm.dtype == torch.int64 and sorted(perm.tolist()) == list(range(H * W))
    r, c = perm // W, perm % W
    for run, side in ((256, 16), (64, 8)):
        rr, cc = r.reshape(-1, run), c.reshape(-1, run)
        assert bool(((rr.max(1).values - rr.min(1).values) == side - 1).all())
        assert bool(((cc.max(1).values - cc.min(1).values) == side - 1).all())
        assert bool((rr.min(1).values % side == 0).all()) and bool((cc.min(1).values % side == 0).all())


def test_tile_order_on_ragged_grids_is_still_a_permutation():
    from differender_amd.bundle import tile_order
    for HW in ((1, 1), (5, 7), (17, 33), (30, 16)):
        assert sorted(tile_order(HW).tolist()) == list(range(HW[0] * HW[1]))
    with pytest.raises(ValueError):
        tile_order((4, 4), tile=5)
    with pytest.raises(ValueError):
        tile_order((0, 4))


# --- 3. the reference pinned to the projections' own ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("seed", [0, 4242], ids=["no_jitter", "jitter"])
def test_the_reference_on_a_pinholes_rays_is_project_camera(mode, seed):
    """out, arg, n and d_vol of the two programs are equal (the ray gradients are autograd's of the same program)."""
    vshape, (W, H), sr, view = (14, 12, 16), (10, 8), 1.0, 3
    vol = torch.rand(vshape, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    cam = torch.tensor(PR.orbit(0.5, 0.3, 2.7), dtype=torch.float64)
    g = torch.from_numpy(np.random.RandomState(1).standard_normal(W * H))
    v = vol.clone().requires_grad_(True)
    want, want_arg, (e, x, r, n) = PR.project_camera(v, cam, W, H, sr, None, mode, jitter_seed=seed, view=view)
    (want * g).sum().backward()
    inp = dict(vol=vol.numpy(), origins=cam.expand(W * H, 3).numpy(), dirs=r.detach().numpy(), grad_out=g.numpy(), sr=sr,
               max_samples=None, jitter_seed=seed, ray_base=view)
    got = PB.run(inp, mode)
    assert (got["n"] == n.numpy()).all() and (got["n"] > 1).sum() > W * H // 2
    assert np.abs(got["out"] - want.detach().numpy()).max() <= 1e-12
    if mode == "max":
        assert (got["arg"] == want_arg.numpy()).all()
    assert np.abs(got["dvol"] - v.grad.numpy()).max() <= 1e-12 * np.abs(got["dvol"]).max()


# --- 4. what the float64 comparisons of the GPU file owe their rule ----------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("shape", sorted(PB.SHAPES))
@pytest.mark.parametrize("bundle", sorted(BR.BUNDLES))
def test_every_gradient_case_keeps_its_rays(bundle, shape, mode):
    """float32 and float64 agree on n (and the argmax) of at least 90 % of the live rays of every case."""
    inp = PB.inputs(bundle, *PB.SHAPES[shape])
    ref, ref32 = PB.run(inp, mode), PB.run(inp, mode, torch.float32)
    same, live = PB.agree(ref, ref32, mode)
    assert live.sum() >= 100 and (same & live).sum() >= 0.9 * live.sum()
    for key in ("d_origin", "d_dir"):
        assert np.abs(ref[key][live]).max() > 0 and (ref[key][~live] == 0).all()
    if "near0" in bundle:
        assert (ref["entry"] == 0).all()   # every interior origin takes the clamp


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_the_rule_rejects_a_one_percent_error_in_a_tail_coefficient(mode):
    """The float32 transliteration passes D8's rule; the float64 reference with 1 % more gradient through tmax (the tail's
    k_max) does not, for either ray gradient."""
    inp = PB.inputs("random", *PB.SHAPES["sr1"])
    ref, ref32 = PB.run(inp, mode), PB.run(inp, mode, torch.float32)
    bad = PB.run(inp, mode, kmax_factor=1.01)
    same, live = PB.agree(ref, ref32, mode)
    keep = same & live
    for key in ("d_origin", "d_dir"):
        PB.d8_check(ref32[key][keep], ref[key][keep], ref32[key][keep], key)
        with pytest.raises(AssertionError):
            PB.d8_check(bad[key][keep], ref[key][keep], ref32[key][keep], key)
    assert np.array_equal(bad["dvol"], ref["dvol"])   # (the volume's gradient does not pass through tmax)


# --- 5. the windowed cases hit the paths they are there for ------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PB.WINDOW_CASES))
def test_window_cases_take_their_paths(name):
    o, d, case = PB.window_case(name)
    e, x, n = PB.slab32(o, d, case["vshape"], case["sr"], None, case["seed"], PB.RAY_BASE)
    plan = PB.group_plan(o, e, x, d, n, case["vshape"])
    for path in case["paths"]:
        assert getattr(plan, path) > 0, (name, plan)
    assert plan.live_groups + plan.dead_groups == -(-o.shape[0] // 256)


def test_window_cases_cover_every_path_and_the_ragged_group():
    K = PB.window_constants()
    assert K["PBW_GROUP"] == 256 and K["PBW_BOX"] * 4 <= 64 * 1024
    paths = {p for c in PB.WINDOW_CASES.values() for p in c["paths"]}
    assert paths == {"lds_full", "lds_halved", "fall_through", "dead_groups"}
    assert PB.window_case("random_300_fall_through")[0].shape[0] % 256 != 0
    o, d, case = PB.window_case("missing_group")
    assert (PB.slab32(o, d, case["vshape"], 1.0)[2][:256] == 0).all()
    # the projections' own constants stay where proj_reference reads them
    assert PR.window_constants() == {"PW_TILE": 16.0, "PW_BOX": 7680.0, "PW_WIN_VOX": 16.0, "PW_MIN_VOX": 2.0}


# --- 5b. the cases of tests/test_gpu_proj_bundle_edges.py, from the float32 slab and the plan alone ------------------------------------

def _edge_trace(case, S):
    e, x, n = PB.slab32(case["origins"], case["dirs"], case["vshape"], case["sr"], case["t_near"], case["seed"], PB.RAY_BASE)
    return PB.group_trace(case["origins"], e, x, case["dirs"], n, case["vshape"], S, case["live"]), n


@pytest.mark.parametrize("name", sorted(PB.EDGE_CASES))
def test_edge_cases_take_their_declared_paths(name):
    case = PB.edge_case(name)
    vol = PR.layout_volume(torch.zeros(case["vshape"]), case["layout"])
    assert PB.LAYOUT_STRIDES[case["layout"]](tuple(vol.stride()), case["vshape"]) and sorted(vol.stride())[0] == 1
    assert ("xyz"[int(np.argmin(vol.stride()))] == case["layout"]) and tuple(vol.shape) == tuple(case["vshape"])
    for S in case["clips"]:
        trace, n = _edge_trace(case, S)
        PB.check_paths(case, S, trace)
        assert len(trace) == -(-n.shape[0] // 256)
        # group_plan is the trace summed: its fields keep their meaning
        plan = PB.group_plan(case["origins"], *PB.slab32(case["origins"], case["dirs"], case["vshape"], case["sr"], case["t_near"],
                                                         case["seed"], PB.RAY_BASE)[:2], case["dirs"], n, case["vshape"], S, case["live"])
        walked = [t for t in trace if t is not None]
        assert plan == PB.GroupPlan(sum(t.lds_full for t in walked), sum(t.lds_halved for t in walked),
                                    sum(t.fell for t in walked), len(trace) - len(walked), len(walked))
        if S is not None:
            assert (n > S).any()   # the clip clips


def test_the_spreading_cone_falls_through_with_samples_taken_and_the_clips_end_it_earlier():
    case = PB.edge_case("cone_spreading")
    counts = {}
    for S in case["clips"]:
        trace, n = _edge_trace(case, S)
        counts[S] = (sum(t.lds_full for t in trace), sum(t.lds_halved for t in trace), sum(t.fell for t in trace))
        if S is None:   # every group leaves through the per-tap loop from s_cur > 0, most of its samples still to come
            total = [int(n[g0:g0 + 256].sum()) for g0 in range(0, 1024, 256)]
            assert all(t.fell and 0 < t.s_cur_at_fall < tot for t, tot in zip(trace, total)), trace
    assert counts == {None: (4, 28, 4), 150: (4, 24, 0), 100: (8, 0, 0), 1: (4, 0, 0)}, counts


def test_the_staggered_group_and_the_group_edges_are_what_they_say():
    case = PB.edge_case("staggered_depths")
    (trace,), n = _edge_trace(case, None)
    assert trace.staggered and n.shape == (256,)
    inside, missing = np.arange(256) % 8 == 3, np.arange(256) % 16 == 5
    assert (n[missing] == 0).all() and (n[~missing] > 1).all()
    assert n[inside].max() < PB.STAGGERED_CLIP < n[~inside & ~missing].min()   # the clip clips the longer rays alone
    g = case["grad_out"]
    assert np.isnan(g[PB.NAN_LANE]) and n[PB.NAN_LANE] > 1 and (g[np.arange(256) % 16 == 9] == 0).all()
    assert not case["live"][PB.NAN_LANE] and case["live"].sum() == 256 - 16 - 1
    # the flag does not hang on the rays from inside the box alone
    e, x, _ = PB.slab32(case["origins"], case["dirs"], case["vshape"], case["sr"], case["t_near"], case["seed"], PB.RAY_BASE)
    for S in case["clips"]:
        assert PB.group_trace(case["origins"], e, x, case["dirs"], n, case["vshape"], S, case["live"] & ~inside)[0].staggered
    for r in (1, 64, 65):
        case = PB.edge_case("group_edges_%d" % r)
        trace, n = _edge_trace(case, None)
        assert n.shape[0] == 512 + r and len(trace) == 3
        assert trace[0] is not None and trace[1] is None and trace[2] is not None   # the middle group returns early
        assert (n[256:512] > 1).all() and (case["grad_out"][256:512] == 0).all()
        assert (n[512:-1] == 0).all() and n[-1] > 1 and case["live"][-1]          # the last lane alone is live


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("shape", sorted(PB.SHAPES))
@pytest.mark.parametrize("bundle", sorted(BR.BUNDLES))
def test_every_clipped_gradient_case_keeps_its_rays(bundle, shape, mode):
    n_free = PB.run(PB.inputs(bundle, *PB.SHAPES[shape]), mode, grads=False)["n"]
    for S in PB.CLIPS:
        inp = PB.inputs(bundle, *PB.SHAPES[shape], max_samples=PB.clip(S, n_free))
        ref, ref32 = PB.run(inp, mode), PB.run(inp, mode, torch.float32)
        same, live = PB.agree(ref, ref32, mode)
        assert live.sum() >= 100 and (same & live).sum() >= 0.9 * live.sum(), (S, same.sum(), live.sum())
        assert np.isfinite(ref["d_origin"]).all() and np.abs(ref["d_origin"][live]).max() > 0


@pytest.mark.parametrize("mode", ["sum", "max"])
@pytest.mark.parametrize("axis,sign", PB.AXES)
def test_axis_parallel_reference_gradients_are_finite_and_keep_their_rays(axis, sign, mode):
    for S in PB.AXIS_CLIPS:
        inp = PB.axis_inputs(axis, sign, S)
        assert (inp["dirs"][:, axis] == sign).all() and (np.delete(inp["dirs"], axis, 1) == 0).all()
        assert (np.abs(np.delete(inp["origins"], axis, 1)) < 0.9).all() and (inp["origins"][:, axis] == -2.5 * sign).all()
        ref, ref32 = PB.run(inp, mode), PB.run(inp, mode, torch.float32)
        same, live = PB.agree(ref, ref32, mode)
        assert live.all() and (ref["n"] > 9).all() and (same & live).sum() >= 0.9 * live.sum()
        for r in (ref, ref32):
            six = np.concatenate([r["d_origin"], r["d_dir"]], 1)
            assert np.isfinite(six).all() and (six != 0).any(1).all()


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_the_f16_volume_case_keeps_its_rays(mode):
    inp = PB.inputs("random", *PB.SHAPES["sr1"], dtype=torch.float16)
    assert np.array_equal(inp["vol"], inp["vol"].astype(np.float16).astype(np.float64))
    same, live = PB.agree(PB.run(inp, mode, grads=False), PB.run(inp, mode, torch.float32, grads=False), mode)
    assert live.sum() >= 100 and (same & live).sum() >= 0.9 * live.sum()


@pytest.mark.parametrize("mode", ["sum", "max"])
def test_the_cone_source_case_keeps_its_rays(mode):
    cone, seed = PB.CONE_SMALL, PB.module_jitter_seed()
    assert seed == PB.module_jitter_seed() != 0
    vol = torch.rand((24, 24, 24), generator=torch.Generator().manual_seed(9)).double().numpy()
    inp = dict(vol=vol, sr=1.0, max_samples=None, jitter_seed=seed, ray_base=0)
    ref, ref32 = (PB.source_gradient(cone, inp, mode, dt) for dt in (torch.float64, torch.float32))
    same, live = PB.agree(ref, ref32, mode)
    assert live.sum() > 200 and (same & live).sum() >= 0.9 * live.sum(), (same.sum(), live.sum())
    g = PB.F32(np.random.RandomState(5).standard_normal(live.size) * (same & live))
    want = PB.source_gradient(cone, inp, mode, torch.float64, g)["d_source"]
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    # the small cone is the spreading cone's: the same source, detector plane and extent
    assert all(PB.CONE[k] == cone[k] for k in ("source", "det_center"))
    assert cone["det"][0] * cone["det_u"][0] == PB.CONE["det"][0] * PB.CONE["det_u"][0]


# --- 6. the module's argument checks ------------------------------------------------------------------------------------------------

def test_module_argument_checks(hiplib):
    from differender_amd.projection import RayBundleProjector
    for bad in (dict(volume_shape=(8, 8)), dict(volume_shape=(8, 1, 8)), dict(mode="mean"), dict(sampling_rate=0.0),
                dict(max_samples=0), dict(t_near=float("nan"))):
        with pytest.raises(ValueError):
            RayBundleProjector(**{"volume_shape": (8, 8, 8), **bad})
    pj = RayBundleProjector((8, 9, 10))
    assert pj.max_samples is None and pj.mode == "sum" and pj.t_near is None
    vol, o, d = torch.rand(1, 8, 9, 10), torch.zeros(5, 7, 3), torch.ones(5, 7, 3)
    for bad in ((vol[0], o, d), (torch.rand(1, 8, 9, 11), o, d), (vol, o[0], d), (vol, o[..., :2], d[..., :2]), (vol, o[:0], d[:0]),
                (torch.rand(2, 8, 9, 10), o, d)):
        with pytest.raises(ValueError):
            pj(*bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # shapes fine, tensors on the CPU: there is no CPU path
        pj(vol, o, d)


def test_ray_tensors_that_require_grad_need_ray_grad(hiplib):
    from differender_amd.projection import RayBundleProjector
    pj = RayBundleProjector((8, 8, 8), mode="max")
    vol = torch.rand(1, 8, 8, 8)
    for name in ("origins", "directions"):
        rays = dict(origins=torch.zeros(6, 3), directions=torch.ones(6, 3))
        rays[name].requires_grad_(True)
        with pytest.raises(ValueError, match=f"no gradient w.r.t. {name}.*ray_grad=True"):
            pj(vol, **rays)
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):   # (nothing to refuse without autograd)
            pj(vol, **rays)


def test_a_zero_length_direction_raises(hiplib):
    from differender_amd.projection import RayBundleProjector
    pj = RayBundleProjector((8, 8, 8), ray_grad=True)
    d = torch.ones(6, 3)
    d[4] = 0.0
    with pytest.raises(ValueError, match="zero length"):
        pj(torch.rand(1, 8, 8, 8), torch.zeros(6, 3), d)
