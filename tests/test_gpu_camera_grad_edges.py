"""camera_grad_kernel where the fixtures of test_gpu_camera_grad.py do not reach: several views in one launch
(the view strides of volume and TF, the per-view jitter hash), row bands, the TF read from LDS and where it lies, images
smaller than a tile and workgroups with idle waves, rays that leave next to an edge of the box, non-finite upstream gradients
(D5), and the way through Raycaster with jitter. Every comparison is with the float64 autograd reference of tests/golden/make_camgrad_golden.py, run at test time on
the inputs the kernel reads, by D8's rule (camgrad_gpu.d8_rule) -- no other tolerance."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import camgrad_gpu as K  # noqa: E402
import make_camgrad_golden as CG  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
F16 = lambda a: np.asarray(a, np.float16).astype(np.float64)
CAMS = [(-1.3, 0.9, 2.0), (2.3, 0.5, -0.9), (0.8, -1.1, -2.1)]   # outside the box, off every axis and plane


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"), dt)


def _inputs(name, WH=None, **over):
    """The inputs of a fixture's case, rounded to what the kernel reads (float32), with other settings laid over them."""
    inp = CG.make_inputs(name)
    if WH is not None:
        inp["grad_out"] = np.random.RandomState(WH[0] * 100 + WH[1]).standard_normal((*WH, 4))
    inp.update(over)
    for k in ("vol", "tf", "cam", "grad_out"):
        inp[k] = F32(inp[k])
    return inp


def _refs(inp):
    return K.with_kinks(inp, CG.run_case(inp)), CG.run_case(inp, dtype=torch.float32)


def _keep(ref, ref32):
    return (ref32["steps"] == ref["steps"]) & (ref32["n"] == ref["n"])


# ---- views: blockIdx.y > 0, the view strides of the volume and the TF, the jitter hash of view_base + view -------------------

VIEW_BASE, VIEW_SEED = 5, 90210


@functools.lru_cache(maxsize=None)
def _view_case(batched):
    """Three cameras on case d's scene (18 x 22 x 16, R = 32, the opaque TF). batched: one volume (representable in float16, so
    that one reference serves both volume types) and one TF per view, all different."""
    base = _inputs("d_jitter", jitter_seed=np.int64(VIEW_SEED))
    rng = np.random.RandomState(17)
    views = []
    for v, cam in enumerate(CAMS):
        inp = dict(base, cam=F32(cam), view=np.int32(VIEW_BASE + v), grad_out=F32(rng.standard_normal(base["grad_out"].shape)))
        if batched:
            inp["vol"] = F16(np.clip(base["vol"] + 0.05 * rng.standard_normal(base["vol"].shape), 0.0, 1.0))
            tf = base["tf"].copy()
            tf[:, :3] = np.roll(tf[:, :3], 5 * v, axis=0) * rng.uniform(0.6, 1.0, size=(1, 3))
            tf[:, 3] *= 1.0 - 0.2 * v
            inp["tf"] = F32(tf)
        views.append((inp,) + _refs(inp))
    return views


def _launch_views(views, vol, tf, keeps=None, **kw):
    inp0 = views[0][0]
    keeps = [_keep(r, r32) for _, r, r32 in views] if keeps is None else keeps
    return K.launch(vol, tf, [i["cam"] for i, _, _ in views], [r for _, r, _ in views], [i["grad_out"] for i, _, _ in views],
                    keeps, int(inp0["max_samples"]), float(inp0["sr"]), VIEW_SEED, VIEW_BASE, **kw)


def _good(ref, ref32, what=None):
    """The keep mask of the second, conditioned pass (camgrad_gpu.well_conditioned)."""
    return K.well_conditioned(ref, ref32, _keep(ref, ref32), what=what)


def _both_passes(inp, ref, ref32, vol_dtype, what):
    """One view, one launch per pass: D8's rule over all compared rays, then over the well-conditioned ones alone.
    -> the first pass's (ray, total, mask)."""
    first = K.hip_per_ray(inp, ref, vol_dtype, _keep(ref, ref32))
    K.d8_rule(*first[:2], ref, ref32, first[2], what)
    ray, total, mask = K.hip_per_ray(inp, ref, vol_dtype, _good(ref, ref32, what))
    K.d8_rule(ray, total, ref, ref32, mask, (what, "conditioned"))
    return first


@pytest.mark.parametrize("kind", ["shared", "batched", "batched_permuted_f16"])
def test_views_of_one_launch_match_the_f64_reference(hiplib, kind):
    views = _view_case(kind != "shared")
    if kind == "shared":
        vol, tf = _dev(views[0][0]["vol"]), _dev(views[0][0]["tf"])
    else:
        vol, tf = _dev(np.stack([i["vol"] for i, _, _ in views])), _dev(np.stack([i["tf"] for i, _, _ in views]))
        assert not torch.equal(tf[0], tf[1]) and not torch.equal(vol[1], vol[2])
    if kind == "batched_permuted_f16":
        # the view Raycaster hands in: (BS, 1, D, H, W) storage seen in field order (BS, W, D, H), x contiguous
        vol = vol.half().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not vol.is_contiguous() and vol.stride(1) == 1
    ray, total, masks, _ = _launch_views(views, vol, tf)
    for v, (inp, ref, ref32) in enumerate(views):
        K.d8_rule(ray[v], total[v], ref, ref32, masks[v], (kind, "view", v))
    ray, total, masks, _ = _launch_views(views, vol, tf, keeps=[_good(r, r32, (kind, "view", v)) for v, (_, r, r32) in enumerate(views)])
    for v, (inp, ref, ref32) in enumerate(views):
        K.d8_rule(ray[v], total[v], ref, ref32, masks[v], (kind, "view", v, "conditioned"))


def test_the_jitter_draw_depends_on_the_view_index(hiplib):
    """Two views with the same camera, volume, TF and ray buffers differ only in the kernel's own draw u(seed, view_base + view,
    pixel), the weight of grad tmin in grad t0: the first is the reference's view, the second must not repeat it."""
    inp, ref, ref32 = _view_case(False)[0]
    twice = [(inp, ref, ref32)] * 2
    ray, total, masks, _ = _launch_views(twice, _dev(inp["vol"]), _dev(inp["tf"]))
    K.d8_rule(ray[0], total[0], ref, ref32, masks[0], "same buffers, view 0")
    m = masks[0] & masks[1]
    differ = (ray[0] != ray[1]).any(-1)[m]
    assert differ.mean() > 0.9, differ.mean()
    assert np.abs(ray[0] - ray[1])[m].max() > 1e-3 * np.abs(ray[0]).max()
    ray, total, masks, _ = _launch_views(twice, _dev(inp["vol"]), _dev(inp["tf"]), keeps=[_good(ref, ref32, "same buffers")] * 2)
    K.d8_rule(ray[0], total[0], ref, ref32, masks[0], "same buffers, view 0, conditioned")


# ---- row bands: row0 != 0 against float64 ----------------------------------------------------------------------------------

BANDS = ((0, 7), (7, 9), (16, 6))   # (row0, rows) of a 22-row image


@functools.lru_cache(maxsize=None)
def _band_case():
    inp = _inputs("a_orbit_sr1", WH=(22, 14), jitter_seed=np.int64(6021), cam=np.array(CAMS[1]))
    return (inp,) + _refs(inp)


def test_row_bands_match_the_rows_of_the_f64_reference(hiplib):
    inp, ref, ref32 = _band_case()
    Wimg = ref["n"].shape[0]
    vol, tf = _dev(inp["vol"]), _dev(inp["tf"])
    # the second pass: the well-conditioned rays of the whole image (one scale), band by band
    for keep, tag in ((_keep(ref, ref32), ()), (_good(ref, ref32, "bands"), ("conditioned",))):
        totals = []
        for row0, Wb in BANDS:
            rows = slice(row0, row0 + Wb)
            band = lambda r: {k: r[k][rows] for k in ("entry", "exit", "rays", "n", "steps", "dcam_ray")}
            ray, total, masks, _ = K.launch(vol, tf, inp["cam"], [band(ref)], [inp["grad_out"][rows]], [keep[rows]],
                                            int(inp["max_samples"]), float(inp["sr"]), int(inp["jitter_seed"]), int(inp["view"]),
                                            rows=(row0, Wimg))
            K.d8_rule(ray[0], total[0], band(ref), band(ref32), masks[0], ("band", row0, Wb) + tag)
            totals.append((total[0], masks[0]))
        mask = np.concatenate([m for _, m in totals], 0)
        K.d8_total_rule(sum(t for t, _ in totals), ref["dcam_ray"], ref32["dcam_ray"], mask, ("the bands' sum",) + tag)


# ---- the TF in LDS (R <= 3072) and read where it lies (R > 3072) -----------------------------------------------------------------

def _lds_limit_bytes():
    """The dispatch constant of cam_dispatch (csrc/camera_grad.hip), read from its source."""
    src = open(os.path.join(ROOT, "differender_amd", "csrc", "camera_grad.hip")).read()
    m = re.search(r"const size_t lds = \(size_t\)a\.R \* sizeof\(float4\);\s*if \(lds <= (\d+) \* 1024\) return launch_tiles\("
                  r"camera_grad_kernel<VT, true>", src)
    assert m, "cam_dispatch no longer reads as this test expects"
    return int(m.group(1)) * 1024


@functools.lru_cache(maxsize=None)
def _table_case(R, f16):
    x = np.linspace(0.0, 1.0, R)[:, None]
    rng = np.random.RandomState(R)
    tf = 0.5 + 0.4 * np.sin(rng.uniform(3.0, 9.0, size=(1, 4)) * x + rng.uniform(0.0, 6.0, size=(1, 4)))
    tf[:, 3] = 0.01 + 0.05 * x[:, 0] ** 2
    inp = _inputs("a_orbit_sr1", tf=tf, cam=np.array(CAMS[0]))
    if f16:
        inp["vol"] = F16(inp["vol"])
    return (inp,) + _refs(inp)


@pytest.mark.parametrize("vol_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("R", [3072, 3073, 4096])
def test_table_in_lds_and_in_memory_match_the_f64_reference(hiplib, R, vol_dtype):
    limit = _lds_limit_bytes()
    assert 3072 * 16 <= limit < 3073 * 16   # 3072 is the last table staged in LDS, 3073 the first read where it lies
    inp, ref, ref32 = _table_case(R, vol_dtype == torch.float16)
    _both_passes(inp, ref, ref32, vol_dtype, ("R", R, "LDS" if R * 16 <= limit else "memory", str(vol_dtype)))


# ---- images smaller than a tile, workgroups with idle lanes and idle waves -------------------------------------------------------

SHAPES = [(1, 1), (3, 5), (8, 8), (9, 17), (33, 7)]


@functools.lru_cache(maxsize=None)
def _shape_case(WH):
    # (1 x 1 from CAMS[2]: the one ray of CAMS[1] lies next to a kink, its float32 reference 2e-3 of its own gradient off)
    inp = _inputs("a_orbit_sr1", WH=WH, jitter_seed=np.int64(77), cam=np.array(CAMS[2 if WH == (1, 1) else WH[0] % 3]))
    return (inp,) + _refs(inp)


@pytest.mark.parametrize("WH", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_image_shapes_match_the_f64_reference_and_sum_up(hiplib, WH):
    inp, ref, ref32 = _shape_case(WH)
    assert (ref["n"] > 1).any()
    ray, total, mask = _both_passes(inp, ref, ref32, torch.float32, ("image", WH))
    # idle lanes and idle waves add nothing to the workgroup's sum (the rule above already holds it to 1e-5 of sum |ray|)
    assert np.abs(total - ray.sum((0, 1))).max() <= 1e-5 * np.abs(ray).sum()
    assert np.abs(total).max() > 0


# ---- taps outside the box: the position predicates of tri_sample_grad ------------------------------------------------------------

# Between entry and exit a sample lies inside the box, and the slope of the last sample along its own exit axis cancels against
# grad tmax, so the predicates 0 < y && !(1 < y) only show where a ray leaves within the normal's tap distance (1e-3) of a second
# face: one tap then lies outside the box, where clamp holds the position and the slope is 0. Fixture o does this for the
# upper y face; these poses (found like it, see make_camgrad_golden.CASES) put eight rays of a row or column 5e-4 inside the
# other faces.
GRAZING = {"x_lower": ((2.4, 0.1981, 0.0), 0, -1.0), "x_upper": ((-2.4, 0.1981, 0.0), 0, 1.0), "y_lower": ((-2.4, -0.1994, 0.0), 1, -1.0),
           "z_upper": ((-2.4, 0.0, 0.1994), 2, 1.0), "z_lower": ((2.4, 0.0, -0.1994), 2, -1.0)}


@functools.lru_cache(maxsize=None)
def _grazing_case(name):
    inp = _inputs("o_edge_grazing", cam=np.array(GRAZING[name][0]))
    return (inp,) + _refs(inp)


def _grazing_rays(name, inp, ref):
    _, axis, sign = GRAZING[name]
    last = inp["cam"] + ref["exit"][..., None] * ref["rays"]
    gap = 1.0 - sign * last[..., axis]
    return (gap > 2e-4) & (gap < 8e-4) & ((1.0 - np.abs(last) < 1e-9).sum(-1) == 1) & (ref["n"] > 1)


@pytest.mark.parametrize("name", sorted(GRAZING))
def test_rays_leaving_next_to_an_edge_match_the_f64_reference(hiplib, name):
    inp, ref, ref32 = _grazing_case(name)
    grazing = _grazing_rays(name, inp, ref)
    assert grazing.sum() >= 6, grazing.sum()
    # (the conditioned pass keeps grazing rays too: tests/test_camera_grad.py holds the case to that)
    assert (grazing & _good(ref, ref32)).sum() >= 6
    ray, total, mask = _both_passes(inp, ref, ref32, torch.float32, ("grazing", name))
    assert mask[grazing].all()


# ---- D5: non-finite upstream gradients ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _d5_case():
    inp = _inputs("e_nonsquare")
    return (inp,) + _refs(inp)


def _d5_launch(upstream, keep_extra=None):
    inp, ref, ref32 = _d5_case()
    keep = _keep(ref, ref32) if keep_extra is None else _keep(ref, ref32) & keep_extra
    return K.launch(_dev(inp["vol"]), _dev(inp["tf"]), inp["cam"], [ref], [inp["grad_out"]], [keep], int(inp["max_samples"]),
                    float(inp["sr"]), int(inp["jitter_seed"]), int(inp["view"]), upstream=upstream)


def test_nan_upstream_gradients_contribute_nothing(hiplib):
    inp, ref, ref32 = _d5_case()
    W, H = ref["n"].shape
    bad = np.zeros(W * H, bool)
    bad[np.random.RandomState(3).choice(W * H, W * H // 4, replace=False)] = True
    bad = bad.reshape(W, H)
    assert (bad & (ref["n"] > 1)).sum() > 20
    bad_t = _dev(bad, torch.bool)[None, ..., None]
    # a NaN in one channel, in all four, and in between
    chan = _dev(np.random.RandomState(4).rand(1, W, H, 4) < 0.5, torch.bool)
    chan[..., 0] |= ~chan.any(-1)
    nans = lambda g: torch.where(bad_t & chan, torch.full_like(g, float("nan")), g)
    ray_n, total_n, masks, g = _d5_launch(nans)
    assert bool(torch.isnan(g).any(-1)[0][_dev(bad, torch.bool)].all())
    ray_0, total_0, masks_0, _ = _d5_launch(None, keep_extra=~bad)
    assert (ray_n[0][bad] == 0).all() and np.isfinite(ray_n).all()
    ok = masks_0[0]
    assert np.array_equal(masks[0] & ~bad, ok) and ok.sum() > 0.6 * (ref["n"] > 1).sum()
    assert np.array_equal(ray_n[0][~bad], ray_0[0][~bad]) and (ray_0[0][ok] != 0).any(-1).all()
    assert np.isfinite(total_n).all()
    assert np.abs(total_n[0] - ray_n[0].sum((0, 1))).max() <= 1e-5 * np.abs(ray_n[0]).sum()
    K.d8_total_rule(total_n[0], ref["dcam_ray"], ref32["dcam_ray"], ok, "NaN upstream")
    # the same total over the well-conditioned rays alone, the NaN pixels still in the upstream gradient
    ray_c, total_c, masks_c, g = _d5_launch(nans, keep_extra=_good(ref, ref32, "NaN upstream"))
    assert bool(torch.isnan(g).any(-1)[0][_dev(bad, torch.bool)].all()) and np.isfinite(total_c).all()
    K.d8_total_rule(total_c[0], ref["dcam_ray"], ref32["dcam_ray"], masks_c[0] & ~bad, "NaN upstream, conditioned")


def test_infinite_upstream_gradients_are_clamped(hiplib):
    inp, ref, ref32 = _d5_case()
    W, H = ref["n"].shape
    live = np.flatnonzero(((ref["n"] > 1) & _keep(ref, ref32)).reshape(-1))
    pick = np.random.RandomState(5).choice(live, 6, replace=False)
    hot = np.zeros(W * H, bool); hot[pick] = True
    hot = hot.reshape(W, H)
    inf = float("inf")

    def poke(g):
        g = g.clone().reshape(-1, 4)
        for k, (p, s) in enumerate(zip(pick, (inf, -inf, inf, -inf, -inf, inf))):
            g[p, k % 4] = s          # one channel each ...
        g[pick[5], :] = inf          # ... and all four of one ray
        return g.reshape(1, W, H, 4)

    ray_i, total_i, masks, g = _d5_launch(poke)
    assert int(torch.isinf(g).sum()) == 9
    ray_0, total_0, masks_0, _ = _d5_launch(None, keep_extra=~hot)
    assert masks[0][hot].all()
    assert np.isfinite(ray_i).all() and np.abs(ray_i[0][hot]).max() <= 1e30
    assert np.array_equal(ray_i[0][~hot], ray_0[0][~hot]) and (ray_0[0][masks_0[0]] != 0).any(-1).all()
    assert np.isfinite(total_i).all()


# ---- what the conditioned pass is fed, for tests/test_camera_grad.py to hold to its conditions without a GPU -------------------

def _band_parts():
    inp, ref, ref32 = _band_case()
    return [(ref, ref32, _keep(ref, ref32), [slice(r0, r0 + wb) for r0, wb in BANDS])]


# id -> a function that returns [(float64 reference, float32 reference, keep mask, row bands or None)], one entry per view
CONDITIONED = {"bands": _band_parts, "d5_e_nonsquare": lambda: [_d5_case()[1:] + (_keep(*_d5_case()[1:]), None)]}
for _b in (False, True):
    CONDITIONED["views_%s" % ("batched" if _b else "shared")] = lambda b=_b: [(r, r32, _keep(r, r32), None) for _, r, r32 in _view_case(b)]
for _R in (3072, 3073, 4096):
    for _f16 in (False, True):
        CONDITIONED["table_%d_%s" % (_R, "f16" if _f16 else "f32")] = \
            lambda R=_R, f=_f16: [_table_case(R, f)[1:] + (_keep(*_table_case(R, f)[1:]), None)]
for _wh in SHAPES:
    CONDITIONED["image_%dx%d" % _wh] = lambda wh=_wh: [_shape_case(wh)[1:] + (_keep(*_shape_case(wh)[1:]), None)]
for _n in sorted(GRAZING):
    CONDITIONED["grazing_" + _n] = lambda n=_n: [_grazing_case(n)[1:] + (_keep(*_grazing_case(n)[1:]), None)]


# ---- through Raycaster, with jitter ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _module_case(kind, seed):
    """Case d's scene at 20 x 16: per view the inputs and the references, views 0 and 1 of the module's own launch."""
    base = _inputs("d_jitter", WH=(20, 16), jitter_seed=np.int64(seed))
    rng = np.random.RandomState(23)
    views = []
    for v in range(2):
        inp = dict(base, view=np.int32(v), grad_out=F32(rng.standard_normal(base["grad_out"].shape)))
        if kind == "shared_cam_batched_vol":
            inp["vol"] = F32(np.clip(base["vol"] + 0.05 * rng.standard_normal(base["vol"].shape), 0.0, 1.0))
        else:
            inp["cam"] = F32(CAMS[v])
        views.append((inp,) + _refs(inp))
    return views


@pytest.mark.parametrize("kind", ["batched_cams", "shared_cam_batched_vol", "float64_look_from"])
def test_raycaster_with_jitter_matches_the_f64_reference(hiplib, kind):
    from differender_amd import functional as F
    from differender_amd.volume_raycaster import Raycaster
    k = 1357
    torch.manual_seed(k)
    seed = F.new_jitter_seed()
    assert seed != 0
    views = _module_case("shared_cam_batched_vol" if kind == "shared_cam_batched_vol" else "batched_cams", seed)
    inp0 = views[0][0]
    WH, S, sr = inp0["grad_out"].shape[:2], int(inp0["max_samples"]), float(inp0["sr"])
    # the module's layouts: volume ([BS,] 1, D, H, W) whose field order is (W, D, H); tf ([BS,] 4, R); image ([BS,] 4, H, W)
    user_vol = lambda a: _dev(a).permute(1, 2, 0)[None].contiguous()
    if kind == "shared_cam_batched_vol":
        vol = torch.stack([user_vol(i["vol"]) for i, _, _ in views])
        lf0 = _dev(inp0["cam"])
    else:
        vol = user_vol(inp0["vol"])
        lf0 = _dev(np.stack([i["cam"] for i, _, _ in views]), torch.float64 if kind == "float64_look_from" else torch.float32)
    tf = _dev(inp0["tf"]).t().contiguous()
    rc = Raycaster(tuple(vol.shape[-3:]), WH, tf.shape[-1], sampling_rate=sr, jitter=True, max_samples=S)

    # the rays the module will march (its own float32 ray setup, the replayed seed): the compared rays are those whose sample
    # count and live samples are the reference's, in float32 and float64 alike
    batched, _, vol_in, tf_in, lf_in = rc._determine_batch(vol, tf, lf0)
    assert batched
    cam = lf_in.reshape(-1, 3).float().contiguous()
    e, x, r, n = F.ray_setup(cam, WH, vol_in.shape[-3:], sr, jitter_seed=seed)
    steps = F.march_fwd(vol_in, tf_in.float().contiguous(), cam, e, x, r, n, S, sr)[1]
    n, steps = n.cpu().numpy(), steps.cpu().numpy()
    masks = [(n[v] == ref["n"]) & (steps[v] == ref["steps"]) & _keep(ref, ref32) & (ref["n"] > 1)
             for v, (_, ref, ref32) in enumerate(views)]
    for m, (_, ref, _) in zip(masks, views):
        assert m.sum() > 0.8 * (ref["n"] > 1).sum()
    g = _dev(np.stack([i["grad_out"] * m[..., None] for m, (i, _, _) in zip(masks, views)]))   # (BS, W, H, 4)
    w = g.permute(0, 3, 2, 1).flip(-2)                                                          # (BS, 4, H, W)
    assert torch.equal(w.flip(-2).permute(0, 3, 2, 1), g)

    lf = lf0.clone().requires_grad_(True)
    torch.manual_seed(k)
    (rc(vol, tf, lf) * w).sum().backward()
    got = lf.grad
    assert got.shape == lf0.shape and got.dtype == lf0.dtype
    got = got.double().cpu().numpy()
    if kind == "shared_cam_batched_vol":   # one camera, expanded to the views: the sum over them
        want = np.concatenate([ref["dcam_ray"] for _, ref, _ in views], 0)
        want32 = np.concatenate([ref32["dcam_ray"] for _, _, ref32 in views], 0)
        K.d8_total_rule(got, want, want32, np.concatenate(masks, 0), kind)
    else:
        for v, (_, ref, ref32) in enumerate(views):
            K.d8_total_rule(got[v], ref["dcam_ray"], ref32["dcam_ray"], masks[v], (kind, v))
