"""The pose gradient where the cases of test_gpu_pose.py do not reach: several views in one launch (each with
its own pose and fov), row bands, the TF read from LDS and where it lies, images smaller than a tile, and a NaN upstream
gradient (D5). Every comparison is with the float64 autograd reference of tests/pose_reference.py, run at test time on the
inputs the kernel reads, by D8's rule for each pose tensor (pose_gpu.pose_rule) -- no other tolerance."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_gpu as PG  # noqa: E402

pytestmark = pytest.mark.gpu

CAMS = [(-1.3, 0.9, 2.0), (2.3, 0.5, -0.9), (0.8, -1.1, -2.1)]
POSE = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(27.0))
VIEW_POSES = [POSE, dict(look_at=(-0.15, 0.2, 0.1), up=(-0.2, 1.0, 0.25), fov_rad=math.radians(33.0)),
              dict(look_at=(0.1, 0.1, -0.2), up=(0.1, 0.9, 0.35), fov_rad=math.radians(22.0))]
VIEW_BASE, VIEW_SEED = 5, 90210


# ---- views: blockIdx.y > 0, each view's own pose row and fov, the jitter hash of view_base + view -----------------------------------

@functools.lru_cache(maxsize=None)
def _view_case():
    base = PG.inputs("d_jitter", jitter_seed=np.int64(VIEW_SEED))
    rng = np.random.RandomState(17)
    views = []
    for v, cam in enumerate(CAMS):
        inp = dict(base, view=np.int32(VIEW_BASE + v), grad_out=PG.F32(rng.standard_normal(base["grad_out"].shape)),
                   **{k: PG.F32(a) for k, a in dict(VIEW_POSES[v], look_from=cam).items()})
        views.append((inp,) + PG.refs(inp))
    return views


def _launch_views(views, keeps, upstream=None):
    inp0 = views[0][0]
    return PG.launch(PG.dev(inp0["vol"]), PG.dev(inp0["tf"]), [i for i, _, _ in views], [r for _, r, _ in views], keeps,
                     int(inp0["max_samples"]), float(inp0["sr"]), VIEW_SEED, VIEW_BASE, upstream=upstream)


def test_views_of_one_launch_match_the_f64_reference(hiplib):
    views = _view_case()
    ray, total, masks, _ = _launch_views(views, [PG.keep(r, r32) for _, r, r32 in views])
    for v, (inp, ref, ref32) in enumerate(views):
        PG.pose_rule(ray[v], total[v], ref, ref32, masks[v], ("view", v))
    assert np.abs(total[0] - total[1]).max() > 1e-3 * np.abs(total).max()
    ray, total, masks, _ = _launch_views(views, [PG.well_conditioned(r, r32, PG.keep(r, r32), ("view", v))
                                                 for v, (_, r, r32) in enumerate(views)])
    for v, (inp, ref, ref32) in enumerate(views):
        PG.pose_rule(ray[v], total[v], ref, ref32, masks[v], ("view", v, "conditioned"))


# ---- a view that misses the box, next to one that does not ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _missing_view_case():
    """View 0 of _view_case and a second view of the same scene that looks away from the box (look_at = 2 look_from)."""
    seen = _view_case()[0]
    away = dict(seen[0], view=np.int32(VIEW_BASE + 1), look_at=PG.F32(2.0 * np.asarray(seen[0]["look_from"])))
    return [seen, (away,) + PG.refs(away)]


def test_a_view_that_misses_the_box_gives_zeros_next_to_one_that_does_not(hiplib):
    views = _missing_view_case()
    (_, ref, ref32), (_, miss, miss32) = views
    assert (miss["n"] <= 1).all() and (miss32["n"] <= 1).all() and (miss["dpose_ray"] == 0).all()
    everything = np.ones(miss["n"].shape, bool)
    full = PG.dev(views[1][0]["grad_out"])   # the missing view's whole upstream gradient reaches the kernel, unmasked
    for keep, tag in ((PG.keep(ref, ref32), ()), (PG.well_conditioned(ref, ref32, PG.keep(ref, ref32), "next to a miss"), ("conditioned",))):
        ray, total, masks, g = _launch_views(views, [keep, everything], upstream=lambda g: torch.stack([g[0], full]))
        assert not masks[1].any() and float(g[1].abs().min()) > 0
        assert np.isfinite(ray[1]).all() and (ray[1] == 0).all() and np.isfinite(total[1]).all() and (total[1] == 0).all()
        PG.pose_rule(ray[0], total[0], ref, ref32, masks[0], ("next to a miss",) + tag)


# ---- row bands: row0 != 0 against float64, and the bands' totals against the whole image's ------------------------------------------

BANDS = ((0, 7), (7, 9), (16, 6))   # (row0, rows) of a 22-row image


@functools.lru_cache(maxsize=None)
def _band_case():
    inp = PG.inputs("a_orbit_sr1", WH=(22, 14), jitter_seed=np.int64(6021), look_from=np.array(CAMS[1]), **POSE)
    return (inp,) + PG.refs(inp)


def test_row_bands_match_the_rows_of_the_f64_reference_and_add_up(hiplib):
    inp, ref, ref32 = _band_case()
    Wimg = ref["n"].shape[0]
    vol, tf = PG.dev(inp["vol"]), PG.dev(inp["tf"])
    # the second pass: the well-conditioned rays of the whole image (one scale per tensor), band by band
    for keep, tag in ((PG.keep(ref, ref32), ()), (PG.well_conditioned(ref, ref32, PG.keep(ref, ref32), "bands"), ("conditioned",))):
        totals = []
        for row0, Wb in BANDS:
            rows = slice(row0, row0 + Wb)
            band = lambda r: {k: r[k][rows] for k in ("entry", "exit", "rays", "n", "steps", "dpose_ray")}
            ray, total, masks, _ = PG.launch(vol, tf, [inp], [band(ref)], [keep[rows]], int(inp["max_samples"]), float(inp["sr"]),
                                             int(inp["jitter_seed"]), int(inp["view"]), rows=(row0, Wimg),
                                             grad_outs=[inp["grad_out"][rows]])
            PG.pose_rule(ray[0], total[0], band(ref), band(ref32), masks[0], ("band", row0, Wb) + tag)
            totals.append((total[0], masks[0]))
        mask = np.concatenate([m for _, m in totals], 0)
        PG.pose_total_rule(sum(t for t, _ in totals), ref["dpose_ray"], ref32["dpose_ray"], mask, ("the bands' sum",) + tag)


# ---- the TF in LDS (R <= 3072) and read where it lies (R > 3072) ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _table_case(R):
    x = np.linspace(0.0, 1.0, R)[:, None]
    rng = np.random.RandomState(R)
    tf = 0.5 + 0.4 * np.sin(rng.uniform(3.0, 9.0, size=(1, 4)) * x + rng.uniform(0.0, 6.0, size=(1, 4)))
    tf[:, 3] = 0.01 + 0.05 * x[:, 0] ** 2
    inp = PG.inputs("a_orbit_sr1", tf=tf, look_from=np.array(CAMS[0]), **POSE)
    return (inp,) + PG.refs(inp)


@pytest.mark.parametrize("R", [3072, 3073])
def test_table_in_lds_and_in_memory_match_the_f64_reference(hiplib, R):
    # (3072 texels of 16 B are the last table cam_dispatch stages in LDS; the pose instances share the fixed camera's tiers)
    inp, ref, ref32 = _table_case(R)
    PG.both_passes(inp, ref, ref32, torch.float32, ("R", R))


# ---- images smaller than a tile, workgroups with idle lanes and idle waves -----------------------------------------------------------

SHAPES = [(1, 1), (3, 5), (9, 17)]


@functools.lru_cache(maxsize=None)
def _shape_case(WH):
    # (1 x 1 from CAMS[2]: the one ray of CAMS[1] lies next to a kink, where its float32 reference is off in the third digit)
    cam = CAMS[2 if WH == (1, 1) else WH[0] % 3]
    inp = PG.inputs("a_orbit_sr1", WH=WH, jitter_seed=np.int64(77), look_from=np.array(cam), **POSE)
    return (inp,) + PG.refs(inp)


@pytest.mark.parametrize("WH", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_image_shapes_match_the_f64_reference_and_sum_up(hiplib, WH):
    inp, ref, ref32 = _shape_case(WH)
    assert (ref["n"] > 1).any()
    ray, total, mask = PG.both_passes(inp, ref, ref32, torch.float32, ("image", WH))
    # idle lanes and idle waves add nothing to any of the four rounds of the workgroup's sum
    assert np.abs(total - ray.sum((0, 1))).max() <= 1e-5 * np.abs(ray).sum()
    assert np.abs(total).max() > 0   # (the centre ray of an odd image has u = v = 0: no d up, no d fov)


# ---- D5: a NaN upstream pixel ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _d5_case():
    inp = PG.inputs("e_nonsquare", **POSE)
    return (inp,) + PG.refs(inp)


def test_nan_upstream_gradients_contribute_nothing(hiplib):
    inp, ref, ref32 = _d5_case()
    W, H = ref["n"].shape
    bad = np.zeros(W * H, bool)
    bad[np.random.RandomState(3).choice(W * H, W * H // 4, replace=False)] = True
    bad = bad.reshape(W, H)
    assert (bad & (ref["n"] > 1)).sum() > 20
    bad_t = PG.dev(bad, torch.bool)[None, ..., None]
    chan = PG.dev(np.random.RandomState(4).rand(1, W, H, 4) < 0.5, torch.bool)   # a NaN in one channel, in all four, and in between
    chan[..., 0] |= ~chan.any(-1)

    def run(upstream, keep):
        return PG.launch(PG.dev(inp["vol"]), PG.dev(inp["tf"]), [inp], [ref], [keep], int(inp["max_samples"]), float(inp["sr"]),
                         int(inp["jitter_seed"]), int(inp["view"]), upstream=upstream)

    keep = PG.keep(ref, ref32)
    nans = lambda g: torch.where(bad_t & chan, torch.full_like(g, float("nan")), g)
    ray_n, total_n, masks, g = run(nans, keep)
    assert bool(torch.isnan(g).any(-1)[0][PG.dev(bad, torch.bool)].all())
    ray_0, total_0, masks_0, _ = run(None, keep & ~bad)
    assert (ray_n[0][bad] == 0).all() and np.isfinite(ray_n).all() and np.isfinite(total_n).all()
    ok = masks_0[0]
    assert np.array_equal(masks[0] & ~bad, ok) and ok.sum() > 0.6 * (ref["n"] > 1).sum()
    assert np.array_equal(ray_n[0][~bad], ray_0[0][~bad]) and (ray_0[0][ok] != 0).any(-1).all()
    assert np.abs(total_n[0] - ray_n[0].sum((0, 1))).max() <= 1e-5 * np.abs(ray_n[0]).sum()
    PG.pose_total_rule(total_n[0], ref["dpose_ray"], ref32["dpose_ray"], ok, "NaN upstream")
    # the same total over the well-conditioned rays alone, the NaN pixels still in the upstream gradient
    ray_c, total_c, masks_c, g = run(nans, PG.well_conditioned(ref, ref32, keep, "NaN upstream"))
    assert bool(torch.isnan(g).any(-1)[0][PG.dev(bad, torch.bool)].all()) and np.isfinite(total_c).all()
    PG.pose_total_rule(total_c[0], ref["dpose_ray"], ref32["dpose_ray"], masks_c[0] & ~bad, "NaN upstream, conditioned")


# ---- what the conditioned pass is fed, for tests/test_pose.py to hold to its conditions without a GPU -----------------------------

def _one(case, bands=None):
    _, ref, ref32 = case
    return [(ref, ref32, PG.keep(ref, ref32), bands)]


# id -> a function that returns [(float64 reference, float32 reference, keep mask, row bands or None)], one entry per view
CONDITIONED = {"views": lambda: [e for c in _view_case() for e in _one(c)],
               "next_to_a_miss": lambda: _one(_missing_view_case()[0]),
               "bands": lambda: _one(_band_case(), [slice(r0, r0 + wb) for r0, wb in BANDS]),
               "d5_e_nonsquare": lambda: _one(_d5_case())}
for _R in (3072, 3073):
    CONDITIONED["table_%d" % _R] = lambda R=_R: _one(_table_case(R))
for _wh in SHAPES:
    CONDITIONED["image_%dx%d" % _wh] = lambda wh=_wh: _one(_shape_case(wh))
