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


def test_views_of_one_launch_match_the_f64_reference(hiplib):
    views = _view_case()
    inp0 = views[0][0]
    ray, total, masks, _ = PG.launch(PG.dev(inp0["vol"]), PG.dev(inp0["tf"]), [i for i, _, _ in views], [r for _, r, _ in views],
                                     [PG.keep(r, r32) for _, r, r32 in views], int(inp0["max_samples"]), float(inp0["sr"]),
                                     VIEW_SEED, VIEW_BASE)
    for v, (inp, ref, ref32) in enumerate(views):
        PG.pose_rule(ray[v], total[v], ref, ref32, masks[v], ("view", v))
    assert np.abs(total[0] - total[1]).max() > 1e-3 * np.abs(total).max()


# ---- row bands: row0 != 0 against float64, and the bands' totals against the whole image's ------------------------------------------

def test_row_bands_match_the_rows_of_the_f64_reference_and_add_up(hiplib):
    Wimg, H = 22, 14
    inp = PG.inputs("a_orbit_sr1", WH=(Wimg, H), jitter_seed=np.int64(6021), look_from=np.array(CAMS[1]), **POSE)
    ref, ref32 = PG.refs(inp)
    vol, tf = PG.dev(inp["vol"]), PG.dev(inp["tf"])
    keep = PG.keep(ref, ref32)
    totals = []
    for row0, Wb in ((0, 7), (7, 9), (16, 6)):
        rows = slice(row0, row0 + Wb)
        band = lambda r: {k: r[k][rows] for k in ("entry", "exit", "rays", "n", "steps", "dpose_ray")}
        ray, total, masks, _ = PG.launch(vol, tf, [inp], [band(ref)], [keep[rows]], int(inp["max_samples"]), float(inp["sr"]),
                                         int(inp["jitter_seed"]), int(inp["view"]), rows=(row0, Wimg),
                                         grad_outs=[inp["grad_out"][rows]])
        PG.pose_rule(ray[0], total[0], band(ref), band(ref32), masks[0], ("band", row0, Wb))
        totals.append((total[0], masks[0]))
    mask = np.concatenate([m for _, m in totals], 0)
    PG.pose_total_rule(sum(t for t, _ in totals), ref["dpose_ray"], ref32["dpose_ray"], mask, "the bands' sum")


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
    ray, total, mask = PG.hip_per_ray(inp, ref, torch.float32, PG.keep(ref, ref32))
    PG.pose_rule(ray, total, ref, ref32, mask, ("R", R))


# ---- images smaller than a tile, workgroups with idle lanes and idle waves -----------------------------------------------------------

@pytest.mark.parametrize("WH", [(1, 1), (3, 5), (9, 17)], ids=lambda wh: "%dx%d" % wh)
def test_image_shapes_match_the_f64_reference_and_sum_up(hiplib, WH):
    inp = PG.inputs("a_orbit_sr1", WH=WH, jitter_seed=np.int64(77), look_from=np.array(CAMS[WH[0] % 3]), **POSE)
    ref, ref32 = PG.refs(inp)
    assert (ref["n"] > 1).any()
    ray, total, mask = PG.hip_per_ray(inp, ref, torch.float32, PG.keep(ref, ref32))
    PG.pose_rule(ray, total, ref, ref32, mask, ("image", WH))
    # idle lanes and idle waves add nothing to any of the four rounds of the workgroup's sum
    assert np.abs(total - ray.sum((0, 1))).max() <= 1e-5 * np.abs(ray).sum()
    assert np.abs(total).max() > 0   # (the centre ray of an odd image has u = v = 0: no d up, no d fov)


# ---- D5: a NaN upstream pixel ----------------------------------------------------------------------------------------------------------

def test_nan_upstream_gradients_contribute_nothing(hiplib):
    inp = PG.inputs("e_nonsquare", **POSE)
    ref, ref32 = PG.refs(inp)
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
    ray_n, total_n, masks, g = run(lambda g: torch.where(bad_t & chan, torch.full_like(g, float("nan")), g), keep)
    assert bool(torch.isnan(g).any(-1)[0][PG.dev(bad, torch.bool)].all())
    ray_0, total_0, masks_0, _ = run(None, keep & ~bad)
    assert (ray_n[0][bad] == 0).all() and np.isfinite(ray_n).all() and np.isfinite(total_n).all()
    ok = masks_0[0]
    assert np.array_equal(masks[0] & ~bad, ok) and ok.sum() > 0.6 * (ref["n"] > 1).sum()
    assert np.array_equal(ray_n[0][~bad], ray_0[0][~bad]) and (ray_0[0][ok] != 0).any(-1).all()
    assert np.abs(total_n[0] - ray_n[0].sum((0, 1))).max() <= 1e-5 * np.abs(ray_n[0]).sum()
    PG.pose_total_rule(total_n[0], ref["dpose_ray"], ref32["dpose_ray"], ok, "NaN upstream")
