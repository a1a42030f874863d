"""What the GPU tests of the camera gradient share (test_gpu_camera_grad.py, test_gpu_camera_grad_edges.py): one launch of
F.march_fwd + F.march_bwd_cam on the ray buffers of the float64 reference (tests/golden/make_camgrad_golden.py), and D8's rule."""
import numpy as np
import torch


def launch(vol, tf, cams, refs, grad_outs, keeps, S, sr, seed=0, view_base=0, rows=None, upstream=None):
    """One launch over len(refs) views. vol, tf: device tensors as the kernels get them (shared or one item per view); cams
    (V, 3); refs: per view the reference's entry, exit, rays, n, steps; grad_outs (W, H, 4) and keeps (W, H) per view: only the
    rays in `keep` whose march stops where the reference's does get an upstream gradient. upstream: a function of the masked
    (V, W, H, 4) device tensor that returns the tensor to hand in instead.
    -> per-ray d_cam (V, W, H, 3) float64, totals (V, 3) float64, masks (V, W, H), the upstream gradient handed in."""
    from differender_amd import functional as F
    dev = torch.device("cuda")
    T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    stack = lambda k, dt=torch.float32: T(np.stack([np.asarray(r[k]) for r in refs]), dt)
    cam = T(np.asarray(cams, np.float64).reshape(-1, 3))
    e, x, r, n = stack("entry"), stack("exit"), stack("rays"), stack("n", torch.int32)
    out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, rows=rows)
    got = steps.cpu().numpy()
    masks = np.stack([(got[v] == refs[v]["steps"]) & (refs[v]["n"] > 1) & keeps[v] for v in range(len(refs))])
    # rays whose f32 march stops elsewhere, and n == 1 rays: zero upstream
    g = T(np.stack([grad_outs[v] * masks[v][..., None] for v in range(len(refs))]))
    if upstream is not None:
        g = upstream(g)
    d, d_ray = F.march_bwd_cam(vol, tf, cam, e, x, r, n, steps, S, sr, g, out, jitter_seed=seed, view_base=view_base, rows=rows,
                               per_ray=True)
    torch.cuda.synchronize()
    return d_ray.double().cpu().numpy(), d.double().cpu().numpy(), masks, g


def hip_per_ray(inp, ref, vol_dtype, keep):
    """(per-ray d_cam (W,H,3), total (3,), mask of the compared rays) of F.march_bwd_cam on the reference's ray buffers; only
    the rays in `keep` get an upstream gradient."""
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float32)
    ray, total, mask, _ = launch(T(inp["vol"]).to(vol_dtype), T(inp["tf"]), inp["cam"], [ref], [inp["grad_out"]], [keep],
                                 int(inp["max_samples"]), float(inp["sr"]), int(inp["jitter_seed"]), int(inp["view"]))
    return ray[0], total[0], mask[0]


def d8_total_rule(total, want_ray, ref32_ray, mask, what=None):
    """The total against the float64 sum: 3x the float32 transliteration's own error in that sum + 1e-4 of the sum of magnitudes."""
    err32_total = np.abs((ref32_ray - want_ray)[mask].sum(0)).max()
    want = want_ray * mask[..., None]
    err = np.abs(total - want.reshape(-1, 3).sum(0)).max()
    assert err <= 3.0 * err32_total + 1e-4 * np.abs(want).sum(), (what, err, err32_total, np.abs(want).sum())


def d8_rule(ray, total, ref, ref32, mask, what=None):
    """D8's rule as test_march_bwd_cam_matches_the_f64_reference states it, for one view (or one band of rows):
    per ray err <= 3 err32 + 1e-4 scale; the total equals the rays' sum to 1e-5 of their magnitudes, and the float64 sum to
    3x the f32 transliteration's error in that sum + 1e-4 of the sum of magnitudes. -> (err / scale, err32 / scale)."""
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum(), (what, mask.sum(), (ref["n"] > 1).sum())
    want = ref["dcam_ray"] * mask[..., None]
    scale = np.abs(want).max()
    err = np.abs(ray - want)[mask].max()
    err32 = np.abs(ref32["dcam_ray"] - ref["dcam_ray"])[mask].max()
    print("camgrad", what, "err/scale %.3g err32/scale %.3g rays %d" % (err / scale, err32 / scale, mask.sum()))
    assert np.isfinite(ray).all() and np.isfinite(total).all(), what
    assert (ray[~mask] == 0).all(), what
    assert err <= 3.0 * err32 + 1e-4 * scale, (what, err / scale, err32 / scale)
    assert np.abs(total - ray.sum((0, 1))).max() <= 1e-5 * np.abs(ray).sum(), what
    d8_total_rule(total, ref["dcam_ray"], ref32["dcam_ray"], mask, what)
    return err / scale, err32 / scale
