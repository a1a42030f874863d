"""What the GPU tests of the lit march share (test_gpu_lighting.py, test_gpu_lighting_edges.py): a light_cases
scene on the device, one forward on the kernels' own ray buffers with the float64 / float32 transliterations
(tests/light_reference.py) run on those buffers, D8's bar, and the comparison of every output of the backward with it."""
import functools

import numpy as np
import torch

import light_cases as LC

DEV = torch.device("cuda")
C = lambda t: t.detach().double().cpu().numpy()


def functional():
    from differender_amd import functional as F
    return F


def native():
    from differender_amd import _native as N
    return N


def upload(sc):
    """A light_cases scene on the device -> (vol, tf, cam, light); a per-view scene's vol is (V,VX,VY,VZ) and its tf (V,R,4)."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
    vol = f(sc["vol"])
    return (vol.half() if sc["f16"] else vol), f(sc["tf"]), f(sc["cam"]), f(sc["light"])


def bound(got, want, want32, what, per_column=False, err32=None, skip=()):
    """D8's bar: error <= 3 x the f32 transliteration's own error + 1e-5 of the largest reference element. per_column: the
    bar must ALSO hold for each of the last axis's columns by itself -- the ten lighting gradients differ by three orders of
    magnitude, and the small ones would otherwise hide under the floor of the large ones. err32: the f32 transliteration's own
    error where it is not max |want32 - want| (the columns' errors, for per_column). skip: columns per_column leaves to the
    caller (those a scene declares exactly zero: they have no scale)."""
    if per_column:
        for k in range(want.shape[-1]):
            if k not in skip:
                bound(got[..., k], want[..., k], want32[..., k], f"{what}[{k}]", err32=None if err32 is None else err32[k])
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    err32 = np.abs(want32 - want).max() if err32 is None else np.max(err32)
    print(f"{what}: err {err:.3e} err32 {err32:.3e} scale {scale:.3e}")
    assert scale > 0, what
    assert np.isfinite(got).all(), what
    assert err <= 3.0 * err32 + 1e-5 * scale, (what, err / scale, err32 / scale)


@functools.lru_cache(maxsize=None)
def forward_state(name):
    """Differentiable scene `name`: its device tensors, the kernels' ray buffers and forward, and light_cases.reference_state on
    those buffers (the references are computed once per scene and shared; nobody writes to them).
    -> dict(sc, vol, tf, cam, light, rays (entry, exit, rays, n), out, steps, st)."""
    F = functional()
    sc = LC.scene(name)
    vol, tf, cam, light = upload(sc)
    S, sr = sc["max_samples"], sc["sr"]
    rays = F.ray_setup(cam, sc["WH"], vol.shape[-3:], sr, jitter_seed=sc["jitter"])
    out, steps = F.march_lit_fwd(vol, tf, cam, light, *rays, S, sr)
    e, x, r, n = rays
    st = LC.reference_state(sc, C(e), C(x), C(r), n.cpu().numpy(), steps.cpu().numpy())
    return dict(sc=sc, vol=vol, tf=tf, cam=cam, light=light, rays=rays, out=out, steps=steps, st=st)


def compare(name):
    """The kernels' rgba, d_vol, d_tf, per-ray d_light and d_light of scene `name` against the float64 transliteration, column by
    column, by D8's rule. A per-view scene's d_vol and d_tf are held to it view by view, and no two views' may agree (a view
    stride of 0 would write them all into one). A column the scene declares zero must be exactly 0 (-0.0 passes) and finite, in
    d_light and in every kept ray's entry; all the others keep the requirement of a positive reference and D8's bar."""
    F = functional()
    fs = forward_state(name)
    sc, st, vol, tf, cam, light, out, steps = (fs[k] for k in ("sc", "st", "vol", "tf", "cam", "light", "out", "steps"))
    e, x, r, n = fs["rays"]
    S, sr, zero = sc["max_samples"], sc["sr"], sc["zero"]
    gm = torch.from_numpy(st["gm"]).float().to(DEV)
    d_vol, d_tf, d_light, d_ray = F.march_lit_bwd(vol, tf, cam, light, e, x, r, n, S, sr, gm, out, per_ray=True)
    ref, ref32, mask = st["ref"], st["ref32"], st["mask"]
    m4 = mask[..., None]
    bound(C(out) * m4, ref["rgba"] * m4, ref32["rgba"] * m4, "rgba")
    if sc["per_view"]:
        V = mask.shape[0]
        for k, got in (("dvol", C(d_vol)), ("dtf", C(d_tf))):
            assert got.shape == ref[k].shape and got.shape[0] == V
            for v in range(V):
                bound(got[v], ref[k][v], ref32[k][v], f"{k} view {v}")
            big = np.abs(got).max()
            assert all(np.abs(got[a] - got[b]).max() > 1e-3 * big for a in range(V) for b in range(a)), k
    else:
        bound(C(d_vol), ref["dvol"], ref32["dvol"], "dvol")
        bound(C(d_tf), ref["dtf"], ref32["dtf"], "dtf")
    bound(C(d_ray) * m4, ref["dlight_ray"] * m4, ref32["dlight_ray"] * m4, "dlight_ray")
    # ... and column by column, over the rays together: the ten gradients differ by three orders of magnitude, and the small
    # ones would hide under the floor of the large ones. A column's LARGEST per-ray error is one ray's rounding noise in the
    # cancellation-prone terms (the normal, the light direction's projection), which two f32 programs of different operation
    # order do not share; the rays' absolute errors SUMMED are a statistic both programs do share.
    sum_abs = lambda a: (np.abs(a) * m4).sum((0, 1, 2))
    col, col32, colref = sum_abs(C(d_ray) - ref["dlight_ray"]), sum_abs(ref32["dlight_ray"] - ref["dlight_ray"]), sum_abs(ref["dlight_ray"])
    for k in range(10):
        print(f"dlight_ray summed abs error [{k}]: err {col[k]:.3e} err32 {col32[k]:.3e} scale {colref[k]:.3e}")
        if k in zero:
            assert colref[k] == 0 and np.isfinite(C(d_ray)[..., k]).all() and np.isfinite(C(d_light)[:, k]).all(), k
            assert (C(d_ray)[mask][:, k] == 0).all() and (C(d_light)[:, k] == 0).all(), k
            continue
        assert colref[k] > 0 and col[k] <= 3.0 * col32[k] + 1e-5 * colref[k], (k, col[k] / colref[k], col32[k] / colref[k])
    # the sums, from the kept rays only: the kernels' own (the others have a zero upstream gradient and add exact zeros), and
    # the per-ray output re-summed
    want = (ref["dlight_ray"] * m4).sum((1, 2))
    want32 = (ref32["dlight_ray"] * m4).sum((1, 2))
    bound(C(d_light), want, want32, "dlight")
    bound((C(d_ray) * m4).sum((1, 2)), want, want32, "dlight resummed")
    # ... and column by column. A column's sum is ONE number per view, and the f32 transliteration's error in it can cancel to
    # nothing by chance (1e-7 of the sum, where single rays are off by 1e-5 of it in both f32 programs): its own error is taken
    # before that cancellation, as the rays' absolute errors summed.
    l1 = (np.abs(ref32["dlight_ray"] - ref["dlight_ray"]) * m4).sum((1, 2)).max(0)
    bound(C(d_light), want, want32, "dlight by column", per_column=True, err32=l1, skip=zero)
    bound((C(d_ray) * m4).sum((1, 2)), want, want32, "dlight resummed by column", per_column=True, err32=l1, skip=zero)
    assert (C(d_ray)[~mask] == 0).all()
    return sc, st, dict(n=n.cpu().numpy(), steps=steps.cpu().numpy(), d_light=C(d_light))


def raw_bwd(vol, tf, cam, light, rays, S, sr, go, out, d_vol=None, d_tf=None, d_light=None, d_ray=None):
    """dr_march_lit_bwd on the caller's own output buffers (functional.march_lit_bwd allocates zeroed ones); d_vol and d_tf of
    inputs the views share."""
    F, N = functional(), native()
    cam, V, W, H, rargs = F._ray_args(vol, cam, *rays)
    dv = (None, 0, 0, 0, 0) if d_vol is None else (d_vol.data_ptr(), *d_vol.stride(), 0)
    rc = N.lib().dr_march_lit_bwd(*F._vol_args(vol, V), *F._tf_args(tf, V), *rargs, S, sr, light.data_ptr(), N.DR_MODE_DIFF,
                                  go.data_ptr(), out.data_ptr(), *dv, F._ptr(d_tf), 0, F._ptr(d_light), F._ptr(d_ray),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
