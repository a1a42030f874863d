"""Edges of the 2-D (value, gradient-magnitude) TF march (csrc/march_tf2d.hip) that tests/test_gpu_tf2d.py does
not reach: a table constant along u against the 1-D baseline kernels bit for bit (no transliteration involved) across every LDS
boundary, exact plateaus (flat samples, |grad| = 0) and values outside [0, 1], volume-only and TF-only backwards in every tier,
rows wider than a wave through the non-differentiable skip, and degenerate table shapes."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_tf2d as B  # noqa: E402  (the scene, table and comparison helpers)
import tf2d_reference as R2  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
C = lambda t: t.detach().double().cpu().numpy()  # noqa: E731


# --- 1. a table constant along u is the 1-D baseline, bit for bit ---------------------------------------------------------------

G_HUGE = 1e30


def _air_volume(shape, seed):
    """B._volume with exact-zero air outside a ball of radius 0.8 and wherever it falls below 0.3: every voxel is 0 or >= 0.3."""
    v = B._volume(shape, seed=seed)
    axes = [torch.linspace(-1.0, 1.0, s, device=DEV) for s in shape]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    air = (x * x + y * y + z * z > 0.64) | (v < 0.3)
    return torch.where(air, torch.zeros_like(v), v).contiguous()


# RV = 16: P = 16 RG puts both sides of the backward's tier boundaries (P 3392 | 3408, 10176 | 10192) and of the NONDIFF
# forward's LDS boundary (16 P + 4 RV bytes: RG 635 | 636) in one sweep; RG = 65 and 635 send rows wider than 64 texels
# through the NONDIFF skip's row maxima
@pytest.mark.parametrize("RG", [2, 7, 65, 212, 213, 635, 636, 637])
@pytest.mark.parametrize("jitter", [0, 977], ids=["nojit", "jit"])
@pytest.mark.parametrize("vdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_u_invariant_table_is_the_1d_baseline_bit_for_bit(hiplib, RG, jitter, vdt):
    """Every column of the table is the same 1-D TF of RV rows, and g_scale = 1e30. A non-flat sample then has
    u (RG - 1) >= 2^24, so fg = 0 exactly and it reads column RG - 1 (beyond 2^31 through the saturating float-to-int
    conversion of axis_index and its min(i0, R - 1) clamp); a flat sample (exact-zero air) reads column 0 with fg = 0. Either
    way rgba = mix(lo, lo, 0) = lo: the forward is march_fwd's bit for bit, d_vol is march_bwd's to atomic ordering (the u path
    adds exact zeros; on a flat sample only the !flat guard keeps 0 * inf out of it), and d_tf2d's columns 0 and RG - 1 sum to
    march_bwd's d_tf while the others stay exactly zero.
    The premise needs |grad| 1e30 (RG - 1) >= 2^24 on every non-flat sample: _air_volume has no voxel in (0, 0.3), so a
    non-flat tap difference is far above 1e-22. With a volume holding values in (0, 1e-10) this test would stop being bit-exact."""
    F, N = B._F(), B._N()
    vol = _air_volume((26, 24, 28), seed=21).to(vdt)
    cam = B._cams(2)
    sr, S, RV = 2.0, 4096, 16
    e, x, r, n = F.ray_setup(cam, (16, 16), vol.shape, sr, jitter_seed=jitter)
    for kind in ("opaque", "skip"):
        tf = B._tf1d(RV, kind, seed=22)
        tf2d = tf[:, None, :].expand(RV, RG, 4).contiguous()
        for mode in (N.DR_MODE_DIFF, N.DR_MODE_NONDIFF):
            ref, ref_steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, mode=mode, variant=N.DR_VARIANT_BASELINE,
                                         workspace=None, hints=0)
            out, steps = F.march_tf2d_fwd(vol, tf2d, cam, e, x, r, n, S, sr, G_HUGE, mode=mode)
            torch.cuda.synchronize()
            assert torch.equal(steps, ref_steps), (kind, mode)
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (kind, mode)
            assert (ref[..., 3] > 0).any()
        g = torch.randn((2, 16, 16, 4), device=DEV, generator=torch.Generator(device=DEV).manual_seed(23))
        out, _ = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0)
        dv0, dt0 = F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out, variant=N.DR_VARIANT_BASELINE, workspace=None)
        dv1, dt1 = F.march_tf2d_bwd(vol, tf2d, cam, e, x, r, n, S, sr, G_HUGE, g, out)
        assert torch.isfinite(dv1).all() and torch.isfinite(dt1).all(), kind
        assert (dv1 - dv0).abs().max() <= 1e-5 * dv0.abs().max(), kind
        assert (dt1[:, 1:RG - 1] == 0).all(), kind
        assert (dt1[:, 0] + dt1[:, RG - 1] - dt0).abs().max() <= 1e-5 * dt0.abs().max(), kind
        assert dt1[:, 0].abs().max() > 0 and dt1[:, RG - 1].abs().max() > 0, kind   # flat samples and the others both met


# --- 2. flat plateaus and values outside [0, 1], against the transliteration ---------------------------------------------------

def _plateau_table(RV, RG, seed):
    """Column 0 (where flat samples read) unlike the others in colour; a small alpha everywhere (air, row 0, and the plateau
    rows included) so that rays cross the whole object."""
    g = torch.Generator().manual_seed(seed)
    tf = torch.rand((RV, RG, 4), generator=g) * 0.5 + 0.05
    tf[..., 3] = 0.02 + 0.1 * torch.rand((RV, RG), generator=g)
    tf[:, 0, :3] = torch.tensor([0.95, 0.9, 0.9])
    tf[:, 0, 3] = 0.02
    return tf.contiguous().to(DEV)


@pytest.mark.parametrize("RV,RG", [(12, 7), (128, 80)], ids=["tier2", "tier0"])
def test_flat_plateaus_and_out_of_range_values(hiplib, RV, RG):
    """tf2d_reference.plateau_volume: exact-zero air, plateaus at 0.25 and 0.5 around a structured shell, and blocks at 2.0
    (I > 1: the value axis's high clamp) and -0.25 (I < 0: its low clamp). Powers of two, so that the samples inside them are flat
    in the f32 kernel and in the f64 transliteration alike (tests/test_tf2d.py checks that premise): u = 0, column 0, no normal,
    and the backward's !flat guard is all that keeps k = u_bar g_scale / |grad| = 0 * inf out of d_vol. DIFF forward + backward
    (in LDS tier 2, and in tier 0 where nothing is staged) and NONDIFF, against the transliteration."""
    vol = torch.from_numpy(R2.plateau_volume((24, 24, 24), seed=24)).to(DEV)
    tf = _plateau_table(RV, RG, seed=25)
    from differender_amd.tf2d import gradient_scale
    g_scale = gradient_scale(vol, q=0.99)
    cam = B._cams(2)
    ref, mask, host = B._compare(vol, tf, cam, (16, 16), 4096, 1.0, g_scale, count_flat=True)
    flat, steps = ref["flat"][mask], ref["steps"][mask]
    assert flat.sum() >= 0.3 * steps.sum() and (flat > 0).mean() > 0.9, (flat.sum(), steps.sum())
    assert ((flat > 0) & (flat < steps)).mean() > 0.3           # rays that meet flat samples and structure both
    dtf = ref["dtf"]
    assert np.abs(dtf[:, 0]).max() > 0 and np.abs(dtf[:, 1:]).max() > 0
    B._compare_nondiff(vol, tf, cam, (16, 16), 4.0, g_scale)


# --- 3. volume-only and TF-only backwards in every tier ------------------------------------------------------------------------

def _tf2d_linear_u(RV, RG, seed):
    """Rows linear along u (random ends, alpha rising with u). A table with a kink at every column puts a jump of its slope
    under each column boundary: with hundreds of columns, the f32 taps (~1e-4 relative in |grad|) put many samples on the other
    side of a boundary than f64 does, and d_vol's u path differs by whole slope jumps -- for both the kernel and the f32
    transliteration, at different samples. Linear rows keep the u slope continuous, so the comparison measures the kernel."""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.0, 1.0, RG)[None, :, None]
    a = torch.rand((RV, 1, 4), generator=g) * 0.9 + 0.05
    b = torch.rand((RV, 1, 4), generator=g) * 0.9 + 0.05
    tf = a + (b - a) * ramp
    tf[..., 3] = 0.05 + 0.9 * torch.rand((RV, 1), generator=g) * ramp[..., 0]
    return tf.contiguous().to(DEV)


@pytest.mark.parametrize("RG", [212, 213, 636, 637], ids=["P3392", "P3408", "P10176", "P10192"])
def test_partial_backwards_in_every_tier(hiplib, RG):
    """want_vol=False / want_tf=False at RV = 16 on both sides of both backward tier boundaries. A volume-only call keeps no
    gradient table, so at P <= 3392 it runs tier 1 where the full call runs tier 2; a TF-only call in tiers 1 and 0 is CellRun's
    float atomics with no volume scatter. Each against the transliteration and against the full call; what was not asked for is
    None. Then the same through Raycaster2D (needs_input_grad picks the call), and with a NaN upstream pixel."""
    from differender_amd.tf2d import Raycaster2D
    F = B._F()
    vol = B._volume((20, 20, 20), seed=26)
    tf = _tf2d_linear_u(16, RG, seed=27)
    cam, S, sr, g_scale = B._cams(1), 4096, 1.0, B._g_scale(vol)
    st = B._reference(vol, tf, cam, (16, 16), S, sr, g_scale)
    call = lambda **kw: F.march_tf2d_bwd(vol, tf, cam, *st["rays"], S, sr, g_scale, st["gm"], st["out"], **kw)  # noqa: E731
    dv, dt = call()
    dv_only, none_t = call(want_tf=False)
    none_v, dt_only = call(want_vol=False)
    assert none_t is None and none_v is None
    for got, k in ((dv, "dvol"), (dt, "dtf"), (dv_only, "dvol"), (dt_only, "dtf")):
        assert torch.isfinite(got).all(), k
        B._assert_close(C(got), st, k)
    assert (dv_only - dv).abs().max() <= 1e-5 * dv.abs().max()
    assert (dt_only - dt).abs().max() <= 1e-5 * dt.abs().max()

    D = H = W = 20
    vol_u = B._volume((D, H, W), seed=28)[None]
    tf_u = tf.permute(2, 0, 1).contiguous()
    lf = B._cams(1)[0]
    rc = Raycaster2D((D, H, W), (16, 16), (16, RG), g_scale, jitter=False, max_samples=S)
    G = torch.randn((4, 16, 16), device=DEV, generator=torch.Generator(device=DEV).manual_seed(29))

    def grads(wv, wt, w=G):
        v = vol_u.clone().requires_grad_(wv)
        t = tf_u.clone().requires_grad_(wt)
        (rc(v, t, lf) * w).sum().backward()
        return v.grad, t.grad

    gv, gt = grads(True, True)
    gv1, none_t = grads(True, False)
    none_v, gt1 = grads(False, True)
    assert none_t is None and none_v is None
    assert gv.abs().max() > 0 and gt.abs().max() > 0
    assert (gv1 - gv).abs().max() <= 1e-5 * gv.abs().max()
    assert (gt1 - gt).abs().max() <= 1e-5 * gt.abs().max()
    w = G.clone()
    w[0, 5, 7] = float("nan")
    nv, nt = grads(True, True, w)
    assert torch.isfinite(nv).all() and torch.isfinite(nt).all()
    assert float(nv.abs().max()) <= 1.5 * float(gv.abs().max())
    assert float(nt.abs().max()) <= 1.5 * float(gt.abs().max())


# --- 4. rows wider than a wave through the NONDIFF skip ------------------------------------------------------------------------

@pytest.mark.parametrize("RV,RG", [(12, 600), (16, 635), (16, 636)], ids=["wide", "lds_edge", "global_edge"])
def test_nondiff_wide_rows_against_the_f64_transliteration(hiplib, RV, RG):
    """test_nondiff_against_the_f64_transliteration with rows wider than the 64 lanes that build the skip's row maxima (each
    lane strides across its row). Rows 4m and 4m + 1 are dead (alpha 0 or below 1e-3); rows 4m + 2 and 4m + 3 are transparent
    in their first 64 columns and live only beyond, growing along u: a row maximum that looked at fewer texels would call them
    dead and skip samples it must composite. (16, 635) stages the table in LDS and skips; (16, 636) is one column past the
    NONDIFF forward's LDS budget (16 P + 4 RV bytes) and reads it where it lies."""
    vol = B._volume((20, 18, 22), seed=30)
    tf = B._tf2d(RV, RG, "opaque", seed=31)
    dead = torch.tensor([k % 4 in (0, 1) for k in range(RV)], device=DEV)
    level = torch.tensor([(0.0, 9.9e-4, 5e-4)[k % 3] for k in range(RV)], device=DEV)
    tf[..., 3] = torch.where(dead[:, None], level[:, None].expand(RV, RG), tf[..., 3])
    tf[dead, 0, 3] = 0.0
    tf[~dead, :64, 3] = 0.0
    tf = tf.contiguous()
    ref, mask = B._compare_nondiff(vol, tf, B._cams(2), (16, 14), 2.0, B._g_scale(vol))
    assert (ref["rgba"][mask][:, 3] > 0.05).mean() > 0.3   # the late-live columns are reached and composited


# --- 5. degenerate table shapes ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("RV,RG", [(1, 9), (16, 2), (1, 1)])
def test_degenerate_table_shapes(hiplib, RV, RG):
    """(1, RG): lv = 0, so the value axis carries no gradient and d_vol comes through u and the normal alone; (RV, 2): u
    interpolates between two columns; (1, 1): one texel. Against the transliteration; (1, 1) also against the 1-D R = 1
    baseline bit for bit."""
    F, N = B._F(), B._N()
    vol = B._volume((20, 18, 22), seed=32)
    tf = B._tf2d(RV, RG, "opaque", seed=33)
    cam, g_scale = B._cams(2), B._g_scale(vol)
    B._compare(vol, tf, cam, (16, 16), 4096, 1.0, g_scale)
    if (RV, RG) == (1, 1):
        tf1 = tf[:, 0, :].contiguous()
        e, x, r, n = F.ray_setup(cam, (16, 16), vol.shape, 1.0)
        for mode in (N.DR_MODE_DIFF, N.DR_MODE_NONDIFF):
            ref, ref_steps = F.march_fwd(vol, tf1, cam, e, x, r, n, 4096, 1.0, mode=mode, variant=N.DR_VARIANT_BASELINE,
                                         workspace=None, hints=0)
            out, steps = F.march_tf2d_fwd(vol, tf, cam, e, x, r, n, 4096, 1.0, g_scale, mode=mode)
            torch.cuda.synchronize()
            assert torch.equal(steps, ref_steps) and torch.equal(out.view(torch.int32), ref.view(torch.int32)), mode
        g = torch.randn((2, 16, 16, 4), device=DEV, generator=torch.Generator(device=DEV).manual_seed(34))
        out, _ = F.march_fwd(vol, tf1, cam, e, x, r, n, 4096, 1.0, variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0)
        dv0, dt0 = F.march_bwd(vol, tf1, cam, e, x, r, n, 4096, 1.0, g, out, variant=N.DR_VARIANT_BASELINE, workspace=None)
        dv1, dt1 = F.march_tf2d_bwd(vol, tf, cam, e, x, r, n, 4096, 1.0, g_scale, g, out)
        assert (dv1 - dv0).abs().max() <= 1e-5 * dv0.abs().max()
        assert (dt1[:, 0] - dt0).abs().max() <= 1e-5 * dt0.abs().max()
