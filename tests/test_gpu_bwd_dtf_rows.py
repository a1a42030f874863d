"""The d_tf adds of the brick backward's main kernel (B1, csrc/march_flat.hip). Every pass sums each run of samples between the
same two texels across lanes and adds from the run's last lane into a [texel][4] LDS table. The other build these cases were
written for is a closed experiment (DR_BWD_DTF_ROWS and DR_BWD_DTF_DIRECT_MIN of tools/patches/closed_experiments.patch; measured
slower, profiles/dtfrows_ab.txt, tools/README.md): there a 64-sample pass that holds at least DR_BWD_DTF_DIRECT_MIN runs moves
each sample's d_tf inputs to lane 16 r + c <- 4 c + r and every lane adds its own eight products into a component-major table
(dtf_rows_add), a pass of fewer, longer runs keeps the run sums. The cases hold for either build, and passed with both. They
are the smallest scenes that send passes down either way and through the edges of the exchange: runs of one sample, monotone
runs of two, one texel from samples far apart, one run per segment, pass run counts right at the threshold, the smallest and
the largest tables, many segments per pass, ragged last passes, poisoned upstream gradients, views, storage, the work-item
kernel and the wide-tap kernels.

Every comparison is DESIGN.md D8's rule of tests/test_gpu_bwd_row_scatter.py (`rule`): on the GPU's own ray buffers, against the
C oracle in float64, err <= 3 err32 + 1e-5 scale, for d_tf and d_volume; the backward found its forward's records
(workspace_stats[9] == 0) and the per-ray fallback took at most a tenth of the rays."""
import numpy as np
import pytest

from test_gpu_bwd_row_scatter import BIG, Scene, T, check, randn_g, rule, Fn  # noqa: F401  (Fn: the module's fixture)

pytestmark = pytest.mark.gpu

DIRECT_MIN = 8   # DR_BWD_DTF_DIRECT_MIN of the patched build (tools/patches/closed_experiments.patch); the shipped kernel has no threshold
BRK = 12         # cells per brick edge (csrc/dr_brick.h)
R256 = 256


def colour_tf(O, R, lo=0.004, hi=0.05, alpha0=None):
    """bench_tf's sinusoidal colours under an alpha ramp (both alpha and its slope are non-zero: d_tf has every term)."""
    tf = O.bench_tf(R, 0.02)
    tf[:, 3] = np.linspace(lo, hi, R)
    if alpha0 is not None:
        tf[0, 3] = alpha0
    return tf


def axes(N):
    return np.meshgrid(*(np.linspace(-1.0, 1.0, n) for n in N), indexing="ij", sparse=True)


def noise_volume(N, seed=11):
    """White noise in [0.1, 0.9]: neighbouring samples of a ray are ~50 texels of 256 apart -- every run has length 1."""
    return np.random.default_rng(seed).uniform(0.1, 0.9, size=(N, N, N)).astype(np.float32)


def ramp_volume(N):
    """Linear along the diagonal: an orbit camera's ray (direction sum ~1.5) climbs ~0.5 texel of 256 per voxel, in monotone
    runs of about two samples at sampling rate 1. Around 0.07, not 0.5: the normal of so flat a ramp is a difference of nearly
    equal voxels, and float32 keeps four more bits of it there (99.8 % of the voxels agree between the two oracles, 98.4 % at 0.45)."""
    X, Y, Z = axes((N, N, N))
    c = (0.5 / 255.0) * (N - 1) / (2.0 * 1.5)
    return (0.07 + c * (X + Y + Z) + 0.0 * X * Y * Z).astype(np.float32)


def blob_volume(N):
    """One gaussian blob: a ray climbs and descends, so a pass holds the same texel from samples far apart."""
    X, Y, Z = axes((N, N, N))
    return (0.2 + 0.12 * np.exp(-(X * X + Y * Y + Z * Z) / 0.5)).astype(np.float32)


def ball_in_air(N):
    """0 outside a ball of 0.6 (one voxel of smooth edge): the air is one run per segment at texel 0."""
    X, Y, Z = axes((N, N, N))
    r = np.sqrt(X * X + Y * Y + Z * Z)
    return (0.6 * np.clip((0.62 - r) * (N / 2.0), 0.0, 1.0)).astype(np.float32)


# ---- A. run lengths ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["noise", "ramp", "blob"])
def test_short_runs(oracle, Fn, name):
    """noise: every run has length 1, every pass adds directly. ramp: monotone runs of ~2. blob: a texel meets samples that are far
    apart in the pass, in the same and in different 16-lane rows after the transposition. 30^3 = 3^3 bricks under a 16^2 image."""
    vol = dict(noise=noise_volume, ramp=ramp_volume, blob=blob_volume)[name](30)
    sc = Scene(Fn, vol, colour_tf(oracle, R256), oracle.in_circles(0.3), (16, 16), 1.0, BIG)
    check(oracle, sc, "dtf A " + name)


@pytest.mark.parametrize("name", ["constant", "ball"])
def test_one_run_per_segment_keeps_the_run_sums(oracle, Fn, name):
    """A constant volume, and a ball in air under a TF whose alpha is 0 at texel 0: the samples of a segment share one texel (all
    of them / those in the air), a pass holds a handful of runs and takes the run-sum path; texel 0 collects every air sample."""
    if name == "constant":
        vol, tf = np.full((26, 26, 26), 0.5, np.float32), colour_tf(oracle, R256)
    else:
        vol, tf = ball_in_air(30), colour_tf(oracle, R256, alpha0=0.0)
    sc = Scene(Fn, vol, tf, oracle.in_circles(0.3), (12, 12), 2.0, BIG)
    res = check(oracle, sc, "dtf B " + name)
    if name == "ball":
        assert np.abs(res["dt"][0]).max() > 0.0   # the air's samples reached texel 0 (their opacity is 0, its adjoint is not: d alpha[0])


# ---- B. pass run counts at the threshold -------------------------------------------------------------------------------------------

def sweep_volume(NZ):
    """Constant in x and y; along z the slope grows from 1.3 to 2.5 texels of 256 per voxel. Seen along z at sampling rate 8 (16
    samples per voxel of this shape, a 64-sample pass spans 4 voxels) the number of texel runs in a pass sweeps from 6 to 11."""
    z = np.arange(NZ, dtype=np.float64)
    prof = 0.1 + (1.3 * z + 1.2 * z * z / (2 * NZ)) / 255.0
    assert prof.max() < 0.95
    return np.broadcast_to(prof[None, None, :], (8, 8, NZ)).astype(np.float32).copy()


def pass_run_counts(O, vol, cam, WH, sr, R):
    """Host model of B1's passes for an image of few rays (one wave holds every segment of a brick, in pixel order): the samples
    of each ray from the oracle's ray buffers (sample_pos, tri_cell, sample_classify of oracle/dr_oracle_impl.inc, float64), cut
    into per-brick segments, concatenated per brick and cut into passes of 64; a run ends where the texel or the ray changes.
    -> the run counts of the FULL passes."""
    e, x, rays, n = O.ray_setup(cam.astype(np.float64), WH[0], WH[1], vol.shape, sr, dtype=np.float64)
    sc = np.array(vol.shape, np.float64) - 1.0 - 1e-4
    per_brick = {}
    for i in range(WH[0]):
        for j in range(WH[1]):
            nn = int(n[i, j])
            if nn < 2:
                continue
            s = np.arange(nn, dtype=np.float64)
            tmin = e[i, j] + 0.5 * (x[i, j] - e[i, j]) / nn
            t = tmin + (x[i, j] - tmin) * (s / (nn - 1))
            pos = cam.astype(np.float64)[None, :] + t[:, None] * rays[i, j][None, :]
            p = np.clip(0.5 * pos + 0.5, 0.0, 1.0) * sc[None, :]
            c0 = np.minimum(np.floor(p).astype(int), np.array(vol.shape) - 1)
            f = p - np.floor(p)
            c1 = np.minimum(c0 + 1, np.array(vol.shape) - 1)
            v = vol.astype(np.float64)
            I = 0.0
            for dx in (0, 1):
                for dy in (0, 1):
                    for dz in (0, 1):
                        w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                        I = I + w * v[(c1 if dx else c0)[:, 0], (c1 if dy else c0)[:, 1], (c1 if dz else c0)[:, 2]]
            lo = np.minimum(np.floor(I * (R - 1)).astype(int), R - 1)
            brick = [tuple(b) for b in (c0 // BRK)]
            for k in range(nn):
                per_brick.setdefault(brick[k], []).append((i * WH[1] + j, int(lo[k])))
    counts = []
    for samples in per_brick.values():
        for p0 in range(0, len(samples) - 63, 64):
            chunk = samples[p0:p0 + 64]
            counts.append(1 + sum(1 for a, b in zip(chunk[:-1], chunk[1:]) if a != b))
    return counts


def test_pass_run_counts_around_the_threshold(oracle, Fn):
    """One ray along the axis of a 1-D volume whose texel staircase narrows along the ray (sweep_volume), at sampling rate 8: a
    brick holds ~190 samples of the ray -- three full passes and a ragged one -- and the passes' run counts sweep across
    DR_BWD_DTF_DIRECT_MIN: the host model finds full passes of exactly one run fewer (run sums), exactly as many and one more
    (direct adds), so both ways and the switch between them feed one table within one workgroup."""
    vol = sweep_volume(72)
    cam = np.array((0.0, 0.0, 2.5), np.float32)
    counts = pass_run_counts(oracle, vol, cam, (1, 1), 8.0, R256)
    print("dtf C run counts of the full passes:", sorted(counts))
    for want in (DIRECT_MIN - 1, DIRECT_MIN, DIRECT_MIN + 1):
        assert want in counts, (want, sorted(counts))
    sc = Scene(Fn, vol, colour_tf(oracle, R256), cam, (1, 1), 8.0, BIG)
    check(oracle, sc, "dtf C sweep", g=randn_g(1, (1, 1), seed=4))


# ---- C. table sizes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2, 3, 2030])
def test_smallest_and_largest_tables(oracle, Fn, R):
    """R = 1: hi == lo == 0, the two adds of a lane meet in every component. R = 2, 3: every sample of the image shares one or
    two cells. R = 2030: the largest table the fast path serves (texel indices need all 11 bits of the packed word; the
    component-major rows are 16 240 B apart); there the smooth synth_volume, whose neighbouring samples are ~60 texels apart --
    runs of one sample, as the noise below it -- because a table that sparse holds one or two samples per entry, and the few
    noise samples whose lighting switches in float32 would be a tenth of its entries."""
    vol = oracle.synth_volume(26) if R > 3 else noise_volume(26, seed=R)
    sc = Scene(Fn, vol, colour_tf(oracle, R), oracle.in_circles(0.3), (12, 12), 1.0, BIG)
    res = check(oracle, sc, "dtf D R=%d" % R)
    assert res["dt"].shape == (R, 4)


# ---- D. segments and passes --------------------------------------------------------------------------------------------------------

def test_many_short_segments_of_different_rays_per_pass(oracle, Fn):
    """A 40^3 volume (4^3 bricks, the outer ones thin) under an 8 x 8 image: a brick has a handful of candidate rays with 3-13
    samples each, all in one wave's single pass -- a transposed lane carries another ray's upstream gradient, and most lanes of
    the pass hold nothing. (synth_volume: neighbouring samples are ~5 texels apart, runs of one sample.)"""
    sc = Scene(Fn, oracle.synth_volume(40), colour_tf(oracle, R256), oracle.in_circles(0.3), (8, 8), 1.0, BIG)
    check(oracle, sc, "dtf E short segments")


@pytest.mark.parametrize("S", [65, 100])
def test_ragged_last_pass(oracle, Fn, S):
    """Rays cut at max_samples = S at sampling rate 16 in a 26^3 volume: a full pass, then one of 1 / 36 samples whose
    transposed lanes read source lanes past the end of the wave's samples."""
    sc = Scene(Fn, ramp_volume(26), colour_tf(oracle, R256), oracle.in_circles(0.3), (8, 8), 16.0, S)
    check(oracle, sc, "dtf F S=%d" % S)


# ---- E. poisoned upstream gradients ------------------------------------------------------------------------------------------------

def test_nan_channel_and_absurd_value_in_grad_out(oracle, Fn):
    """One pixel with a NaN channel, one with 1e35 in a channel: both gradients stay finite (NaN products dropped, absurd ones
    clamped, per receiving lane), and every voxel the two rays do not reach is what the call computes without the two pixels."""
    sc = Scene(Fn, noise_volume(30), colour_tf(oracle, R256), oracle.in_circles(0.3), (16, 16), 1.0, BIG)
    n_h = sc.rays_h[3][0]
    px = np.argwhere(n_h > 20)[[30, 120]]
    g = randn_g(1, sc.WH)
    ok, bad = g.copy(), g.copy()
    mask = np.zeros(sc.WH, bool)
    for p in px:
        ok[0, p[0], p[1]] = 0.0
        mask[p[0], p[1]] = True
    bad[0, px[0][0], px[0][1], 1] = np.nan
    bad[0, px[1][0], px[1][1], 2] = 1e35
    res = check(oracle, sc, "dtf G without the two pixels", g=ok)
    dv_bad, dt_bad = sc.backward(res["ws"], res["out"], bad)
    assert np.isfinite(dv_bad).all() and np.isfinite(dt_bad).all()
    eh, xh, rh, nh = sc.rays_h
    reached = np.zeros(sc.vshape, bool)
    for seed in (0, 1):
        gp = np.zeros((*sc.WH, 4), np.float64)
        gp[mask] = np.random.default_rng(seed).uniform(0.5, 1.5, size=(int(mask.sum()), 4))
        a, _ = oracle.march_bwd(sc.vol_o.astype(np.float64), sc.tf_h.astype(np.float64), sc.cams_h[0].astype(np.float64), eh[0].astype(np.float64),
                                xh[0].astype(np.float64), rh[0].astype(np.float64), nh[0], sc.S, sc.sr, gp)
        reached |= a != 0
    scale = float(np.abs(res["dv64"]).max())
    d = float(np.abs(dv_bad - res["dv"])[~reached].max())
    print("dtf G reached voxels %d of %d, elsewhere max diff / scale %.3g" % (reached.sum(), reached.size, d / scale))
    assert 0 < reached.sum() < 0.3 * reached.size
    assert d <= 1e-5 * scale, d / scale


# ---- F. views, storage, kernels ----------------------------------------------------------------------------------------------------

def test_two_views_with_a_tf_each(oracle, Fn):
    tf = colour_tf(oracle, R256)
    tfs = np.stack([tf, np.clip(tf[::-1] * 0.8, 0, 1)]).astype(np.float32)
    cams = np.stack([oracle.in_circles(0.3), oracle.in_circles(2.2)])
    sc = Scene(Fn, noise_volume(26), tfs, cams, (12, 10), 1.0, BIG)
    res = check(oracle, sc, "dtf H two views", g=randn_g(2, (12, 10)))
    assert res["dt"].shape == (2, R256, 4)


def test_f16_storage(oracle, Fn):
    sc = Scene(Fn, ramp_volume(30), colour_tf(oracle, R256), oracle.in_circles(0.3), (16, 16), 1.0, BIG, f16=True)
    check(oracle, sc, "dtf I f16")


def test_camera_inside_the_volume(oracle, Fn):
    """The bricks around the eye become overflow work items: brick_flat_items_kernel, which keeps the [texel][4] table and the run
    sums (csrc/march_flat.hip: DTF_CM), beside the main kernel's component-major one -- both flush into one d_tf. The one case
    with more than 24^2 pixels: a brick is cut into items from 1024 candidate pixels on, and the eye's brick has them all."""
    sc = Scene(Fn, oracle.synth_volume(40), colour_tf(oracle, R256), np.array((0.2, 0.1, 0.3), np.float32), (36, 32), 1.0, BIG)
    res = check(oracle, sc, "dtf J inside")
    assert int(res["st_f"][5]) > 0   # work items existed


def test_wide_taps(oracle, Fn):
    """An axis longer than 991 voxels: the NARROW = false kernels (scatter_sample keeps its "both outside planes" tests there)."""
    vshape = (1100, 20, 16)
    i, j, k = (np.arange(v, dtype=np.float64) for v in vshape)
    vol = (0.5 + 0.45 * np.sin(0.05 * i)[:, None, None] * np.cos(0.3 * j)[None, :, None] * np.sin(0.5 + 0.3 * k)[None, None, :])
    sc = Scene(Fn, vol.astype(np.float32), colour_tf(oracle, R256), np.array((0.4, 0.3, 2.4), np.float32), (24, 20), 1.0, BIG)
    assert int(sc.rays_h[3].max()) > 1000
    check(oracle, sc, "dtf K long-x")


# ---- G. the other backwards of the same forward ------------------------------------------------------------------------------------

def test_against_the_tf_only_backward_and_a_second_call(oracle, Fn):
    """On ONE forward: B1's d_tf, the brick-centric TF-only backward's (want_vol=False, no tape: its own kernel, [texel][4] table,
    run sums at two samples per lane) and B1's again -- each under the rule against the float64 oracle; a second call finds
    zeroed tables and the same records."""
    sc = Scene(Fn, oracle.synth_volume(30), colour_tf(oracle, R256), oracle.in_circles(0.3), (16, 16), 1.0, BIG)
    res = check(oracle, sc, "dtf L first call", key="g2")
    (dv64, dt64), (dv32, dt32) = sc.refs(oracle, res["g"], "g2")
    _, dt_only = sc.Fn.march_bwd(sc.vol, sc.tf, sc.cam, *sc.rays, sc.S, sc.sr, T(res["g"]), res["out"], want_vol=False, want_tf=True,
                                 workspace=res["ws"])
    assert int(sc.Fn.workspace_stats(res["ws"])[9]) == 0
    rule(dt_only.cpu().numpy(), dt64, dt32, "dtf L TF-only d_tf")
    print("dtf L max |B1 - TF-only| / scale %.3g" % (np.abs(dt_only.cpu().numpy() - res["dt"]).max() / np.abs(dt64).max()))
    dv2, dt2 = sc.backward(res["ws"], res["out"], res["g"])
    assert int(sc.Fn.workspace_stats(res["ws"])[9]) == 0
    rule(dv2, dv64, dv32, "dtf L second call d_volume")
    rule(dt2, dt64, dt32, "dtf L second call d_tf")
