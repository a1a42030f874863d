"""The NARROW brick kernels (volume edges up to 991) read "this +-delta tap sits in the centre tap's cell" from the fractions --
fr+ >= fr, fr- <= fr (csrc/dr_brick_common.h, "tap-cell flags"; the host proof is tests/test_tapflag_proof.py) -- in the shared-lerp
taps of F1 and B1, in the adjoint lines of B1's d_volume scatter and behind its row transposition, whose packed word now carries the
centre cell and the validity only. The wide-tap kernels (edges 992 .. 2000) keep the integer cells. The scenes are the smallest at
which a flag can go wrong: one brick, one cell into a second brick, two bricks; rays that enter through each of the six faces at a grazing angle, where a tap
clamps alone, and rays that leave through it, whose last sample clamps together with its tap; the last NARROW edge and the first wide one; and, for the d_tf run sums that B1 computes beside the
scatter, passes of one run of 64 lanes, of runs of one lane, and of runs of 2, 3, 5, 9, 17 and 33 lanes (every step of the
segmented scan needed by some lanes, runs across the 16- and 32-lane boundaries), at R = 256 and R = 2.

Every comparison is DESIGN.md D8's rule of tests/test_gpu_bwd_row_scatter.py on the GPU's own ray buffers, against the C oracle in
float64: err <= 3 err32 + 1e-5 scale, for the image, the sample counts, d_volume and d_tf."""
import numpy as np
import pytest

from test_gpu_bwd_row_scatter import BIG, Scene, T, check, randn_g, rule, Fn  # noqa: F401  (Fn: the module's fixture)
from test_gpu_bwd_dtf_rows import colour_tf, noise_volume

pytestmark = pytest.mark.gpu

DELTA = 1e-3   # the normal taps' offset in world units (VR.py:193)


def d8(got, ref64, ref32, what):
    """The rule's inequality alone (image, sample counts)."""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    scale = float(np.abs(ref64).max())
    err, err32 = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    print("flags %s err/scale %.3g err32/scale %.3g scale %.3g" % (what, err / max(scale, 1e-300), err32 / max(scale, 1e-300), scale))
    assert np.isfinite(got).all() and scale > 0.0, what
    assert err <= 3.0 * err32 + 1e-5 * scale, (what, err / scale, err32 / scale)


def check_all(O, sc, what, **kw):
    """check() of the row-scatter tests (d_volume, d_tf, records found, brick kernels did the work) + image and sample counts."""
    res = check(O, sc, what, **kw)
    _, steps = sc.Fn.march_fwd(sc.vol, sc.tf, sc.cam, *sc.rays, sc.S, sc.sr, workspace=res["ws"])
    out = res["out"].cpu().numpy()
    steps = steps.cpu().numpy()
    eh, xh, rh, nh = sc.rays_h
    for v in range(sc.V):
        ref = [O.march_fwd(sc.vol_o.astype(f), sc.tf_of(v).astype(f), sc.cams_h[v].astype(f), eh[v].astype(f), xh[v].astype(f),
                           rh[v].astype(f), nh[v], sc.S, sc.sr, 0) for f in (np.float64, np.float32)]
        d8(out[v], ref[0][0], ref[1][0], what + " image")
        d8(steps[v], ref[0][1], ref[1][1], what + " sample counts")
    return res


# ---- A. one brick, one cell into a second, two bricks ------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [13, 14, 25])
def test_one_and_two_bricks(oracle, Fn, N):
    """12 cells fill one brick; 13 put one cell into a second brick along every axis (its box is mostly the clamped edge); 24 fill
    two. A 36 x 32 image: 1152 candidate pixels per brick, more than the main launch takes, so the work-item kernels run too."""
    sc = Scene(Fn, oracle.synth_volume(N), colour_tf(oracle, 64), oracle.in_circles(0.3), (36, 32), 1.0, BIG)
    res = check_all(oracle, sc, "A N=%d" % N)
    print("flags A N=%d work items %d" % (N, int(res["st_f"][5])))
    if N == 13:
        assert int(res["st_f"][5]) > 0   # the one brick's rectangle is the whole volume's: beyond 1024 candidates


# ---- B. rays that enter through a face at a grazing angle, rays that leave through it -----------------------------------------------

def _fma(a, b, c):
    """fmaf on float32 operands: the product is exact in double, the sum rounded to double and then to float."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def clamped_taps(sc, v, axis, sign):
    """View v's samples as the brick kernels place them (sample_pos_rcp and axis_coord of csrc/, operation for operation, from the
    GPU's ray buffers): how many have their outward tap beyond the face `sign` of `axis` while the centre is inside (the tap alone
    clamps), and how many have the centre's a = fma(0.5, p, 0.5) at the clamp value too -- 1 on the + side (from p = 1 - 2^-25 on it
    rounds there), 0 on the - side (p <= -1) -- so that centre and tap share one q: fr+ == fr, fr- == fr."""
    f32 = np.float32
    e, x, r, n = (a[v] for a in sc.rays_h)
    cam = sc.cams_h[v]
    alone = both = 0
    for i, j in np.argwhere(n >= 2):
        nn = int(n[i, j])
        t0 = f32(e[i, j] + f32(0.5) * (x[i, j] - e[i, j]) / f32(nn))
        q = np.arange(nn, dtype=f32) / f32(nn - 1)     # (the kernels' reciprocal sequence IS the correctly rounded quotient)
        t = _fma(x[i, j], q, t0 * (f32(1.0) - q))      # mixf(t0, exit, q): the last sample sits at t = exit exactly
        pos = _fma(t, r[i, j, axis], cam[axis])
        a0 = _fma(f32(0.5), pos, f32(0.5))
        ap = _fma(f32(0.5), pos + f32(sign * DELTA), f32(0.5))
        tap_c, centre_c = ((ap >= 1.0), (a0 >= 1.0)) if sign > 0 else ((ap <= 0.0), (a0 <= 0.0))
        alone += int((tap_c & ~centre_c).sum())
        both += int((tap_c & centre_c).sum())
    return alone, both


FACES = [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]


@pytest.mark.parametrize("axis,sign", FACES, ids=["+x", "-x", "+y", "-y", "+z", "-z"])
def test_rays_through_a_face(oracle, Fn, axis, sign):
    """Two views of a 25^3 volume per face (its cells lie in the second brick on the + side, in the first on the - side).
    View 0 ENTERS through it at a grazing angle: the camera stands 0.3 outside the face's plane, six units away, and the rays of
    one column (row, for y) meet the face at a slope of ~0.05, so at sampling rate 4 their first samples lie within delta of it --
    the outward tap clamps, the centre does not (fr+ of the clamped q against a fraction of the last cell; fr- = 0 against one of
    the first).
    View 1 LEAVES through it: the camera stands six units out on the other side. A ray's last sample sits at t = exit, its
    coordinate on the exit face's axis within an ulp of +-1: for a good share of the rays it clamps, or rounds to the clamped q,
    TOGETHER with its outward tap -- fr+ == fr, fr- == fr, the equalities at which >= and <= differ from strict compares.
    Both counts come from the host's restatement of the sample positions on the GPU's ray buffers, and both are asserted."""
    graze = np.zeros(3, np.float32)
    graze[axis] = sign * 1.3
    graze[2 if axis != 2 else 0] = 6.0
    leave = np.array((0.8, 0.5, 0.6), np.float32)
    leave[axis] = -sign * 6.0
    sc = Scene(Fn, oracle.synth_volume(25), colour_tf(oracle, 64), np.stack([graze, leave]), (36, 32), 4.0, BIG)
    face = ("+" if sign > 0 else "-") + "xyz"[axis]
    alone0, both0 = clamped_taps(sc, 0, axis, sign)
    alone1, both1 = clamped_taps(sc, 1, axis, sign)
    print("flags B face %s: rays %d; entering view: tap alone clamps %d, with the centre %d; leaving view: %d, %d" % (face, sc.hit, alone0, both0, alone1, both1))
    assert alone0 >= 8, (face, alone0)
    assert both1 >= 8, (face, both1)
    check_all(oracle, sc, "B face " + face)


# ---- C. the last NARROW edge and the first wide one --------------------------------------------------------------------------------

@pytest.mark.parametrize("NX", [991, 992])
def test_last_narrow_and_first_wide_edge(oracle, Fn, NX):
    """(991, 20, 16): delta = 0.495 voxel along x, the NARROW kernels with the flags from the fractions; (992, 20, 16): 0.4955, the
    wide-tap kernels with the integer cells (taps_narrow, csrc/march_flat.hip). The same field and camera for both."""
    vshape = (NX, 20, 16)
    i, j, k = (np.arange(v, dtype=np.float64) for v in vshape)
    vol = (0.5 + 0.45 * np.sin(0.05 * i)[:, None, None] * np.cos(0.3 * j)[None, :, None] * np.sin(0.5 + 0.3 * k)[None, None, :])
    sc = Scene(Fn, vol.astype(np.float32), colour_tf(oracle, 256), np.array((0.4, 0.3, 2.4), np.float32), (24, 20), 1.0, BIG)
    assert int(sc.rays_h[3].max()) > 900
    check_all(oracle, sc, "C NX=%d" % NX)


# ---- D. the d_tf run sums beside the scatter: run lengths ---------------------------------------------------------------------------

def z_ramp_volume(run, per_voxel, R=256, NZ=26):
    """Constant in x and y, linear along z; seen along z by rays that place `per_voxel` samples in a voxel, consecutive samples
    are 1 / (run (R - 1)) apart in intensity: `run` samples between the same two texels."""
    prof = 0.03 + np.arange(NZ, dtype=np.float64) * per_voxel / (run * (R - 1.0))
    assert prof.max() < 0.97, prof.max()
    return np.broadcast_to(prof[None, None, :], (8, 8, NZ)).astype(np.float32).copy()


@pytest.mark.parametrize("R", [256, 2])
@pytest.mark.parametrize("name", ["constant", "noise"])
def test_one_run_of_64_and_runs_of_one(oracle, Fn, name, R):
    """constant: the samples of a segment share one texel, a full pass is one run of 64 lanes and needs every step of the segmented
    scan. noise: neighbouring samples are ~50 texels apart, runs of one lane, no step moves anything. R = 2: one cell for all."""
    vol = np.full((26, 26, 26), 0.5, np.float32) if name == "constant" else noise_volume(26, seed=3)
    sc = Scene(Fn, vol, colour_tf(oracle, R), oracle.in_circles(0.3), (12, 12), 2.0, BIG)
    check_all(oracle, sc, "D %s R=%d" % (name, R))


@pytest.mark.parametrize("run", [2, 3, 5, 9, 17, 33])
def test_runs_of_a_few_lanes(oracle, Fn, run):
    """Four rays along z through a ramp whose slope puts `run` consecutive samples between the same two texels: step k of the scan
    is needed by the lanes 2^k and more into their run and by no others, and runs of 3, 5, 9, 17 and 33 lanes start at every
    offset within a 16-lane row, so some straddle lanes 15 | 16 and 31 | 32 (the two row-broadcast steps).
    At R = 256 only: a table of two texels has one texel pair, every sample of a segment falls between the same two and no slope
    can cut a segment into runs -- R = 2 is the constant and the noise scene above, where it means "one run per segment"."""
    cam, NZ = np.array((0.0, 0.0, 2.5), np.float32), 26
    # samples per voxel along the central ray, from the GPU's ray buffers (they depend on the volume's shape alone)
    e, x, r, n = (a[0] for a in Scene(Fn, np.zeros((8, 8, NZ), np.float32), colour_tf(oracle, 256), cam, (2, 2), 8.0, BIG).rays_h)
    nn = int(n[0, 0])
    dt = float(x[0, 0] - e[0, 0]) * (1.0 - 0.5 / nn) / (nn - 1)   # the samples run from entry + half a planned step to the exit
    per_voxel = 1.0 / (dt * abs(float(r[0, 0, 2])) * 0.5 * (NZ - 1 - 1e-4))
    vol = z_ramp_volume(run, per_voxel)
    sc = Scene(Fn, vol, colour_tf(oracle, 256), cam, (2, 2), 8.0, BIG)
    # the ramp as the rays see it: texel run lengths along the central ray
    t0 = e[0, 0] + 0.5 * (x[0, 0] - e[0, 0]) / nn
    z = 2.5 + (t0 + (x[0, 0] - t0) * np.arange(nn) / (nn - 1)) * r[0, 0, 2]
    q = np.clip(0.5 * z + 0.5, 0, 1) * (NZ - 1 - 1e-4)
    I = np.interp(q, np.arange(NZ), vol[0, 0].astype(np.float64))
    lo = np.floor(I * 255).astype(int)
    runs = np.diff(np.flatnonzero(np.diff(lo) != 0))
    print("flags D run=%d samples %d (%.2f per voxel), texel runs along the central ray: median %g (min %d max %d)" % (
        run, nn, per_voxel, np.median(runs), runs.min(), runs.max()))
    assert abs(np.median(runs) - run) <= max(1, run // 8), (run, np.median(runs))
    check_all(oracle, sc, "D run=%d" % run, g=randn_g(1, (2, 2), seed=run))
