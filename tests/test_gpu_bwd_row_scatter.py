"""The d_volume scatter of the brick backward (B1, csrc/march_flat.hip: scatter_sample_rows) from the row-transposed lane layout:
the pass runs in lane order up to the adjoint, then lane 16 r + c scatters the sample that lane 4 c + r computed, its inputs moved
through ds_bpermute_b32 (DR_BWD_ROW_SCATTER, csrc/dr_tuning.h). Every case is the smallest shape at which that exchange can go
wrong: passes with one or two live lanes, a full pass, a ragged last pass whose source lanes lie past the end of the wave's
samples, passes that hold several segments (a transposed lane takes the sample of another ray), both accumulator formats, the
over-limit samples that bypass the box in lane order, the work items of heavy bricks, the wide-tap kernels, f16 storage and the
d_volume-only backward.

Every comparison is DESIGN.md D8's: on the GPU's own ray buffers, the C oracle in float64 is the reference and the same oracle in
float32 says what float32 arithmetic costs on this scene,

    err = max |got - ref64|,  err32 = max |ref32 - ref64|,  scale = max |ref64|:   err <= 3 err32 + 1e-5 scale

for d_volume and, where wanted, d_tf. Besides: the backward found its forward's records (workspace_stats[9] == 0) and the brick
kernels did the work -- the rays of the per-ray fallback (workspace_stats[2]) are at most a tenth of the rays that have samples --
unless a case says why not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 1 << 20


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def Fn(hiplib):
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from differender_amd import functional
    return functional


def rule(got, ref64, ref32, what):
    """D8 against the float64 oracle -> (err / scale, err32 / scale)."""
    got = np.asarray(got, np.float64)
    scale = float(np.abs(ref64).max())
    err = float(np.abs(got - ref64).max())
    err32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    print("rows %s err/scale %.3g err32/scale %.3g scale %.3g" % (what, err / max(scale, 1e-300), err32 / max(scale, 1e-300), scale))
    assert np.isfinite(got).all(), what
    assert np.isfinite(ref64).all() and scale > 0.0, what   # (a scene without a defined gradient tests nothing)
    assert err <= 3.0 * err32 + 1e-5 * scale, (what, err / scale, err32 / scale)
    # On the ordinary scenes err32 is the work of a few dozen voxels: a sample within rounding distance of a kink of the lighting
    # model takes the other branch in float32, and the voxels around it are off by percents of the scale -- a bound
    # under which one lost sample of a pass would pass too. The kernels re-shade such samples so that their switches fall as the
    # float32 oracle's, so the same rule is asked again of the voxels on which the two oracles agree to 1e-4 of the scale
    # (more than 99 % of them on every scene here), with err32 taken over those.
    good = np.abs(ref32.astype(np.float64) - ref64) <= 1e-4 * scale
    errg = float(np.abs(got - ref64)[good].max())
    err32g = float(np.abs(ref32.astype(np.float64) - ref64)[good].max())
    print("rows %s where float32 is good (%d of %d): err/scale %.3g err32/scale %.3g" % (what, good.sum(), good.size, errg / scale, err32g / scale))
    assert good.mean() > 0.99, what
    assert errg <= 3.0 * err32g + 1e-5 * scale, (what, errg / scale, err32g / scale)
    return err / scale, err32 / scale


class Scene:
    """Inputs on host and device, and the GPU's own ray buffers of one whole image per view."""

    def __init__(self, Fn, vol_h, tf_h, cams, WH, sr, S, f16=False):
        self.Fn, self.WH, self.sr, self.S = Fn, WH, float(sr), int(S)
        self.cams_h = np.atleast_2d(np.asarray(cams, np.float32))
        self.V = len(self.cams_h)
        self.tf_h = np.ascontiguousarray(tf_h, np.float32)
        self.R = self.tf_h.shape[-2]
        self.vshape = vol_h.shape
        if f16:
            self.vol, self.vol_o = T(vol_h.astype(np.float16)), vol_h.astype(np.float16).astype(np.float32)
        else:
            self.vol, self.vol_o = T(vol_h.astype(np.float32)), vol_h.astype(np.float32)
        self.tf, self.cam = T(self.tf_h), T(self.cams_h)
        self.rays = Fn.ray_setup(self.cam, WH, self.vshape, self.sr)
        self.rays_h = tuple(t.cpu().numpy() for t in self.rays)
        self.hit = int((self.rays_h[3] > 0).sum())
        self._refs = {}

    def tf_of(self, v):
        return self.tf_h[v] if self.tf_h.ndim == 3 else self.tf_h

    def forward(self):
        ws = self.Fn.alloc_workspace(self.V, self.WH, self.vshape, self.R, dev())
        assert ws is not None
        out, _ = self.Fn.march_fwd(self.vol, self.tf, self.cam, *self.rays, self.S, self.sr, workspace=ws)
        return ws, out, self.Fn.workspace_stats(ws)

    def backward(self, ws, out, g, want_tf=True):
        dv, dt = self.Fn.march_bwd(self.vol, self.tf, self.cam, *self.rays, self.S, self.sr, T(g), out, want_vol=True, want_tf=want_tf,
                                   workspace=ws)
        return dv.float().cpu().numpy(), None if dt is None else dt.cpu().numpy()

    def refs(self, O, g, key=None):
        """-> ((dv64, dt64), (dv32, dt32)): the oracle's gradients for the upstream gradient g (views, W, H, 4) on the GPU's ray
        buffers; computed once per key and shared."""
        if key is not None and key in self._refs:
            return self._refs[key]
        eh, xh, rh, nh = self.rays_h
        res = []
        for f in (np.float64, np.float32):
            dv = np.zeros(self.vshape, f)
            dt = np.zeros(self.tf_h.shape, f)
            for v in range(self.V):
                a, b = O.march_bwd(self.vol_o.astype(f), self.tf_of(v).astype(f), self.cams_h[v].astype(f), eh[v].astype(f),
                                   xh[v].astype(f), rh[v].astype(f), nh[v], self.S, self.sr, g[v].astype(f))
                dv += a
                if self.tf_h.ndim == 3:
                    dt[v] = b
                else:
                    dt += b
            res.append((dv, dt))
        if key is not None:
            self._refs[key] = tuple(res)
        return tuple(res)


def randn_g(V, WH, seed=2):
    return np.random.RandomState(seed).randn(V, *WH, 4).astype(np.float32)


def check(O, sc, what, g=None, want_tf=True, cap=True, key=None):
    """One forward + d_volume backward through a workspace under the rule and the conditions every case shares."""
    g = randn_g(sc.V, sc.WH) if g is None else g
    ws, out, st_f = sc.forward()
    dv, dt = sc.backward(ws, out, g, want_tf)
    st = sc.Fn.workspace_stats(ws)
    (dv64, dt64), (dv32, dt32) = sc.refs(O, g, key)
    print("rows %s rays %d per-ray %d items %d f64 bricks %d" % (what, sc.hit, int(st_f[2]), int(st_f[5]), int(st[4])))
    assert int(st[9]) == 0, what
    if cap:
        assert int(st_f[2]) <= 0.1 * sc.hit, (what, int(st_f[2]), sc.hit)
    e, e32 = rule(dv, dv64, dv32, what + " d_volume")
    if want_tf:
        rule(dt, dt64, dt32, what + " d_tf")
    else:
        assert dt is None
    return dict(dv=dv, dt=dt, dv64=dv64, st_f=st_f, st=st, err=e, err32=e32, ws=ws, out=out, g=g)


def ramp_tf(O, R=64, top=0.03):
    tf = O.bench_tf(R, 0.02)
    tf[:, 3] = np.linspace(0.0, top, R)
    return tf


# ---- A. ray lengths around the 64-sample pass --------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 127, 129])
def test_ray_length_around_a_pass(oracle, Fn, S):
    """Every ray longer than max_samples = S is marched for exactly S samples, at sampling rate 16 through a 20^3 volume (a ray
    stays in one brick for up to ~200 samples): passes with one to three live lanes, a full pass, and last passes of 1, 63 and
    one sample behind full ones -- whose transposed lanes read source lanes past the end of the wave's samples."""
    sc = Scene(Fn, oracle.synth_volume(20), ramp_tf(oracle), oracle.in_circles(0.3), (12, 10), 16.0, S)
    # S = 1: every ray is a single-sample ray, and those belong to the per-ray pass by design (workspace_stats[2]): no cap
    check(oracle, sc, "A sr16 S=%d" % S, cap=S > 1)


# ---- B. several segments per pass; storage formats; d_volume alone ----------------------------------------------------------------

@pytest.fixture(scope="module")
def seg_scenes(oracle, Fn):
    cache = {}

    def get(sr, f16):
        if (sr, f16) not in cache:
            cache[(sr, f16)] = Scene(Fn, oracle.synth_volume(36), ramp_tf(oracle), oracle.in_circles(0.3), (40, 40), sr, BIG, f16=f16)
        return cache[(sr, f16)]
    return get


@pytest.mark.parametrize("want_tf", [True, False], ids=["vol+tf", "vol"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("sr", [1.0, 2.0])
def test_passes_of_several_segments(oracle, Fn, seg_scenes, sr, f16, want_tf):
    """A 36^3 volume (3^3 bricks) under a 40^2 image at rates 1 and 2: a ray's segment in a brick holds 10-40 samples, so every
    64-sample pass holds several segments of several rays and a transposed lane takes over a sample of another ray and entry."""
    sc = seg_scenes(sr, f16)
    check(oracle, sc, "B sr%g %s %s" % (sr, "f16" if f16 else "f32", "vol+tf" if want_tf else "vol"), want_tf=want_tf, key="g2")


# ---- C. double accumulators -------------------------------------------------------------------------------------------------------

def test_wide_range_upstream_gradient_takes_double_boxes(oracle, Fn, seg_scenes):
    """|grad_out| spans e^18 from pixel to pixel: more than 2^6 within a brick's candidates, so the boxes accumulate in double
    (ACC_F64) -- the exchange serves that format too."""
    sc = seg_scenes(1.0, False)
    g = randn_g(1, sc.WH)
    g *= np.exp(np.random.default_rng(5).uniform(-9, 9, size=(1, *sc.WH, 1))).astype(np.float32)
    res = check(oracle, sc, "C wide range", g=g)
    assert int(res["st"][4]) > 0


# ---- D. clamp and drop ------------------------------------------------------------------------------------------------------------

def test_absurd_and_nan_pixels_leave_the_other_rays_alone(oracle, Fn, seg_scenes):
    """One pixel with an upstream gradient of 1e30 (clamped, its bricks in double) and one NaN pixel (dropped): the output is finite,
    and every voxel those two rays do not reach is what the same call computes without them -- to 1e-5 of the scale, D8's floor:
    the two calls differ there only in the order of the flush's float atomics and in the accumulator format of the bricks the
    1e30 ray crosses (fixed point to 2^-40 of the brick's largest upstream gradient against double)."""
    sc = seg_scenes(1.0, False)
    n_h = sc.rays_h[3][0]
    px = np.argwhere(n_h > 30)[[200, 700]]
    g = randn_g(1, sc.WH)
    ok = g.copy()
    bad = g.copy()
    mask = np.zeros(sc.WH, bool)
    for p in px:
        ok[0, p[0], p[1]] = 0.0
        mask[p[0], p[1]] = True
    bad[0, px[0][0], px[0][1], 1] = 1e30
    bad[0, px[1][0], px[1][1], 2] = np.nan
    res = check(oracle, sc, "D without the two pixels", g=ok)
    dv_bad, dt_bad = sc.backward(res["ws"], res["out"], bad)
    assert np.isfinite(dv_bad).all() and np.isfinite(dt_bad).all()
    assert int(sc.Fn.workspace_stats(res["ws"])[4]) > 0
    # the voxels the two rays reach: two probe gradients, so that a cancellation in one cannot hide a voxel
    eh, xh, rh, nh = sc.rays_h
    sv = np.zeros(sc.vshape, bool)
    for seed in (0, 1):
        gp = np.zeros((*sc.WH, 4), np.float64)
        gp[mask] = np.random.default_rng(seed).uniform(0.5, 1.5, size=(int(mask.sum()), 4))
        a, _ = oracle.march_bwd(sc.vol_o.astype(np.float64), sc.tf_h.astype(np.float64), sc.cams_h[0].astype(np.float64), eh[0].astype(np.float64),
                                xh[0].astype(np.float64), rh[0].astype(np.float64), nh[0], sc.S, sc.sr, gp)
        sv |= a != 0
    scale = float(np.abs(res["dv64"]).max())
    d = float(np.abs(dv_bad - res["dv"])[~sv].max())
    print("rows D reached voxels %d of %d, elsewhere max diff / scale %.3g" % (sv.sum(), sv.size, d / scale))
    assert 0 < sv.sum() < 0.2 * sv.size
    assert d <= 1e-5 * scale, d / scale


# ---- E. samples beyond the range of the fixed-point box ---------------------------------------------------------------------------

def flat_scene(O, Fn):
    """A volume that is flat at 1e-7 of synth_volume()'s contrast AROUND ZERO, under a TF of constant alpha 0.05: the central
    differences are ~1e-10, their normalisation amplifies the normal's adjoint by 1e7 and more -- far beyond 2^12 x the brick's
    largest upstream gradient -- while float32 keeps its relative precision (a volume that flat around 0.5 would leave only
    rounding noise of the differences). With the two CPU oracles alone: err32 = 7.6e-5 of the scale for d_volume, 8e-6 for d_tf,
    and one ray's largest d_volume entry is 1.7e6 x its upstream gradient."""
    return Scene(Fn, (1e-7 * O.synth_volume(24)).astype(np.float32), O.bench_tf(64, 0.05), O.in_circles(0.3), (16, 16), 1.0, BIG)


def test_samples_beyond_the_fixed_point_range_bypass_the_box(oracle, Fn):
    """Adjoints beyond the box's range go straight to the gradient volume (ACC_GLOBAL), in the lane's own order and BEFORE the
    exchange; the rest of the pass is exchanged and scattered as usual. That such samples exist is shown on one ray: its d_volume
    entries -- each the sum of at most 16 samples' shares (the taps reach two cells, a cell holds ~2 samples at rate 1, and the
    shares are below the adjoint's bound) -- exceed 16 x 2^13 x its upstream gradient, so some sample's bound exceeds 2^13 x that,
    the largest limit its brick can have."""
    sc = flat_scene(oracle, Fn)
    res = check(oracle, sc, "E flat around zero")
    assert res["err32"] <= 2e-4, res["err32"]   # float32 is good for this scene (flat_scene: 7.6e-5 with the oracles alone)
    eh, xh, rh, nh = sc.rays_h
    i, j = sc.WH[0] // 2, sc.WH[1] // 2
    assert nh[0][i, j] > 10
    g1 = np.zeros((*sc.WH, 4), np.float64)
    g1[i, j] = res["g"][0, i, j]
    a, _ = oracle.march_bwd(sc.vol_o.astype(np.float64), sc.tf_h.astype(np.float64), sc.cams_h[0].astype(np.float64), eh[0].astype(np.float64),
                            xh[0].astype(np.float64), rh[0].astype(np.float64), nh[0], sc.S, sc.sr, g1)
    amp = float(np.abs(a).max() / np.abs(g1).max())
    print("rows E one ray: max |d_volume| / max |grad_out| = %.3g" % amp)
    assert amp > 16 * 2.0 ** 13


# ---- F. heavy bricks: the work-item kernel ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("want_tf", [True, False], ids=["vol+tf", "vol"])
def test_camera_inside_the_volume(oracle, Fn, want_tf):
    """A camera inside a 48^3 volume: the bricks around the eye are candidates of every pixel and are cut into overflow work
    items -- brick_flat_items_kernel shares the body and the exchange."""
    sc = Scene(Fn, oracle.synth_volume(48), ramp_tf(oracle), np.array((0.2, 0.1, 0.3), np.float32), (48, 40), 1.0, BIG)
    res = check(oracle, sc, "F inside %s" % ("vol+tf" if want_tf else "vol"), want_tf=want_tf)
    assert int(res["st_f"][5]) > 0   # work items existed


# ---- G. wide taps -----------------------------------------------------------------------------------------------------------------

def test_wide_taps(oracle, Fn):
    """An axis longer than 991 voxels: NARROW = false, both outside planes of an axis may receive a share. The smooth analytic
    field of tests/test_gpu_tf_tape_edges.py (float32 is good for it)."""
    vshape = (1100, 20, 16)
    i, j, k = (np.arange(v, dtype=np.float64) for v in vshape)
    vol = (0.5 + 0.45 * np.sin(0.05 * i)[:, None, None] * np.cos(0.3 * j)[None, :, None] * np.sin(0.5 + 0.3 * k)[None, None, :])
    tf = oracle.bench_tf(32, 0.02); tf[:, 3] = np.linspace(0.004, 0.05, 32)
    sc = Scene(Fn, vol.astype(np.float32), tf, np.array((0.4, 0.3, 2.4), np.float32), (24, 20), 1.0, BIG)
    assert int(sc.rays_h[3].max()) > 1000
    check(oracle, sc, "G long-x")


# ---- H. views ---------------------------------------------------------------------------------------------------------------------

def test_two_views_with_a_tf_each(oracle, Fn):
    tf = ramp_tf(oracle)
    tfs = np.stack([tf, np.clip(tf[::-1] * 0.8, 0, 1)]).astype(np.float32)
    cams = np.stack([oracle.in_circles(0.3), oracle.in_circles(2.2)])
    sc = Scene(Fn, oracle.synth_volume(32), tfs, cams, (24, 20), 2.0, BIG)
    res = check(oracle, sc, "H two views", g=randn_g(2, (24, 20)))
    assert res["dt"].shape == (2, 64, 4)
