"""The TF-only backward over the per-sample tape (DR_TAPE_TF: csrc/tf_tape.hip and the TAPE instantiations of the brick forward,
csrc/march_flat.hip) at the edges of its machinery: ray lengths on either side of every pass boundary (passes of 256 samples at
four per lane while more than 128 are left, a last pass at two per lane), the work items of heavy bricks, the wide-tap kernels, air
under an exactly transparent TF, termination under right and wrong hints, views and row bands, R at both ends of its range, wide and
non-finite upstream gradients, and the reuse of one tape.

Every comparison is DESIGN.md D8's: on the GPU's own ray buffers, the C oracle's d_tf in float64 is the reference and the same
oracle in float32 says what float32 arithmetic costs on this scene,

    err = max |got - ref64|,  err32 = max |ref32 - ref64|,  scale = max |ref64|:   err <= 3 err32 + 1e-5 scale

(the factor 3 as in tests/camgrad_gpu.py, the floor as tests/test_gpu_tv_loss.py has it for gradients). Besides: d_tf is finite, the
backward found its forward's tape (workspace_stats[9] == 0), and the tape did the work -- the rays of the per-ray fallback
(workspace_stats[2]) are at most a tenth of the rays that have samples -- unless a case says why not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
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
    print("tape %s err/scale %.3g err32/scale %.3g scale %.3g" % (what, err / max(scale, 1e-300), err32 / max(scale, 1e-300), scale))
    assert np.isfinite(got).all(), what
    assert np.isfinite(ref64).all() and scale > 0.0, what   # (a scene without a defined gradient tests nothing)
    assert err <= 3.0 * err32 + 1e-5 * scale, (what, err / scale, err32 / scale)
    return err / scale, err32 / scale


def device_volume(vol_h, f16=False, strided=False):
    """-> (the device tensor the kernels read, the float32 array the references read)"""
    if f16:
        return T(vol_h.astype(np.float16)), vol_h.astype(np.float16).astype(np.float32)
    if strided:   # a slice of a larger tensor
        big = torch.zeros(tuple(v + 3 for v in vol_h.shape), device=dev())
        vol = big[1:1 + vol_h.shape[0], 2:2 + vol_h.shape[1], 0:vol_h.shape[2]]
        vol.copy_(T(vol_h))
        assert not vol.is_contiguous()
        return vol, vol_h
    return T(vol_h), vol_h


class Scene:
    """Inputs on host and device, and the GPU's own ray buffers of one whole image per view."""

    def __init__(self, Fn, vol_h, tf_h, cams, WH, sr, S, f16=False, strided=False):
        self.Fn, self.WH, self.sr, self.S = Fn, WH, float(sr), int(S)
        self.cams_h = np.atleast_2d(np.asarray(cams, np.float32))
        self.V = len(self.cams_h)
        self.tf_h = np.ascontiguousarray(tf_h, np.float32)
        self.R = self.tf_h.shape[-2]
        self.vshape = vol_h.shape
        self.vol, self.vol_o = device_volume(vol_h, f16, strided)
        self.tf, self.cam = T(self.tf_h), T(self.cams_h)
        self.set_rays(*Fn.ray_setup(self.cam, WH, self.vshape, self.sr))

    def set_rays(self, e, x, r, n):
        self.rays = (e, x, r, n)
        self.rays_h = tuple(t.cpu().numpy() for t in (e, x, r, n))
        self.hit = int((self.rays_h[3] > 0).sum())

    def tf_of(self, v):
        return self.tf_h[v] if self.tf_h.ndim == 3 else self.tf_h

    def workspace(self, WH=None):
        ws = self.Fn.alloc_workspace(self.V, WH or self.WH, self.vshape, self.R, dev(), tape=(self.S, self.sr))
        assert ws is not None
        return ws

    def forward(self, ws, hints=0):
        out, steps = self.Fn.march_fwd(self.vol, self.tf, self.cam, *self.rays, self.S, self.sr, workspace=ws, hints=hints, tape=True)
        return out, steps, self.Fn.workspace_stats(ws)

    def backward(self, ws, out, g):
        _, dt = self.Fn.march_bwd(self.vol, self.tf, self.cam, *self.rays, self.S, self.sr, T(g), out, want_vol=False, workspace=ws,
                                  tape=True)
        return dt.cpu().numpy()

    def oracle_fwd(self, O):
        eh, xh, rh, nh = self.rays_h
        return [O.march_fwd(self.vol_o, self.tf_of(v), self.cams_h[v], eh[v], xh[v], rh[v], nh[v], self.S, self.sr, 0)
                for v in range(self.V)]

    def refs(self, O, g):
        """-> (ref64, ref32): the oracle's d_tf for the upstream gradient g (views, W, H, 4) on the GPU's ray buffers"""
        eh, xh, rh, nh = self.rays_h
        res = []
        for f in (np.float64, np.float32):
            acc = np.zeros(self.tf_h.shape, f)
            for v in range(self.V):
                _, b = O.march_bwd(self.vol_o.astype(f), self.tf_of(v).astype(f), self.cams_h[v].astype(f), eh[v].astype(f),
                                   xh[v].astype(f), rh[v].astype(f), nh[v], self.S, self.sr, g[v].astype(f), want_vol=False)
                if self.tf_h.ndim == 3:
                    acc[v] = b
                else:
                    acc += b
            res.append(acc)
        return res[0], res[1]


def randn_g(V, WH, seed=2):
    return np.random.RandomState(seed).randn(V, *WH, 4).astype(np.float32)


def check(O, sc, what, g=None, hints=0, cap=True, found=True):
    """One taped forward + backward under the rule and the conditions every case shares -> what the case looks at further."""
    Fn = sc.Fn
    g = randn_g(sc.V, sc.WH) if g is None else g
    ws = sc.workspace()
    out, steps, st_f = sc.forward(ws, hints)
    got = sc.backward(ws, out, g)
    st = Fn.workspace_stats(ws)
    ref64, ref32 = sc.refs(O, g)
    print("tape %s rays %d per-ray %d items %d repaired views %d exact %d" % (what, sc.hit, int(st_f[2]), int(st_f[5]), int(st_f[8]),
                                                                              int(st_f[15])))
    if found:
        assert int(st[9]) == 0, what
    if cap:
        assert int(st_f[2]) <= 0.1 * sc.hit, (what, int(st_f[2]), sc.hit)
    e, e32 = rule(got, ref64, ref32, what)
    return dict(got=got, ref64=ref64, ref32=ref32, ws=ws, out=out, steps=steps, st_f=st_f, st=st, g=g, err=e, err32=e32)


def ramp_tf(O, R=64, top=0.03):
    tf = O.bench_tf(R, 0.02)
    tf[:, 3] = np.linspace(0.0, top, R)
    return tf


# ---- A. ray length at every pass boundary ---------------------------------------------------------------------------------------

S_SWEEP = [1, 2, 3, 127, 128, 129, 130, 255, 256, 257, 383, 384, 385, 511, 512, 513, 514]


def _length_case(O, Fn, S, vol_h, tf_h, sr, cam, what, f16=False):
    sc = Scene(Fn, vol_h, tf_h, cam, (12, 10), sr, S, f16=f16)
    res = check(O, sc, what, cap=S > 1)   # S = 1: every ray is a single-sample ray, whichever pass serves those: no cap
    steps = res["steps"].cpu().numpy()
    assert np.array_equal(steps[0], sc.oracle_fwd(O)[0][1])
    at_S = int((steps == S).sum())
    print("tape %s rays with steps == S: %d of %d" % (what, at_S, sc.hit))
    assert 2 * at_S >= sc.hit > 0, (what, at_S, sc.hit)   # S is the length of most rays: what makes it the tested length
    return res


@pytest.mark.parametrize("S", S_SWEEP)
def test_ray_length_at_every_pass_boundary(oracle, Fn, S):
    """Every ray longer than max_samples = S is marched for exactly S samples: S on either side of 128 (one pass of two per lane /
    one of four), 256, 384 (a pass of four, then the last 128 at two per lane / two passes of four), 512; the composite is carried
    from pass to pass over lane 63. Sampling rate 16 on a 20^3 volume (the DR_FWD_K_HI forward): no ray terminates early."""
    _length_case(oracle, Fn, S, oracle.synth_volume(20), ramp_tf(oracle), 16.0, oracle.in_circles(0.3), "A sr16 S=%d" % S)


@pytest.mark.parametrize("S", [128, 129, 256, 257])
def test_ray_length_at_pass_boundaries_low_rate_forward(oracle, Fn, S):
    """The same boundaries behind the DR_FWD_K forward (sampling rates below 1.75): rate 1.5 through a 96^3 volume."""
    _length_case(oracle, Fn, S, oracle.synth_volume(96), ramp_tf(oracle), 1.5, oracle.in_circles(0.3), "A sr1.5 S=%d" % S)


def noise_scene():
    vol = np.random.RandomState(11).rand(64, 64, 64).astype(np.float32)[:20, :20, :20]
    return np.ascontiguousarray(vol)


@pytest.mark.parametrize("S", [129, 257, 385])
def test_ray_length_with_a_run_per_sample(oracle, Fn, S):
    """White noise under a 300-entry TF at rate 16: consecutive samples hardly ever share a TF cell, so a lane's four samples are up
    to four runs of d_tf -- one of them emitted inside the lane -- on both sides of a pass boundary."""
    _length_case(oracle, Fn, S, noise_scene(), ramp_tf(oracle, 300, 0.01), 16.0, oracle.in_circles(0.3), "A noise R300 S=%d" % S)


@pytest.mark.parametrize("S", [129, 257])
def test_ray_length_float16_volume(oracle, Fn, S):
    _length_case(oracle, Fn, S, oracle.synth_volume(20), ramp_tf(oracle), 16.0, oracle.in_circles(0.3), "J f16 S=%d" % S, f16=True)


# ---- B. heavy bricks: the overflow-item kernel with TAPE ------------------------------------------------------------------------

@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("sr", [1.0, 2.0])
@pytest.mark.parametrize("cam", [(0.2, 0.1, 0.3), (0.9, 0.3, -1.15)], ids=["inside", "corner"])
def test_heavy_bricks_leave_their_tape_through_work_items(oracle, Fn, cam, sr, f16):
    """A camera inside or next to the volume: a brick with more than 1024 candidate pixels in its screen box is cut into overflow
    work items, marched by a kernel of their own -- with TAPE its own instantiation."""
    sc = Scene(Fn, oracle.synth_volume(32), ramp_tf(oracle), np.array(cam, np.float32), (48, 40), sr, BIG, f16=f16)
    res = check(oracle, sc, "B %s sr%g %s" % (cam, sr, "f16" if f16 else "f32"))
    assert int(res["st_f"][5]) > 0   # work items existed


# ---- C. wide taps ---------------------------------------------------------------------------------------------------------------

def test_wide_taps_leave_their_tape(oracle, Fn):
    """An axis longer than 991 voxels: taps_narrow == false, the F1<TAPE, NARROW = false> instantiations. A smooth analytic field:
    the two CPU oracles agree to 3.6e-6 of the scale on it (asserted: 3e-5 or better), so that the rule stays tight -- white noise
    averaged once per axis moves a float32 march by 2.2e-4 here (the sample position along 1100 voxels has 6e-5 voxels of
    rounding), and a field as flat as synth_volume() stretched over the long axis by 8e-4 (its normals cancel)."""
    vshape = (1100, 20, 16)
    i, j, k = (np.arange(v, dtype=np.float64) for v in vshape)
    vol = (0.5 + 0.45 * np.sin(0.05 * i)[:, None, None] * np.cos(0.3 * j)[None, :, None] * np.sin(0.5 + 0.3 * k)[None, None, :])
    tf = oracle.bench_tf(32, 0.02); tf[:, 3] = np.linspace(0.004, 0.05, 32)
    sc = Scene(Fn, vol.astype(np.float32), tf, np.array((0.4, 0.3, 2.4), np.float32), (24, 20), 1.0, BIG)
    assert int(sc.rays_h[3].max()) > 1000
    res = check(oracle, sc, "C long-x")
    assert res["err32"] <= 3e-5, res["err32"]


# ---- D. air under an exactly transparent TF -------------------------------------------------------------------------------------

@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("sr", [1.0, 2.0])
@pytest.mark.parametrize("cam", ["orbit", "inside"])
def test_air_under_an_exactly_transparent_tf(oracle, Fn, cam, sr, strided):
    """96 % of the voxels classify into texels whose alpha is exactly 0. Their colour gradient is exactly 0, their ALPHA gradient the
    largest entry of d_tf (alpha = 0 has a slope): a taped forward that skipped air like the untaped one -- empty bricks, unlit
    segments, unshaded transparent samples -- or left a stale tape there would be wrong by the full scale."""
    tf = oracle.bench_tf(64, 0.05)
    tf[:32, 3] = 0.0
    cam_h = oracle.in_circles(0.4) if cam == "orbit" else np.array((0.2, 0.1, 0.3), np.float32)
    vol_h = oracle.synth_volume(32)
    assert (vol_h < 0.5).mean() > 0.9
    sc = Scene(Fn, vol_h, tf, cam_h, (48, 40), sr, BIG, strided=strided)
    res = check(oracle, sc, "D %s sr%g %s" % (cam, sr, "strided" if strided else "dense"))
    got, scale = res["got"], float(np.abs(res["ref64"]).max())
    assert (got[:31, :3] == 0).all()
    assert float(np.abs(got[:31, 3]).max()) >= 0.5 * scale


# ---- E. termination with a tape -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [2.0, 8.0])
def test_termination_with_a_tape_under_right_and_wrong_hints(oracle, Fn, sr):
    """The tf1 preset: a third of the rays terminate, their live counts on both sides of several pass boundaries. No hint, the false
    claim "no ray terminates" (DR_HINT_NO_EARLY_TERMINATION: the device repairs the view ray by ray, so the tape serves nobody) and
    "many rays terminate" (the grouped pre-pass: the tape holds live samples only) choose a path, never a result."""
    from differender_amd.utils import get_tf
    tf = get_tf("tf1", 64).t().contiguous().numpy()
    sc = Scene(Fn, oracle.synth_volume(48), tf, oracle.in_circles(0.3), (48, 40), sr, BIG)
    ref_img, ref_steps = sc.oracle_fwd(oracle)[0]
    n_h = sc.rays_h[3][0]
    assert int(((ref_steps < n_h) & (n_h > 0)).sum()) > 0.2 * sc.hit   # rays do terminate
    g = randn_g(1, sc.WH)
    for hints in (0, 0x100, 0x200):
        res = check(oracle, sc, "E sr%g hints %#x" % (sr, hints), g=g, hints=hints, cap=hints != 0x100)
        if hints == 0x100:
            assert int(res["st_f"][8]) > 0   # the wrong hint was noticed
        assert np.array_equal(res["steps"][0].cpu().numpy(), ref_steps)
        assert float(np.abs(res["out"][0].cpu().numpy() - ref_img).max()) <= FWD_TOL


def test_rays_ending_on_an_exactly_opaque_sample(oracle, Fn):
    """White noise under a TF whose alpha is exactly 0 below texel 56 and exactly 1 from there, at sampling rate 1: a quarter of
    the rays end on a sample of opacity 1 -- transmittance 0 behind it, 1 / (1 - op) infinite. The last sample of a ray has no
    suffix to divide (tape_pass selects 0 for it): without that select 0 * inf (or a rounding residue * inf) would take the place
    of the largest single contribution of such a ray. Their lengths lie on both sides of 128 (both pass widths). (Rate 1 only:
    at any other rate d/da (1 - a)^(1/sr) is infinite at a = 1, in the reference as well.)"""
    vol = np.random.RandomState(11).rand(64, 64, 64).astype(np.float32)
    tf = oracle.bench_tf(64, 0.0)
    tf[56:, 3] = 1.0
    sc = Scene(Fn, vol, tf, oracle.in_circles(0.3), (24, 20), 1.0, BIG)
    res = check(oracle, sc, "E opaque last sample")
    steps, n_h = res["steps"][0].cpu().numpy(), sc.rays_h[3][0]
    ref_img, ref_steps = sc.oracle_fwd(oracle)[0]
    assert np.array_equal(steps, ref_steps)
    assert float(np.abs(res["out"][0].cpu().numpy() - ref_img).max()) <= FWD_TOL
    opaque = (steps < n_h) & (res["out"][0, :, :, 3].cpu().numpy() == 1.0)   # ended early, on nothing less than opacity 1
    print("tape E opaque last sample: %d of %d rays, %d of them longer than 128" % (opaque.sum(), sc.hit, (steps[opaque] > 128).sum()))
    assert 5 * int(opaque.sum()) >= sc.hit
    assert int((steps[opaque] > 128).sum()) >= 10 and int((steps[opaque] <= 128).sum()) >= 10


# ---- F. views and bands ---------------------------------------------------------------------------------------------------------

def _three_views(O):
    return np.stack([O.in_circles(0.3), O.in_circles(2.2), O.in_circles(4.0, y=-0.4)])


def test_views_sharing_one_tf(oracle, Fn):
    """Three views, one volume, one TF: the views' double tables commit into one d_tf."""
    sc = Scene(Fn, oracle.synth_volume(32), ramp_tf(oracle), _three_views(oracle), (24, 20), 2.0, BIG)
    res = check(oracle, sc, "F shared tf", g=randn_g(3, (24, 20)))
    assert res["got"].shape == (64, 4)


def test_views_with_a_tf_each(oracle, Fn):
    tf = ramp_tf(oracle)
    tfs = np.stack([tf, np.clip(tf * 1.3, 0, 1), np.clip(tf[::-1] * 0.8, 0, 1)]).astype(np.float32)
    sc = Scene(Fn, oracle.synth_volume(32), tfs, _three_views(oracle), (24, 20), 2.0, BIG)
    res = check(oracle, sc, "F tf per view", g=randn_g(3, (24, 20)))
    assert res["got"].shape == (3, 64, 4)


@pytest.mark.parametrize("cut", [7, 12], ids=["odd", "even"])
def test_row_bands_with_a_tape_each(oracle, Fn, cut):
    """One view as two bands of rows (rows=(row0, W)), each with its own taped workspace: the sum of their d_tf against the whole
    image's reference."""
    WH, sr = (24, 20), 2.0
    sc = Scene(Fn, oracle.synth_volume(32), ramp_tf(oracle), oracle.in_circles(0.3), WH, sr, BIG)
    g = randn_g(1, WH)
    got = np.zeros((64, 4), np.float64)
    pieces, per_ray = [], 0
    for row0, nr in ((0, cut), (cut, WH[0] - cut)):
        rows = (row0, WH[0])
        rb = Fn.ray_setup(sc.cam, (nr, WH[1]), sc.vshape, sr, rows=rows)
        ws = Fn.alloc_workspace(1, (nr, WH[1]), sc.vshape, sc.R, dev(), tape=(BIG, sr))
        out, _ = Fn.march_fwd(sc.vol, sc.tf, sc.cam, *rb, BIG, sr, workspace=ws, rows=rows, hints=0, tape=True)
        per_ray += int(Fn.workspace_stats(ws)[2])
        _, dt = Fn.march_bwd(sc.vol, sc.tf, sc.cam, *rb, BIG, sr, T(g[:, row0:row0 + nr]), out, want_vol=False, workspace=ws, rows=rows,
                             tape=True)
        assert int(Fn.workspace_stats(ws)[9]) == 0
        got += dt.cpu().numpy()
        pieces.append(rb)
    whole = tuple(torch.cat([p[k] for p in pieces], dim=1) for k in range(4))
    assert all(torch.equal(a, b) for a, b in zip(whole, sc.rays))   # the bands' rays are the whole image's
    assert per_ray <= 0.1 * sc.hit
    rule(got, *sc.refs(oracle, g), "F bands cut %d" % cut)


# ---- G. R at both ends ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2, 3, 2030])
def test_tf_size_at_both_ends(oracle, Fn, R):
    """R = 2030 is the largest table the fast path serves: 97 440 B of dynamic LDS for the tape kernel's TF and d_tf table."""
    tf = oracle.bench_tf(R, 0.03)
    tf[:, 3] = np.linspace(0.01, 0.06, R)
    sc = Scene(Fn, oracle.synth_volume(24), tf, oracle.in_circles(0.3), (16, 16), 1.0, 4096)
    check(oracle, sc, "G R=%d" % R, g=randn_g(1, (16, 16), seed=3))


def test_no_taped_workspace_beyond_the_largest_tf(Fn):
    assert Fn.alloc_workspace(1, (16, 16), (24, 24, 24), 2031, dev(), tape=(4096, 1.0)) is None
    assert Fn.tape_workspace_bytes(1, (16, 16), (24, 24, 24), 2031, 4096, 1.0) == 0
    assert Fn.tape_workspace_bytes(1, (16, 16), (24, 24, 24), 2030, 4096, 1.0) > 0


# ---- H. the upstream gradient ---------------------------------------------------------------------------------------------------

def _h_scene(O, Fn):
    return Scene(Fn, O.synth_volume(32), ramp_tf(O), O.in_circles(0.3), (24, 20), 2.0, BIG)


def test_wide_range_upstream_gradient(oracle, Fn):
    sc = _h_scene(oracle, Fn)
    rng = np.random.default_rng(5)
    g = randn_g(1, sc.WH)
    g *= np.exp(rng.uniform(-9, 9, size=(1, *sc.WH, 1))).astype(np.float32)
    check(oracle, sc, "H wide range", g=g)


def test_half_the_image_scaled_down(oracle, Fn):
    sc = _h_scene(oracle, Fn)
    g = randn_g(1, sc.WH)
    g[:, : sc.WH[0] // 2] *= np.float32(1e-5)
    check(oracle, sc, "H half at 1e-5", g=g)


def test_non_finite_upstream_gradient_leaves_nothing_behind(oracle, Fn):
    """NaN, +inf and -3e30 in three pixels: d_tf is finite (the sanitising branch is taken wave-wide). Then, on the same
    workspace without a new forward, the backward with those pixels zeroed holds the rule: nothing stale in the LDS table or in the
    call's double table."""
    sc = _h_scene(oracle, Fn)
    ws = sc.workspace()
    out, _, st_f = sc.forward(ws)
    n_h = sc.rays_h[3][0]
    px = np.argwhere(n_h > 100)[[3, 40, 90]]   # three rays with a tape
    g = randn_g(1, sc.WH)
    bad = g.copy()
    bad[0, px[0][0], px[0][1], 0] = np.nan
    bad[0, px[1][0], px[1][1], 3] = np.inf
    bad[0, px[2][0], px[2][1], 1] = -3e30
    got = sc.backward(ws, out, bad)
    assert np.isfinite(got).all()
    for p in px:
        g[0, p[0], p[1]] = 0.0
    got = sc.backward(ws, out, g)
    st = Fn.workspace_stats(ws)
    assert int(st[9]) == 0 and int(st_f[2]) <= 0.1 * sc.hit
    rule(got, *sc.refs(oracle, g), "H after non-finite")


def test_upstream_gradient_at_the_end_of_the_float_range(oracle, Fn):
    sc = _h_scene(oracle, Fn)
    ws = sc.workspace()
    out, _, _ = sc.forward(ws)
    g = np.where(randn_g(1, sc.WH) > 0, np.float32(3e38), np.float32(-3e38)).astype(np.float32)
    got = sc.backward(ws, out, g)
    assert np.isfinite(got).all() and int(Fn.workspace_stats(ws)[9]) == 0


# ---- I. reuse of one tape -------------------------------------------------------------------------------------------------------

def test_backward_calls_sharing_one_tape(oracle, Fn):
    """Two backward calls with different upstream gradients on one taped workspace, each against its own reference; a third with the
    first gradient again agrees with the first call to 1e-6 of the scale (the double atomics are unordered: not bit equality)."""
    sc = _h_scene(oracle, Fn)
    ws = sc.workspace()
    out, _, st_f = sc.forward(ws)
    assert int(st_f[2]) <= 0.1 * sc.hit
    g1, g2 = randn_g(1, sc.WH, seed=6), 3.0 * randn_g(1, sc.WH, seed=7)
    got1 = sc.backward(ws, out, g1)
    got2 = sc.backward(ws, out, g2)
    got3 = sc.backward(ws, out, g1)
    assert int(Fn.workspace_stats(ws)[9]) == 0
    r1 = sc.refs(oracle, g1)
    rule(got1, *r1, "I first")
    rule(got2, *sc.refs(oracle, g2), "I second")
    rule(got3, *r1, "I first again")
    assert float(np.abs(got3 - got1).max()) <= 1e-6 * float(np.abs(r1[0]).max())
