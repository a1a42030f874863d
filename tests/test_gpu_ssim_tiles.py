"""The SSIM loss kernels (image_loss.hip; msssim.hip, D10) where their tiling can go wrong: high-contrast tiles
(the per-tile shift of the moments), every tile height and LDS branch of the backward, tile edges, non-default
data_range / win_sigma / K, signed and negative images, more than 256 planes, and non-finite values in either image.
Each case is held to the D8 rule (3x what torch's own float32 evaluation is off by) against float64 torch on the CPU, with
data_range, win_sigma and K passed through to ssim2d / ms_ssim2d. Each high-contrast case asserts its own premise on the tile
geometry restated below, so that it cannot silently stop testing what it is named for."""
import math

import pytest
import torch
import torch.nn.functional as TF

from differender_amd import functional as F
from differender_amd.utils import MS_SSIM_WEIGHTS, ms_ssim2d, ssim2d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# ---- the tile geometry of csrc/dr_ssim.h (TX, pick_ty, fwd_lds_floats, bwd_lds_floats), restated -----------------------
TX, FWD_TY = 64, 16
LDS_DEFAULT, LDS_MAX, STATIC_LDS = 64 * 1024, 160 * 1024, 256


def _fwd_floats(ty, kh, kw):
    ih, iw = ty + kh - 1, TX + kw - 1
    return 2 * ih * iw + 5 * ty * iw


def _bwd_floats(ty, kh, kw):
    ih, iw, qh, qw = ty + 2 * (kh - 1), TX + 2 * (kw - 1), ty + kh - 1, TX + kw - 1
    return max(2 * ih * iw, 4 * qh * qw) + max(5 * qh * iw, 4 * qh * TX)


def tile_ty(bwd, k, H, W):
    """(TY, opt_in): the tile height pick_ty chooses for a window k on an H x W plane, and whether its LDS is above the
    default 64 KB. A side shorter than the window is not filtered (kh or kw = 1)."""
    kh, kw = (k if H >= k else 1), (k if W >= k else 1)
    floats = _bwd_floats if bwd else _fwd_floats
    for cap in (LDS_DEFAULT, LDS_MAX):
        ty = 16
        while ty >= 1:
            if floats(ty, kh, kw) * 4 + STATIC_LDS <= cap:
                return ty, cap > LDS_DEFAULT
            ty //= 2
    raise AssertionError("no tile fits")


def tile_origins(bwd, k, H, W):
    """The (y0, x0) of every tile of a plane: the forward tiles the Ho x Wo outputs by 64 x 16, the backward the H x W
    inputs by 64 x TY. Either way the shift is taken at the input pixel (y0, x0)."""
    kh, kw = (k if H >= k else 1), (k if W >= k else 1)
    ey, ex = (H, W) if bwd else (H - kh + 1, W - kw + 1)
    ty = tile_ty(bwd, k, H, W)[0]
    return [(y, x) for y in range(0, ey, ty) for x in range(0, ex, TX)]


def tile_block(bwd, k, H, W, y0, x0):
    """The pixels a tile owns (its rows and columns), to judge what most of a tile holds."""
    ty = tile_ty(bwd, k, H, W)[0] if bwd else FWD_TY
    return slice(y0, min(y0 + ty, H)), slice(x0, min(x0 + TX, W))


def pyramid(X, levels):
    """The levels of ms_ssim2d: 2x2 average pooling with a padding of (H % 2, W % 2), the padded zeros counted."""
    out = [X]
    for _ in range(levels - 1):
        X = out[-1]
        out.append(TF.avg_pool2d(X, kernel_size=2, padding=[X.shape[2] % 2, X.shape[3] % 2]))
    return out


def _footprint(level, r, sides):
    """The level-0 rows (or columns) [lo, hi) that pool into row r of `level`; sides[j] = that side at level j."""
    lo, hi = r, r + 1
    for j in range(level, 0, -1):
        p = sides[j - 1] % 2
        lo, hi = max(2 * lo - p, 0), min(2 * hi - p, sides[j - 1])
    return lo, hi


# ---- the float64 reference and the D8 rule ---------------------------------------------------------------------------
def _torch_ref(X, Y, dtype, ms, cfg):
    X = X.detach().cpu().to(dtype).requires_grad_(True)
    Y = Y.detach().cpu().to(dtype).requires_grad_(True)
    if ms:
        s = ms_ssim2d(X, Y, data_range=cfg["data_range"], win_size=cfg["win_size"], win_sigma=cfg["win_sigma"],
                      weights=cfg["weights"], K=cfg["K"])
    else:
        s = ssim2d(X, Y, data_range=cfg["data_range"], win_size=cfg["win_size"], win_sigma=cfg["win_sigma"], K=cfg["K"],
                   nonnegative_ssim=True)
    d = 1.0 - s
    mse = TF.mse_loss(X, Y)
    loss = torch.nan_to_num(d) + mse
    loss.backward()
    return [t.detach().double() for t in (loss, d, mse, X.grad, Y.grad)]


def _cfg(ms, win_size=11, data_range=1.0, win_sigma=1.5, K=(0.01, 0.03), weights=None):
    cfg = dict(data_range=data_range, win_size=win_size, win_sigma=win_sigma, K=K)
    if ms:
        cfg["weights"] = MS_SSIM_WEIGHTS if weights is None else weights
    return cfg


def _kernel(X, Y, ms, cfg):
    fwd, bwd = (F.msssim_mse_fwd, F.msssim_mse_bwd) if ms else (F.dssim_mse_fwd, F.dssim_mse_bwd)
    X, Y = X.to(DEV), Y.to(DEV)
    stats = fwd(X, Y, **cfg)
    gx, gy = bwd(X, Y, stats, want_ref_grad=True, **cfg)
    s = stats.cpu()
    return s[-3], s[-2], s[-1], gx, gy


def _check(X, Y, ms, cfg):
    """(loss, ssim or ms term, mse, dX, dY) of the kernels against float64 torch, with D8's tolerances."""
    got = _kernel(X, Y, ms, cfg)
    r64 = _torch_ref(X, Y, torch.float64, ms, cfg)
    r32 = _torch_ref(X, Y, torch.float32, ms, cfg)
    for name, g, a, b in zip(("loss", "dssim", "mse"), got[:3], r64[:3], r32[:3]):
        g = float(g)
        tol = max(3 * abs(float(b) - float(a)), 1e-6)
        assert abs(g - float(a)) <= tol, (name, g, float(a), tol)
    for name, g, a, b in zip(("dX", "dY"), got[3:], r64[3:], r32[3:]):
        g = g.detach().cpu().double()
        finite = torch.isfinite(a)
        tol = max(3 * float((b - a)[finite].abs().max()), 1e-5 * float(a[finite].abs().max()))
        err = float((g - a)[finite].abs().max())
        assert err <= tol, (name, err, tol)


def _random(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=g)
    return X, (0.7 * X + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)


# ---- a. high-contrast tiles ------------------------------------------------------------------------------------------
# Base images lie in [0, 1] (except "negative"); a variant scales them (data_range 255) or maps them to [-1, 1]
# (data_range 2). Bright origins: X = 1, Y = 0.9 on a dark or exactly black background.
D9_SHAPE = (2, 2, 84, 138)    # k = 11: Wo = 128, Ho = 74 (a partial last forward row of tiles); backward TY 8, 3 x 11 tiles
MS_SHAPE = (1, 2, 176, 192)   # even at every level (176 -> 88 -> 44 -> 22 -> 11, 192 -> ... -> 12): no padding darkens an origin
DARK, BRIGHT = 0.05, 0.8


def _origin_mask(shape, ms, k=11, rows=2):
    """Where the bright origins go, in level-0 pixels: x = 0 (mod 64) on every `rows`-th row (rows = 2 serves any TY >= 2)
    and, for MS-SSIM, the level-0 blocks that pool into each forward and backward tile origin of levels 1..L-1."""
    H, W = shape[2:]
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0::rows, 0::TX] = True
    if ms:
        hs, ws = [H], [W]
        for _ in range(len(MS_SSIM_WEIGHTS) - 1):
            hs.append((hs[-1] + 1) // 2)
            ws.append((ws[-1] + 1) // 2)
        for lv in range(1, len(hs)):
            for bwd in (False, True):
                for y0, x0 in tile_origins(bwd, k, hs[lv], ws[lv]):
                    r0, r1 = _footprint(lv, y0, hs)
                    c0, c1 = _footprint(lv, x0, ws)
                    m[r0:r1, c0:c1] = True
    return m


def _discs(shape, centres, radius=3.0):
    H, W = shape[2:]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.zeros(H, W, dtype=torch.bool)
    for y0, x0 in centres:
        d |= (yy - y0) ** 2 + (xx - x0) ** 2 <= radius * radius
    return d


def _render(shape):
    """A real Raycaster render of the synthetic volume (X with tf1, Y with the gray TF): RGBA, 0 exactly where the rays miss
    the volume's box. shape = (views, 4, H, W)."""
    from differender.utils import get_tf, in_circles
    from differender_amd.volume_raycaster import Raycaster
    from examples.render_nondiff_synthetic import synthetic_volume
    V, C, H, W = shape
    assert C == 4
    vol = synthetic_volume(32, DEV).float()
    rc = Raycaster(vol.shape[-3:], (H, W), 64, jitter=False, max_samples=2048)
    cams = torch.stack([in_circles(0.4), in_circles(2.1)]).float().to(DEV)[:V]
    with torch.no_grad():
        X = rc(vol, get_tf("tf1", 64).to(DEV).float(), cams).cpu()
        Y = rc(vol, get_tf("gray", 64).to(DEV).float(), cams).cpu()
    return X.contiguous(), Y.contiguous()


def high_contrast(case, shape, ms, seed=0):
    """(X, Y) of a high-contrast case in [0, 1] (all negative for "negative")."""
    g = torch.Generator().manual_seed(seed)
    H, W = shape[2:]
    u = lambda: torch.rand(shape, generator=g)  # noqa: E731
    if case == "dark_dots":      # dark noise, bright at every tile origin (and, for MS-SSIM, at every level's)
        X, Y = DARK * u(), DARK * u()
        m = _origin_mask(shape, ms)
        X[..., m], Y[..., m] = 1.0, 0.9
    elif case == "discs":        # small bright discs on an exactly black background, one centred on every tile origin (k = 11)
        o = _origin_mask(shape, ms, rows=8)
        m = o | _discs(shape, [(y, x) for y in range(0, H, 8) for x in range(0, W, TX)])
        X, Y = torch.zeros(shape), torch.zeros(shape)
        X[..., m] = (0.8 + 0.2 * u())[..., m]
        Y[..., m] = (0.7 + 0.2 * u())[..., m]
        X[..., o], Y[..., o] = 1.0, 0.9
    elif case in ("half_black_right", "half_black_left"):   # half of every 64-wide tile black, the other half texture
        tex = (torch.arange(W) % TX < TX // 2) == (case == "half_black_right")
        X, Y = u(), u()
        Y = 0.6 * X + 0.4 * Y
        X[..., ~tex], Y[..., ~tex] = 0.0, 0.0
    elif case == "flat_noise":   # bright and flat, with a little noise
        X, Y = 0.9 + 1e-3 * u(), 0.9 + 1e-3 * u()
    elif case == "flat_hole":    # bright and flat, with one black pixel in every 64 x 16 block
        X, Y = torch.full(shape, 0.9), 0.9 + 1e-3 * u()
        X[..., 8::16, 32::TX] = 0.0
    elif case == "negative":     # all negative and flat
        X, Y = torch.full(shape, -0.7), torch.full(shape, -0.4)
    else:
        raise ValueError(case)
    return X.contiguous(), Y.contiguous()


def _assert_bright_origins(X, ms, k=11):
    """The premise of the origin cases: every forward and backward tile origin of every level is bright in X (and most of each
    tile is dark), on the pyramid ms_ssim2d builds."""
    levels = pyramid(X, len(MS_SSIM_WEIGHTS)) if ms else [X]
    for lv, P in enumerate(levels):
        H, W = P.shape[2:]
        for bwd in (False, True):
            for y0, x0 in tile_origins(bwd, k, H, W):
                assert float(P[..., y0, x0].min()) >= BRIGHT, (lv, bwd, y0, x0, float(P[..., y0, x0].min()))
                rows, cols = tile_block(bwd, k, H, W, y0, x0)
                tile = P[..., rows, cols].flatten(2)
                assert float((tile <= 0.3).double().mean(-1).min()) >= 0.5, (lv, bwd, y0, x0)


CASES = ["dark_dots", "discs", "half_black_right", "half_black_left", "flat_noise", "flat_hole", "negative"]
VARIANTS = {"unit": (1.0, 0.0, 1.0), "x255": (255.0, 0.0, 255.0), "signed": (2.0, -1.0, 2.0)}   # scale, offset, data_range


def _variant(X, Y, variant):
    a, b, dr = VARIANTS[variant]
    return a * X + b, a * Y + b, dr


HC = [(c, v) for c in CASES for v in VARIANTS if not (c == "negative" and v == "signed")]


@pytest.mark.parametrize("ms", [False, True], ids=["dssim", "msssim"])
@pytest.mark.parametrize("case,variant", HC, ids=[f"{c}-{v}" for c, v in HC])
def test_high_contrast_tiles(case, variant, ms):
    shape = MS_SHAPE if ms else D9_SHAPE
    X, Y = high_contrast(case, shape, ms)
    if case in ("dark_dots", "discs"):
        _assert_bright_origins(X, ms)
        _assert_bright_origins(Y / 0.9, ms)
        if case == "discs":
            assert float((X == 0).double().mean()) >= 0.5   # an exactly black background
    elif case.startswith("half"):
        assert float((X == 0).double().mean()) >= 0.45 and float((X[X != 0]).mean()) >= 0.3
    X, Y, dr = _variant(X, Y, variant)
    if variant == "signed":
        assert float(torch.cat([X, Y]).abs().max()) <= 1.0
    _check(X, Y, ms, _cfg(ms, data_range=dr))


@pytest.mark.parametrize("ms", [False, True], ids=["dssim", "msssim"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_render_on_black(variant, ms):
    shape = (2, 4, 176, 192) if ms else (2, 4, 128, 128)
    X, Y = _render(shape)
    # premise: the background is exactly 0 and tile origins land on the object
    assert float((X == 0).double().mean()) >= 0.1 and float((Y == 0).double().mean()) >= 0.1
    H, W = shape[2:]
    for bwd in (False, True):
        on = [float(X[..., y0, x0].max()) >= 0.1 for y0, x0 in tile_origins(bwd, 11, H, W)]
        assert sum(on) >= 3, (bwd, sum(on))
    if variant == "x255":
        # the colour channels only: at data_range 255 the alpha channel (flat at 255 inside the object, 0 outside, so every
        # tile on the silhouette is shifted by 0) puts the kernels' float32 error at ~1e-5 per plane, 10x torch's own there
        X, Y = X[:, :3].contiguous(), Y[:, :3].contiguous()
    X, Y, dr = _variant(X, Y, variant)
    _check(X, Y, ms, _cfg(ms, data_range=dr))


# ---- b. every tile height and LDS branch of the backward -------------------------------------------------------------
# (k, H, W, backward (TY, opt-in)) : both sides >= k; W < k <= H (kw = 1); H < k <= W (kh = 1)
TY_CASES = [(1, 40, 130, (16, False)), (3, 42, 132, (16, False)), (9, 48, 138, (8, False)), (15, 54, 144, (4, False)),
            (17, 56, 146, (2, False)), (19, 58, 148, (16, True)), (27, 66, 156, (16, True)), (29, 68, 158, (8, True)),
            (15, 50, 12, (8, False)), (23, 60, 20, (4, False)), (27, 64, 26, (2, False)), (29, 66, 27, (16, True)),
            (21, 15, 150, (16, False))]


@pytest.mark.parametrize("k,H,W,cell", TY_CASES, ids=[f"k{k}-{H}x{W}-ty{c[0]}{'-optin' if c[1] else ''}"
                                                      for k, H, W, c in TY_CASES])
def test_tile_heights_dssim(k, H, W, cell):
    assert tile_ty(True, k, H, W) == cell
    assert tile_ty(False, k, H, W) == (16, False)
    X, Y = _random((1, 3, H, W), seed=k)
    _check(X, Y, False, _cfg(False, win_size=k))


MS_TY = [(3, (1, 2, 40, 70), (16, False)), (15, (1, 2, 225, 240), (4, False)), (17, (1, 1, 257, 260), (2, False))]


@pytest.mark.parametrize("k,shape,cell", MS_TY, ids=[f"k{k}" for k, _, _ in MS_TY])
def test_tile_heights_msssim(k, shape, cell):
    assert min(shape[2:]) == 16 * (k - 1) + 1 or k == 3
    assert tile_ty(True, k, *shape[2:]) == cell
    X, Y = _random(shape, seed=k)
    _check(X, Y, True, _cfg(True, win_size=k))


# ---- c. tile edges -----------------------------------------------------------------------------------------------
# Wo around one and two tiles; H so that Ho is 16m - 1, 16m, 16m + 1 (forward) and H is 8m - 1, 8m, 8m + 1 (backward)
EDGE_WO, EDGE_H = [63, 64, 65, 128], [55, 56, 57, 58, 59]


@pytest.mark.parametrize("H", EDGE_H)
@pytest.mark.parametrize("Wo", EDGE_WO)
def test_tile_edges_dssim(Wo, H):
    assert tile_ty(True, 11, H, Wo + 10)[0] == 8
    X, Y = _random((1, 2, H, Wo + 10), seed=H * 1000 + Wo)
    _check(X, Y, False, _cfg(False))


@pytest.mark.parametrize("shape", [(1, 3, 162, 194), (1, 2, 194, 163)], ids=["162x194", "194x163"])
def test_odd_and_even_levels_msssim(shape):
    H, W = shape[2:]
    sides = [(s.shape[2], s.shape[3]) for s in pyramid(torch.zeros(shape), len(MS_SSIM_WEIGHTS))]
    assert {h % 2 for h, _ in sides[:-1]} == {0, 1} and {w % 2 for _, w in sides[:-1]} == {0, 1}, sides
    X, Y = _random(shape, seed=H + W)
    _check(X, Y, True, _cfg(True))


# ---- d. non-default window and constants ---------------------------------------------------------------------------
PARAMS = [dict(win_sigma=0.5), dict(win_sigma=3.0), dict(K=(0.05, 0.1))]


@pytest.mark.parametrize("ms", [False, True], ids=["dssim", "msssim"])
@pytest.mark.parametrize("params", PARAMS, ids=["sigma0.5", "sigma3", "K0.05-0.1"])
def test_parameters(params, ms):
    X, Y = _random(MS_SHAPE if ms else D9_SHAPE, seed=5)
    _check(X, Y, ms, _cfg(ms, **params))
    X, Y = high_contrast("dark_dots", MS_SHAPE if ms else D9_SHAPE, ms, seed=6)
    _check(X, Y, ms, _cfg(ms, **params))


# ---- e. more than 256 planes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms,shape", [(False, (301, 3, 24, 40)), (True, (3, 91, 170, 170))], ids=["dssim", "msssim"])
def test_many_planes(ms, shape):
    planes = shape[0] * shape[1]
    assert planes > 256 and planes % 256 != 0
    X, Y = _random(shape, seed=planes)
    _check(X, Y, ms, _cfg(ms))


# ---- f. non-finite values elsewhere ------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [False, True], ids=["dssim", "msssim"])
@pytest.mark.parametrize("where", ["nan_in_y", "inf_in_x"])
def test_non_finite(where, ms):
    shape = MS_SHAPE if ms else D9_SHAPE
    X, Y = _random(shape, seed=9)
    if where == "nan_in_y":
        Y[-1, 0, shape[2] // 3, shape[3] // 2] = float("nan")
    else:
        X[0, 1, shape[2] // 2, shape[3] // 4] = float("inf")
    cfg = _cfg(ms)
    loss, d, mse, gx, gy = _kernel(X, Y, ms, cfg)
    r64 = _torch_ref(X, Y, torch.float64, ms, cfg)
    for name, g, a in zip(("loss", "dssim", "mse"), (loss, d, mse), r64[:3]):
        g, a = float(g), float(a)
        assert (math.isnan(g), math.isinf(g)) == (math.isnan(a), math.isinf(a)), (name, g, a)
        if math.isfinite(a):
            assert abs(g - a) <= 1e-6, (name, g, a)
    # no SSIM gradient is left: the mse term alone, non-finite exactly where an input is
    e = (X.to(DEV) - Y.to(DEV)) * (2.0 / X.numel())
    bad = ~(torch.isfinite(X) & torch.isfinite(Y)).to(DEV)
    for g, sign, a in ((gx, 1.0, r64[3]), (gy, -1.0, r64[4])):
        assert torch.equal(~torch.isfinite(g), bad)
        assert torch.allclose(g[~bad], sign * e[~bad], rtol=1e-6, atol=0)
        finite = torch.isfinite(a)
        assert torch.allclose(g.cpu().double()[finite], a[finite], rtol=1e-5, atol=1e-12)
    # ... and of which kind at the infinite pixel of x: D9 runs the chain through its zero maps,
    # 2 (x - shift) 0 = NaN in both gradients; D10 skips the chain, and the mse term's +-inf stays
    if where == "inf_in_x":
        at = (0, 1, shape[2] // 2, shape[3] // 4)
        if ms:
            assert float(gx[at]) == math.inf and float(gy[at]) == -math.inf
        else:
            assert math.isnan(float(gx[at])) and math.isnan(float(gy[at]))
