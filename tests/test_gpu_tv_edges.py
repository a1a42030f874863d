"""The fused 3-D total variation (tv_loss.hip) at the edges of its launch plan: partial tiles, z chunks, the 4-wide
vector path and its alignment rules, gradient buffers of another layout, negative and zero strides, offsets beyond 2^31
elements, single voxels on tile corners and chunk boundaries, non-finite voxels and small eps.

The plan is restated in tv_gpu.py (plan, aligned4: NT = 256 threads, VX = 4 voxels per thread along x, a TX x TY = 64 x 16
tile, z chunks of zc = max(ZMIN = 16, ceil(NZ / ceil(TARGET_BLOCKS = 2048 / tiles))) slices; the axes D, H, W go to x, y, z by
|stride|, extent-1 axes last, stable; the 4-wide path needs a pointer aligned to 4 elements, x of stride 1 and every other stride
a multiple of 4, for the volume and, in the backward, for the gradient buffer too). Every case first asserts, against that
restatement, the path it is named for.

Three kinds of bar. Exact: on volumes of the integers 0..7 every operation of "l1" and "sq" is exact in float32 and the sum is
exact in float64, so the sum equals float64 tv3d and the gradient equals float64 autograd to the bit (0 and -0 taken as equal).
Bitwise: one set of values through two paths (vector / scalar, another pointer, pitch or gradient layout that keeps the axis
order) gives the same gradient bits, and sums within 1e-12 relative (the workgroups' float64 atomics come in any order).
D8: tv_gpu.check, 3x what torch's own float32 evaluation is off by, with its floors.

eps: "iso" adds (float)(eps * eps). The entry points turn down (ValueError, DR_EINVAL) an eps whose square is 0 in float32,
where torch's own float32 tv3d gives NaN at flat voxels; down to a subnormal square (eps = 1e-20) the kernels are held to D8."""
import itertools

import pytest
import torch

import tv_gpu as T
from differender_amd import functional as F
from differender_amd.utils import fused_tv3d_loss
from tv_gpu import check, plan_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.float16]
THREE = [("l1", 1e-3), ("iso", 1e-2), ("sq", 1e-3)]
NAN, INF = float("nan"), float("inf")


def _exact(vol, norm):
    """"l1" / "sq" on small integers: the sum and the gradient equal float64 torch's exactly. -> the gradient."""
    assert norm in ("l1", "sq")
    s, g = F.tv3d_fwd(vol, norm), F.tv3d_bwd(vol, norm=norm)
    l64, g64 = T.ref(vol, norm, 1e-3, torch.float64, reduction="sum")
    assert float(s) == float(l64), (tuple(vol.shape), float(s), float(l64))
    g, want = g.cpu(), g64.float()
    assert torch.equal(g, want), (tuple(vol.shape), int((g != want).sum()), (g != want).nonzero()[:8].tolist())
    return g


def _direct(vol, norm, eps):
    """tv3d_fwd and tv3d_bwd themselves (no autograd) under D8. -> (sum, gradient)."""
    s, g = F.tv3d_fwd(vol, norm, eps), F.tv3d_bwd(vol, norm=norm, eps=eps)
    check(vol, norm, eps, "sum", loss=s, grad=g)
    return s, g


def _exact_or_d8(vol, norm, eps):
    return _exact(vol, norm) if norm != "iso" else _direct(vol, norm, eps)[1].cpu()


def _close_sums(a, b):
    a, b = float(a), float(b)
    assert abs(a - b) <= 1e-12 * abs(b), (a, b)


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------------

TILE_W, TILE_H = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129), (1, 15, 16, 17, 33)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
def test_tile_edges(norm, eps, dtype):
    """Every pairing of a row that ends 1, 3 or 0 voxels into a thread's vector, on the first, second or third tile, with a tile
    column that ends on its first, last or second-to-last row."""
    seen = set()
    for W, H in itertools.product(TILE_W, TILE_H):
        vol = T.small_ints((1, 3, H, W), seed=1000 * W + H, dtype=dtype)
        p = plan_of(vol)
        ext = [n for n in (W, H, 3) if n > 1]
        assert (p.NX, p.NY, p.NZ) == tuple(ext + [1] * (3 - len(ext)))   # by stride, the extent-1 axes last
        assert (p.tiles_x, p.tiles_y, p.chunks) == (-(-p.NX // T.TX), -(-p.NY // T.TY), [p.NZ])
        seen.add((p.tiles_x, p.NX % T.TX, p.tiles_y, p.NY % T.TY))
        _exact_or_d8(vol, norm, eps)
    for tiles_x, rx in ((1, 63), (1, 0), (2, 1), (2, 63), (2, 0), (3, 1)):
        for tiles_y, ry in ((1, 15), (1, 0), (2, 1), (3, 1)):
            assert (tiles_x, rx, tiles_y, ry) in seen


# shape -> (tiles, want, zc, chunks)
CHUNKS = {(1, 16, 5, 9): (1, 2048, 16, [16]), (1, 17, 17, 65): (4, 512, 16, [16, 1]), (1, 32, 5, 9): (1, 2048, 16, [16, 16]),
          (1, 33, 5, 9): (1, 2048, 16, [16, 16, 1]), (512, 41, 17, 2): (1024, 2, 21, [21, 20]),
          (400, 50, 17, 2): (800, 3, 17, [17, 17, 16]), (1100, 41, 17, 2): (2200, 1, 41, [41])}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
@pytest.mark.parametrize("shape", list(CHUNKS), ids=lambda s: "x".join(map(str, s)))
def test_chunk_edges(shape, norm, eps, dtype):
    vol = T.small_ints(shape, seed=sum(shape), dtype=dtype)
    p = plan_of(vol)
    assert p.NZ == shape[1] and (p.tiles, p.want, p.zc, p.chunks) == CHUNKS[shape]
    _exact_or_d8(vol, norm, eps)


IMPULSE_SHAPE = (20, 18, 70)
IMPULSES = list(itertools.product((0, 15, 16, 19), (0, 15, 16, 17), (0, 3, 4, 63, 64, 69)))   # (z, y, x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
def test_impulses_on_tile_corners_and_chunk_boundaries(norm, eps, dtype):
    """One voxel of 1 in a volume of zeros, one volume per position: the fluxes that only the low halo owners (row y0 - 1, column
    x0 - 1) or the slice before a chunk compute reach the gradient alone, not in bulk."""
    vol = torch.zeros((len(IMPULSES), *IMPULSE_SHAPE), dtype=dtype, device=DEV)
    for b, (z, y, x) in enumerate(IMPULSES):
        vol[b, z, y, x] = 1.0
    p = plan_of(vol)
    assert (p.tiles_x, p.tiles_y, p.zc, p.chunks) == (2, 2, 16, [16, 4])   # x = 63 | 64, y = 15 | 16, z = 15 | 16 are the seams
    g = _exact_or_d8(vol, norm, eps)
    g64 = T.ref(vol, norm, eps, torch.float64, reduction="sum")[1]
    assert torch.equal(g != 0, g64 != 0)
    per_volume = (g64 != 0).flatten(1).sum(1)
    assert int(per_volume.min()) >= 1 and int(per_volume.max()) == 7   # the voxel and its six neighbours, where they exist


# ---- 2. the vector path and its boundary -----------------------------------------------------------------------------------------

PADDED = (1, 20, 18, 72)        # rows of pitch 72
WIDTHS = (61, 63, 65, 66, 67, 72)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", T.NORMS)
def test_padded_rows(norm, eps, dtype):
    """Rows of pitch 72 of which Wv voxels belong to the volume: the forward is 4-wide, and the thread that ends a row owns
    Wv % 4 voxels. The backward is 4-wide when `out` is padded alike, and scalar into a dense buffer of pitch Wv."""
    base = T.volume(PADDED, seed=21, dtype=dtype)
    assert {w % T.VX for w in WIDTHS} == {0, 1, 2, 3}
    for Wv in WIDTHS:
        view, dense = base[..., :Wv], base[..., :Wv].contiguous()
        g_dense = F.tv3d_bwd(dense, norm=norm, eps=eps)
        pd = plan_of(dense, g_dense)
        assert pd.vec_fwd == pd.vec_bwd == (Wv % T.VX == 0)            # dense: 4-wide only where the pitch Wv allows it
        g_view = F.tv3d_bwd(view, norm=norm, eps=eps)                  # the default buffer is dense
        p = plan_of(view, g_view)
        assert p.vec_fwd and p.tail == Wv % T.VX and g_view.stride() == g_dense.stride() and p.vec_bwd == pd.vec_bwd
        buf = torch.full(PADDED, NAN, device=DEV)
        out = buf[..., :Wv]
        assert plan_of(view, out).vec_bwd
        assert F.tv3d_bwd(view, norm=norm, eps=eps, out=out) is out
        assert torch.equal(g_view, g_dense) and torch.equal(out, g_dense), Wv
        assert bool(torch.isnan(buf[..., Wv:]).all()) and not bool(torch.isnan(out).any()), Wv   # the padding is not written
        s_view = F.tv3d_fwd(view, norm, eps)
        _close_sums(s_view, F.tv3d_fwd(dense, norm, eps))
        check(view, norm, eps, "sum", loss=s_view, grad=out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", T.NORMS)
def test_accumulate_into_a_padded_buffer(norm, eps, dtype):
    """The 4-wide read-modify-write of accumulate=True, and its scalar tail: bitwise prefill + gradient, the padding untouched."""
    base = T.volume(PADDED, seed=22, dtype=dtype)
    up = torch.tensor(2.5, device=DEV)
    for Wv, kw in itertools.product((61, 72), ({}, dict(upstream=up, scale=0.125))):
        view = base[..., :Wv]
        pre = torch.randn(PADDED, generator=torch.Generator().manual_seed(Wv)).to(DEV)
        buf, gbuf = pre.clone(), torch.zeros(PADDED, device=DEV)
        out, g = buf[..., :Wv], gbuf[..., :Wv]
        assert plan_of(view, out).vec_bwd and plan_of(view, g).vec_bwd
        F.tv3d_bwd(view, norm=norm, eps=eps, out=g, **kw)
        F.tv3d_bwd(view, norm=norm, eps=eps, out=out, accumulate=True, **kw)
        assert torch.equal(out, pre[..., :Wv] + g), (Wv, sorted(kw))
        assert torch.equal(buf[..., Wv:], pre[..., Wv:]), (Wv, sorted(kw))
        plain = F.tv3d_bwd(view, norm=norm, eps=eps)
        coef = 2.5 * 0.125 if kw else 1.0
        assert float((g - coef * plain).abs().max()) <= 1e-6 * coef * float(plain.abs().max())


ALIGN_SHAPE = (1, 8, 12, 68)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", T.NORMS)
def test_pointer_alignment(norm, eps, dtype):
    """One volume at element offset k of an aligned allocation: 4-wide needs 16 bytes (f32) or 8 bytes (f16: k = 2 and 6 are
    4-byte aligned only). The gradient buffer's pointer decides the backward's path as well."""
    vals = T.volume(ALIGN_SHAPE, seed=23, dtype=dtype)
    f16 = dtype == torch.float16
    offsets, vector_at = ((0, 2, 4, 6, 8), {0, 4, 8}) if f16 else ((0, 1, 2, 3, 4), {0, 4})
    grads, sums = [], []
    for k in offsets:
        flat = torch.zeros(k + vals.numel(), dtype=dtype, device=DEV)
        assert flat.data_ptr() % 16 == 0
        v = flat[k:].view(ALIGN_SHAPE)
        v.copy_(vals)
        g = F.tv3d_bwd(v, norm=norm, eps=eps)
        p = plan_of(v, g)
        assert p.vec_fwd == p.vec_bwd == (k in vector_at), k
        grads.append(g)
        sums.append(F.tv3d_fwd(v, norm, eps))
    obuf = torch.full((1 + vals.numel(),), NAN, device=DEV)
    out = obuf[1:].view(ALIGN_SHAPE)
    p = plan_of(vals, out)
    assert p.vec_fwd and not p.vec_bwd          # a 4-wide forward with a scalar backward
    grads.append(F.tv3d_bwd(vals, norm=norm, eps=eps, out=out))
    assert bool(torch.isnan(obuf[0]))
    for k, g in enumerate(grads[1:], 1):
        assert torch.equal(g, grads[0]), k
    for s in sums[1:]:
        _close_sums(s, sums[0])
    check(vals, norm, eps, "sum", loss=sums[0], grad=grads[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", T.NORMS)
def test_stride_alignment(norm, eps, dtype):
    """68 voxels a row at pitch 70 (sy % 4 != 0: scalar) and at pitch 72 (4-wide): the same values, the same gradient."""
    vals = T.volume(ALIGN_SHAPE, seed=24, dtype=dtype)
    got = []
    for pitch, vector in ((70, False), (72, True)):
        v = torch.zeros((*ALIGN_SHAPE[:3], pitch), dtype=dtype, device=DEV)[..., :68]
        v.copy_(vals)
        g = F.tv3d_bwd(v, norm=norm, eps=eps)
        p = plan_of(v, g)
        assert p.s[2] == pitch and p.vec_fwd == vector and p.vec_bwd == vector
        got.append((F.tv3d_fwd(v, norm, eps), g))
    assert torch.equal(got[0][1], got[1][1])
    _close_sums(got[0][0], got[1][0])
    check(vals, norm, eps, "sum", loss=got[1][0], grad=got[1][1])


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
def test_out_in_another_axis_order(norm, eps, dtype):
    """A contiguous volume with `out` in the march's (W, D, H) storage, and a volume in that storage with a contiguous `out`:
    the volume's order is the plan's, the gradient's x stride is not 1, so a 4-wide forward goes with a scalar backward."""
    B, D, H, W = 1, 20, 68, 72
    vol = T.volume((B, D, H, W), seed=25, dtype=dtype)
    s0, g0 = _direct(vol, norm, eps)
    assert plan_of(vol, g0).vec_bwd
    out = torch.full((B, W, D, H), NAN, device=DEV).permute(0, 2, 3, 1)
    p = plan_of(vol, out)
    assert p.order == ("W", "H", "D") and p.g == (0, D * H, 1, H) and p.vec_fwd and not p.vec_bwd
    F.tv3d_bwd(vol, norm=norm, eps=eps, out=out)
    assert torch.equal(out, g0)
    pv = vol.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)    # the same values in (W, D, H) storage
    assert torch.equal(pv, vol) and pv.stride() == out.stride()
    s1, g1 = _direct(pv, norm, eps)                                    # x = H now: another order of operations than g0's
    assert g1.stride() == pv.stride() and plan_of(pv, g1).vec_bwd
    out = torch.full((B, D, H, W), NAN, device=DEV)
    p = plan_of(pv, out)
    assert p.order == ("H", "D", "W") and p.g == (0, W, H * W, 1) and (p.tiles_x, p.tail) == (2, 0) and p.vec_fwd and not p.vec_bwd
    F.tv3d_bwd(pv, norm=norm, eps=eps, out=out)
    assert torch.equal(out, g1)


FLIPS = [(3,), (2,), (1,), (1, 2, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
@pytest.mark.parametrize("dims", FLIPS, ids=lambda d: "flip" + "".join("BDHW"[a] for a in d))
def test_negative_strides_through_the_abi(hiplib, dims, norm, eps, dtype):
    """torch makes no negative strides: the memory of a contiguous volume read backwards along W, H, D or all three, straight
    through dr_tv3d_fwd / dr_tv3d_bwd, is torch.flip of it (whose TV is its own: "iso" is not flip-invariant). The gradient
    buffer flipped alike, and plain. At pitch 72 a flip of H or D keeps the 4-wide path."""
    f16 = dtype == torch.float16
    shape = (1, 19, 18, 70 if f16 else 72)
    mem = T.volume(shape, seed=26, dtype=dtype)
    ptr, s = T.flipped(mem, dims)
    assert all((s[a] < 0) == (a in dims) for a in (1, 2, 3))
    assert T.plan(shape, s, ptr, mem.element_size()).vec_fwd == (not f16 and 3 not in dims)
    logical = torch.flip(mem, dims)
    total = T.abi_fwd(hiplib, ptr, f16, shape, s, norm, eps)
    for flip_grad in (True, False):
        gmem = torch.full(shape, NAN, device=DEV)
        gptr, gs = T.flipped(gmem, dims) if flip_grad else (gmem.data_ptr(), T.strides4(gmem))
        p = T.plan(shape, s, ptr, mem.element_size(), gs, gptr)
        assert p.order == ("W", "H", "D") and p.vec_bwd == p.vec_fwd
        T.abi_bwd(hiplib, ptr, f16, shape, s, norm, eps, gptr, gs)
        torch.cuda.synchronize()
        check(logical, norm, eps, "sum", loss=total, grad=torch.flip(gmem, dims) if flip_grad else gmem)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
def test_stride_zero(norm, eps, dtype):
    """An expanded batch (every volume the same memory) and an expanded W axis (x of stride 0)."""
    B, D, H, W = 2, 20, 18, 70
    one = T.volume((1, D, H, W), seed=27, dtype=dtype)
    many = one.expand(B, D, H, W)
    assert plan_of(many).s[0] == 0 and plan_of(many).NB == B
    s1, g1 = _direct(one, norm, eps)
    _close_sums(F.tv3d_fwd(many, norm, eps), B * float(s1))
    gB = F.tv3d_bwd(many, norm=norm, eps=eps)
    assert gB.shape == many.shape and all(torch.equal(gB[b], g1[0]) for b in range(B))
    leaf = one.clone().requires_grad_(True)
    loss = fused_tv3d_loss(leaf.expand(B, D, H, W), norm, eps, reduction="sum")
    loss.backward()
    assert abs(float(loss.detach()) - B * float(s1)) <= 1e-6 * B * float(s1)
    assert torch.equal(leaf.grad, (B * g1).to(dtype))    # B = 2: doubling is exact, in f16 too
    thin = T.volume((1, D, H, 1), seed=28, dtype=dtype)
    wide = thin.expand(1, D, H, W)
    p = plan_of(wide)
    assert p.order == ("W", "H", "D") and p.s[1] == 0 and not p.vec_fwd
    s_wide, g_wide = _direct(wide, norm, eps)
    s_copy, g_copy = _direct(wide.contiguous(), norm, eps)
    assert torch.equal(g_wide, g_copy)
    _close_sums(s_wide, s_copy)
    # no difference along W: W times the TV of the one column (whose W axis, of extent 1, adds nothing)
    assert abs(float(s_wide) - W * float(F.tv3d_fwd(thin, norm, eps))) <= 1e-6 * float(s_wide)


def test_offsets_beyond_2_to_31_elements():
    """A slice stride of 2^29 elements: the last of 5 slices starts at element 2^31, of an f16 volume and then of the f32
    gradient buffer, both views of one allocation that is never touched as a whole. The plan's axis order is the dense one's,
    so the results equal the dense volume's bitwise."""
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        reason = f"{free / 2 ** 30:.1f} GiB of device memory free, this test wants 16 GiB"
        print(reason)
        pytest.skip(reason)
    D, H, W, SZ = 5, 18, 70, 2 ** 29
    shape, strides = (1, D, H, W), (D * SZ, SZ, W, 1)
    last = (D - 1) * SZ + (H - 1) * W + (W - 1)               # the largest element offset of either view
    nbytes = 4 * (last + 1)
    assert last >= 2 ** 31 and nbytes <= 9 * 2 ** 30
    big = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    small = T.volume(shape, seed=29, dtype=torch.float16)
    halves = big.view(torch.float16)
    assert last < halves.numel()
    vol = halves.as_strided(shape, strides)
    vol.copy_(small)
    assert torch.equal(vol, small)
    p = plan_of(vol)
    assert p.order == ("W", "H", "D") and p.s[3] == SZ and (p.NZ - 1) * p.s[3] >= 2 ** 31
    for norm, eps in THREE:
        s0, g0 = _direct(small, norm, eps)
        _close_sums(F.tv3d_fwd(vol, norm, eps), s0)
        assert torch.equal(F.tv3d_bwd(vol, norm=norm, eps=eps, out=torch.empty(shape, device=DEV)), g0)
    floats = big.view(torch.float32)
    assert last < floats.numel()
    out = floats.as_strided(shape, strides)
    p = plan_of(small, out)
    assert p.g[3] == SZ and (p.NZ - 1) * p.g[3] >= 2 ** 31
    for norm, eps in THREE:
        out.fill_(NAN)
        F.tv3d_bwd(small, norm=norm, eps=eps, out=out)
        assert torch.equal(out, F.tv3d_bwd(small, norm=norm, eps=eps))
    del vol, out, halves, floats, big
    torch.cuda.empty_cache()


# ---- 4. non-finite voxels and small eps ------------------------------------------------------------------------------------------

BAD_VOXELS = (NAN, INF, -INF)
BAD_AT = ((9, 7, 30), (9, 16, 64), (16, 7, 30))   # (z, y, x): interior, the tile corner (x, y) = (64, 16), the chunk seam z = 16
# the voxels of the float64 gradient that are not finite, per bad voxel: norm -> (NaN voxel, infinite voxel)
FOOTPRINT = {"l1": (0, 0), "iso": (13, 7), "sq": (7, 7)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,eps", THREE)
def test_non_finite_voxels_in_the_backward(norm, eps, dtype):
    """One NaN, +inf or -inf voxel per volume: the gradient is not finite exactly where float64 autograd's is not (NaN where it
    is NaN, the same infinity where it is infinite), and finite elsewhere under D8."""
    cases = list(itertools.product(BAD_VOXELS, BAD_AT))
    vol = T.volume((len(cases), *IMPULSE_SHAPE), seed=30, dtype=dtype)
    for b, (bad, (z, y, x)) in enumerate(cases):
        vol[b, z, y, x] = bad
    p = plan_of(vol)
    assert (p.tiles_x, p.tiles_y, p.chunks) == (2, 2, [16, 4])
    l64, g64 = T.ref(vol, norm, eps, torch.float64, reduction="sum")
    g32 = T.ref(vol, norm, eps, torch.float32, reduction="sum")[1]
    for b, (bad, _) in enumerate(cases):   # a torch of other semantics (sign(nan), 0 * inf) would show here
        assert int((~torch.isfinite(g64[b])).sum()) == FOOTPRINT[norm][bad == bad], (norm, bad)
    assert torch.equal(torch.isfinite(g32), torch.isfinite(g64))
    g = F.tv3d_bwd(vol, norm=norm, eps=eps).cpu()
    assert torch.equal(torch.isnan(g), torch.isnan(g64))
    inf = torch.isinf(g64)
    assert torch.equal(torch.isinf(g), inf) and torch.equal(g[inf], g64[inf].float())
    fin = torch.isfinite(g64)
    tol, _ = T.grad_tol(g64[fin], g32[fin])
    err = float((g[fin].double() - g64[fin]).abs().max())
    assert err <= tol, (err, tol)
    s = float(F.tv3d_fwd(vol, norm, eps))
    assert s != s and float(l64) != float(l64)   # NaN and inf - inf ... in one sum: NaN, as the reference's


MIN_NORMAL = 2.0 ** -126   # of float32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("eps", [1e-6, 2e-19, 1e-20])
def test_small_eps(eps, dtype):
    """eps^2 an ordinary float32, one within two binades of the smallest normal, and a subnormal: on a piecewise-constant
    volume the flat voxels' flux is 0 / eps = 0, never 0 * inf."""
    eps2 = float(torch.tensor(eps * eps, dtype=torch.float32))
    assert {1e-6: eps2 > 2 ** 40 * MIN_NORMAL, 2e-19: MIN_NORMAL <= eps2 < 4 * MIN_NORMAL, 1e-20: 0 < eps2 < MIN_NORMAL}[eps]
    vol = T.volume((1, *IMPULSE_SHAPE), seed=31, dtype=dtype, flat=True)
    d = [torch.diff(vol.float(), dim=a, append=vol.float().narrow(a, vol.shape[a] - 1, 1)) for a in (1, 2, 3)]
    assert int(((d[0] == 0) & (d[1] == 0) & (d[2] == 0)).sum()) > 100    # flat voxels
    for dt in (torch.float64, torch.float32):
        l, g = T.ref(vol, "iso", eps, dt, reduction="sum")
        assert bool(torch.isfinite(l)) and bool(torch.isfinite(g).all())
    s, g = _direct(vol, "iso", eps)
    assert bool(torch.isfinite(s)) and bool(torch.isfinite(g).all())
    check(vol, "iso", eps)


@pytest.mark.parametrize("eps", [1e-30, 2.0 ** -75])
def test_eps_whose_square_is_zero_in_float32_is_turned_down(hiplib, eps):
    """(float)(eps * eps) == 0 (2^-150 is the tie that rounds to 0): ValueError / DR_EINVAL for "iso", whatever the volume; the
    other norms do not read eps."""
    assert float(torch.tensor(eps * eps, dtype=torch.float32)) == 0.0 and eps * eps > 0.0
    vol = T.volume((1, 4, 5, 6), seed=32)
    for call in (lambda: F.tv3d_fwd(vol, "iso", eps), lambda: F.tv3d_bwd(vol, norm="iso", eps=eps),
                 lambda: fused_tv3d_loss(vol, "iso", eps)):
        with pytest.raises(ValueError):
            call()
    g = torch.full(vol.shape, NAN, device=DEV)
    with pytest.raises(RuntimeError, match="code -1"):
        T.abi_fwd(hiplib, vol.data_ptr(), False, vol.shape, T.strides4(vol), "iso", eps)
    with pytest.raises(RuntimeError, match="code -1"):
        T.abi_bwd(hiplib, vol.data_ptr(), False, vol.shape, T.strides4(vol), "iso", eps, g.data_ptr(), T.strides4(g))
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all())                                    # nothing was launched
    T.abi_bwd(hiplib, vol.data_ptr(), False, vol.shape, T.strides4(vol), "l1", eps, g.data_ptr(), T.strides4(g))
    assert torch.equal(g, F.tv3d_bwd(vol, norm="l1"))
    _direct(vol, "iso", 3e-23)                                           # the smallest eps the message names
