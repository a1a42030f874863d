"""What the GPU tests of the fused 3-D total variation share (test_gpu_tv_loss.py, test_gpu_tv_edges.py): the
float64 / float32 torch references and the D8 rule, the volumes, the kernels' launch plan restated from
tv_loss.hip::fill_params and aligned4, and the entry points called through the C ABI on raw pointers and strides. Importing it
needs no GPU."""
import ctypes
import types

import torch

from differender_amd.utils import fused_tv3d_loss, tv3d

NORMS = [("l1", 1e-3), ("iso", 1e-3), ("iso", 1e-1), ("sq", 1e-3)]


def dev():
    return torch.device("cuda")


# ---- references and the D8 rule --------------------------------------------------------------------------------------------------

def ref(vol, norm, eps, dtype, device="cpu", reduction="mean"):
    v = vol.detach().to(device=device, dtype=dtype).requires_grad_(True)
    loss = tv3d(v, norm, eps, reduction)
    loss.backward()
    return loss.detach().double(), v.grad.detach().double()


def loss_tol(l64, l32):
    return max(3 * abs(float(l32 - l64)), 2e-6 * abs(float(l64)), 1e-7)


def grad_tol(g64, g32):
    """D8 for the gradient: 3x what torch's own float32 evaluation is off by, with its floors. -> (tolerance, max |g64|)."""
    gmax = float(g64.abs().max())
    return max(3 * float((g32 - g64).abs().max()), 1e-5 * gmax, 1e-30), gmax


def check(vol, norm, eps, reduction="mean", device="cpu", loss=None, grad=None):
    """The kernels' loss and gradient (through fused_tv3d_loss unless given) under the D8 rule."""
    from differender_amd import functional as F
    if loss is None:
        v = vol.detach().clone().requires_grad_(True)
        loss = fused_tv3d_loss(v, norm, eps, reduction)
        loss.backward()
        assert loss.dtype == torch.float32 and loss.ndim == 0
        assert v.grad.dtype == vol.dtype and v.grad.shape == vol.shape
        grad = v.grad
    l64, g64 = ref(vol, norm, eps, torch.float64, device, reduction)
    l32, g32 = ref(vol, norm, eps, torch.float32, device, reduction)
    tol = loss_tol(l64, l32)
    loss = float(loss.detach())
    assert abs(loss - float(l64)) <= tol, (loss, float(l64), tol)
    gtol, gmax = grad_tol(g64, g32)
    grads = [(grad, gtol)]
    if vol.dtype == torch.float16:
        # the autograd gradient comes back in the volume's dtype: half an f16 ulp more (2^-25 where it is subnormal); the
        # kernel's own float32 gradient is held to the rule itself
        scale = 1.0 / vol.numel() if reduction == "mean" else 1.0
        grads = [(grad, gtol + 2 ** -11 * gmax + 2 ** -25), (F.tv3d_bwd(vol, scale=scale, norm=norm, eps=eps), gtol)]
    for g, t in grads:
        err = float((g.detach().to(device).double() - g64).abs().max())
        assert err <= t, (err, t)


def volume(shape, seed=0, dtype=torch.float32, flat=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g)
    if flat:
        v = (v * 4).floor() / 4
    return v.to(dtype).to(dev())


def small_ints(shape, seed=0, dtype=torch.float32):
    """Integers 0..7: every difference, square and flux of "l1" and "sq" is exact in float32 (and in float16 storage)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 8, shape, generator=g).to(dtype).to(dev())


# ---- the kernels' plan, restated (tv_loss.hip: fill_params, aligned4) ------------------------------------------------------------

NT, VX, TX, TY, TARGET_BLOCKS, ZMIN = 256, 4, 64, 16, 2048, 16   # threads, voxels per thread along x, tile, chunk rule


def aligned4(ptr, elem, s, n):
    """The 4-wide access is legal: a pointer aligned to 4 elements, x (axis 1 of b, x, y, z) of stride 1, every other stride a
    multiple of 4; an axis of extent 1 is never stepped along."""
    if ptr % (VX * elem):
        return False
    if any(n[a] > 1 and s[a] % VX for a in (0, 2, 3)):
        return False
    return n[1] <= 1 or s[1] == 1


def plan(shape, strides, ptr=0, elem=4, gstrides=None, gptr=0):
    """fill_params for a logical (B, D, H, W) volume with element strides `strides` at byte address `ptr` (elem bytes per
    voxel) and, when gstrides is given, a float32 gradient buffer at gptr. The axes D, H, W go to z, y, x by |stride|, the
    smallest to x; an axis of extent 1 goes last; the sort is stable."""
    B, ext = shape[0], tuple(shape[1:])
    key = lambda k: abs(strides[1 + k]) if ext[k] > 1 else 2 ** 63 - 1
    order = sorted(range(3), key=key)   # (stable, as the insertion sort of the host code)
    p = types.SimpleNamespace(order=tuple("DHW"[k] for k in order))
    p.NB, (p.NX, p.NY, p.NZ) = B, (ext[k] for k in order)
    p.s = (strides[0],) + tuple(strides[1 + k] for k in order)
    p.tiles_x, p.tiles_y = -(-p.NX // TX), -(-p.NY // TY)
    p.tiles = p.tiles_x * p.tiles_y * B
    p.want = -(-TARGET_BLOCKS // p.tiles)
    p.zc = min(max(-(-p.NZ // p.want), ZMIN), p.NZ)
    p.nchunks = -(-p.NZ // p.zc)
    p.chunks = [min(p.zc, p.NZ - c * p.zc) for c in range(p.nchunks)]
    n = (B, p.NX, p.NY, p.NZ)
    p.vec_fwd = aligned4(ptr, elem, p.s, n)
    p.vec_bwd = None
    if gstrides is not None:
        p.g = (gstrides[0],) + tuple(gstrides[1 + k] for k in order)
        p.vec_bwd = p.vec_fwd and aligned4(gptr, 4, p.g, n)
    # the x extent of the last thread of a row that owns voxels: below VX it takes the scalar branch under VEC too
    p.tail = p.NX % VX
    return p


def strides4(t):
    """(B, D, H, W) tensor -> its four element strides, the batch stride 0 when there is one volume (functional._tv_strides)."""
    assert t.ndim == 4
    return ((t.stride(0) if t.shape[0] > 1 else 0),) + tuple(t.stride()[1:])


def plan_of(vol, out=None):
    """plan for a (B, D, H, W) tensor and, when given, the gradient tensor the backward writes."""
    return plan(tuple(vol.shape), strides4(vol), vol.data_ptr(), vol.element_size(),
                None if out is None else strides4(out), 0 if out is None else out.data_ptr())


# ---- the C ABI on raw pointers ---------------------------------------------------------------------------------------------------

def _i64x4(s):
    return (ctypes.c_int64 * 4)(*s)


def abi_fwd(lib, ptr, f16, shape, strides, norm, eps):
    """dr_tv3d_fwd at a raw device address with any (negative too) element strides -> the sum, a 0-d float64 tensor."""
    from differender_amd import _native as N
    from differender_amd import functional as F
    out = torch.empty((), dtype=torch.float64, device=dev())
    rc = lib.dr_tv3d_fwd(ptr, N.DR_F16 if f16 else N.DR_F32, *shape, _i64x4(strides), F._TV_NORMS[norm], eps, out.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    N.check(rc, "dr_tv3d_fwd")
    return out


def abi_bwd(lib, ptr, f16, shape, strides, norm, eps, gptr, gstrides, scale=1.0, accumulate=False):
    """dr_tv3d_bwd at raw device addresses: the caller owns the gradient buffer that gptr and gstrides describe."""
    from differender_amd import _native as N
    from differender_amd import functional as F
    rc = lib.dr_tv3d_bwd(ptr, N.DR_F16 if f16 else N.DR_F32, *shape, _i64x4(strides), F._TV_NORMS[norm], eps, None, scale, gptr,
                         _i64x4(gstrides), int(accumulate), torch.cuda.current_stream().cuda_stream)
    N.check(rc, "dr_tv3d_bwd")


def flipped(t, dims):
    """The address and element strides under which the memory of the (B, D, H, W) tensor t reads as torch.flip(t, dims): the
    pointer at the last element of every flipped axis, its stride negated."""
    ptr, s = t.data_ptr(), list(strides4(t))
    for a in dims:
        ptr += (t.shape[a] - 1) * t.stride(a) * t.element_size()
        s[a] = -t.stride(a)
    return ptr, tuple(s)
