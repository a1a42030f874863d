"""Float64 / float32 reference of the projections of a ray bundle: `bundle_reference.slab` followed by
`proj_reference.project` with one origin per ray in the camera's place, differentiated by torch.autograd with the branches
frozen (n, the jitter draw, the slab faces, the t_near clamp, the cells, the argmax). Nothing is derived by hand. For the MIP at
a given argmax: `proj_reference.sample_at`.

Beside the program: group_plan (which path the windowed SUM backward takes per group of 256 consecutive rays: a float32 model of
its decisions, not of its arithmetic, like proj_reference.window_plan), and the cases of tests/test_gpu_proj_bundle.py, which
tests/test_proj_bundle.py checks on the CPU.
"""
import collections
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bundle_reference as BR  # noqa: E402
import proj_reference as PR  # noqa: E402

F32 = BR.F32
RAY_BASE = 3


def run(inp, mode, dtype=torch.float64, arg=None, grads=True, kmax_factor=1.0):
    """inp: vol (VX,VY,VZ), origins, dirs (P,3), grad_out (P,), sr, max_samples (or None); optional t_near, jitter_seed,
    ray_base. The whole program in `dtype`. arg (P,): the MIP sampled at these indices instead of its own argmax.
    kmax_factor: scales the gradient that flows through tmax (the exit distance) -- a mutation of the ray gradient's tail
    coefficient k_max, for the test of the test. -> out (P,), arg (P,) or None, n (P,), entry, exit (P,), d_origin, d_dir (P,3),
    dvol, all numpy (float64 / int64)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    o, d, vol = T(inp["origins"]).requires_grad_(grads), T(inp["dirs"]).requires_grad_(grads), T(inp["vol"]).requires_grad_(grads)
    with torch.set_grad_enabled(grads):
        e, x, n = BR.slab(o, d, tuple(inp["vol"].shape), float(inp["sr"]), inp.get("t_near"), int(inp.get("jitter_seed", 0)),
                          int(inp.get("ray_base", 0)))
        if grads and kmax_factor != 1.0:
            x.register_hook(lambda g: g * kmax_factor)
        if arg is None:
            out, a = PR.project(vol, o, e, x, d, n, inp.get("max_samples"), mode)
        else:
            a = torch.as_tensor(np.asarray(arg)).long()
            out = PR.sample_at(vol, o, e, x, d, n, a)
        if grads:
            (out * T(inp["grad_out"])).sum().backward()
    N = lambda t: t.detach().double().numpy()
    res = dict(out=N(out), arg=None if a is None else a.numpy().astype(np.int64), n=n.numpy().astype(np.int64), entry=N(e),
               exit=N(x))
    if grads:
        z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else N(t.grad)
        res.update(d_origin=z(o), d_dir=z(d), dvol=z(vol))
    return res


def on_buffers(vol, origins, dirs, entry, exit_, n, grad_out, max_samples, mode, dtype, arg=None):
    """out and d_vol of the projection on given ray buffers (the kernels' own: n, the entry, the exit, and for the MIP the
    kernel's own argmax are inputs here, not recomputed) -> out (P,), dvol, numpy float64."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    v = T(vol).requires_grad_(True)
    bufs = (T(origins), T(entry), T(exit_), T(dirs), torch.as_tensor(np.asarray(n)).long())
    if mode == "sum":
        out, _ = PR.project(v, *bufs, max_samples, mode)
    else:
        out = PR.sample_at(v, *bufs, torch.as_tensor(np.asarray(arg)).long())
    (out * T(grad_out)).sum().backward()
    return out.detach().double().numpy(), v.grad.double().numpy()


def d8_tolerance(ref64, ref32):
    """The project's D8 rule: max(3 err32, 1e-5 max(scale, 1)) with err32 the float32 transliteration's own error -> tol, err32,
    scale."""
    err32 = float(np.abs(ref32 - ref64).max())
    scale = float(np.abs(ref64).max())
    return max(3.0 * err32, 1e-5 * max(scale, 1.0)), err32, scale


def d8_check(got, ref64, ref32, what):
    tol, err32, scale = d8_tolerance(ref64, ref32)
    err = float(np.abs(got - ref64).max())
    print("proj_bundle", what, "err %.3g tol %.3g err32 %.3g scale %.3g" % (err, tol, err32, scale))
    assert np.isfinite(got).all() and err <= tol, (what, err, tol, err32, scale)


def agree(ref, ref32, mode, n_kernel=None, arg_kernel=None):
    """The rays whose n (and, for the MIP, argmax) float32 and float64 agree on -- and the kernel, where given -- and the live
    rays (n > 1 in float64), (P,) bool each."""
    same = ref["n"] == ref32["n"]
    if n_kernel is not None:
        same &= np.asarray(n_kernel).astype(np.int64) == ref["n"]
    if mode == "max":
        same &= ref["arg"] == ref32["arg"]
        if arg_kernel is not None:
            same &= np.asarray(arg_kernel).astype(np.int64) == ref["arg"]
    return same, ref["n"] > 1


# ---- the cases of the float64 comparisons ------------------------------------------------------------------------------------------

SHAPES = {"sr1": ((14, 12, 16), 1.0), "sr2": ((12, 14, 12), 2.0)}


def inputs(bundle, vshape, sr, max_samples=None, dtype=torch.float32, seed=8, rays=None):
    """A random volume in [0, 1) (rounded to what the kernels read in `dtype`) under a bundle of bundle_reference.BUNDLES with
    its t_near and jitter seed, and a random upstream gradient per ray."""
    make, t_near, jseed = BR.BUNDLES[bundle]
    o, d = make() if rays is None else rays
    o, d = F32(o), F32(d)
    g = torch.Generator().manual_seed(seed)
    vol = torch.rand(tuple(vshape), generator=g).to(dtype).double().numpy()
    inp = dict(vol=vol, origins=o, dirs=d, grad_out=F32(np.random.RandomState(o.shape[0]).standard_normal(o.shape[0])), sr=sr,
               max_samples=max_samples, jitter_seed=jseed, ray_base=RAY_BASE)
    if t_near is not None:
        inp["t_near"] = t_near
    return inp


# ---- which path the windowed SUM backward takes (a model of its decisions only, to choose test cases) ----------------------------

KERNEL_SOURCE = os.path.join(os.path.dirname(HERE), "differender_amd", "csrc", "projection_bundle.hip")
GroupPlan = collections.namedtuple("GroupPlan", "lds_full lds_halved fall_through dead_groups live_groups")


def window_constants():
    """PBW_GROUP, PBW_BOX, PBW_WIN_VOX, PBW_MIN_VOX as projection_bundle.hip defines them today."""
    text = open(KERNEL_SOURCE).read()
    out = {}
    for name in ("PBW_GROUP", "PBW_BOX", "PBW_WIN_VOX", "PBW_MIN_VOX"):
        m = re.search(r"constexpr\s+(?:int|float)\s+%s\s*=\s*([0-9.]+)f?\s*;" % name, text)
        assert m, name
        out[name] = float(m.group(1))
    return out


def group_plan(origins, entry, exit_, dirs, n, vshape, max_samples=None):
    """project_bundle_bwd_window_kernel's choice of path for origins, dirs (P, 3) and the ray buffers entry, exit_, n (P,),
    anything numpy can read: proj_reference.window_plan's float32 model with a group of PBW_GROUP consecutive rays in the tile's
    place, each ray with its own origin, and the kernel's one departure -- a group whose box does not fit at the shallowest
    window leaves the walk (every ray with samples is taken as live). Returns GroupPlan: windows that went to LDS at the first
    depth, to LDS at a halved depth; groups that fell through to global atomics; groups without a live ray; groups with one."""
    f32 = np.float32
    K = window_constants()
    G, BOX = int(K["PBW_GROUP"]), int(K["PBW_BOX"])
    origins, dirs = np.asarray(origins, dtype=f32).reshape(-1, 3), np.asarray(dirs, dtype=f32).reshape(-1, 3)
    entry, exit_ = np.asarray(entry, dtype=f32).reshape(-1), np.asarray(exit_, dtype=f32).reshape(-1)
    n = np.asarray(n).astype(np.int64).reshape(-1)
    S = (1 << 31) - 1 if max_samples is None else int(max_samples)
    vox = f32(2.0) / f32(max(vshape) - 1)
    win_t0, win_tmin = f32(K["PBW_WIN_VOX"]) * vox, f32(K["PBW_MIN_VOX"]) * vox
    full = halved = fell = dead = alive = 0
    for g0 in range(0, n.shape[0], G):
        sl = slice(g0, g0 + G)
        nn = n[sl]
        keep = nn > 1
        if not keep.any():
            dead += 1
            continue
        alive += 1
        nn = nn[keep]
        en, ex, rr, oo = entry[sl][keep], exit_[sl][keep], dirs[sl][keep], origins[sl][keep]
        m = np.minimum(nn, S)
        t0 = en + f32(0.5) * (ex - en) / nn.astype(f32)
        s_per_t = (nn - 1).astype(f32) / (ex - t0)
        tlo, thi = t0.min(), ex.max()
        s_cur = np.zeros_like(nn)
        tw0, d = tlo, win_t0
        while True:
            tw1 = f32(tw0 + d)
            last = (not tw1 < thi) or (not tw1 > tw0)
            s_end = m.copy()
            if not last:
                k = np.minimum(np.maximum((tw1 - t0) * s_per_t, f32(0.0)), m.astype(f32))
                s_end = np.maximum(s_cur, np.ceil(k).astype(np.int64))
            act = s_cur < s_end
            nvox = 0
            if act.any():
                a = (oo[act].T, t0[act], ex[act], rr[act], nn[act])   # (_cells32 reads cam[axis]: one row per axis)
                lo0, hi0 = PR._cells32(*a, s_cur[act], vshape)
                lo1, hi1 = PR._cells32(*a, s_end[act] - 1, vshape)
                ext = np.maximum(hi0, hi1).max(0) - np.minimum(lo0, lo1).min(0) + 1
                nvox = int(ext[0]) * int(ext[1]) * int(ext[2])
            if nvox > BOX and d > win_tmin:
                d = f32(d * f32(0.5))
                continue
            if nvox > BOX:
                fell += 1
                break
            if nvox > 0:
                if d == win_t0:
                    full += 1
                else:
                    halved += 1
            s_cur, tw0 = s_end, tw1
            if last:
                break
    return GroupPlan(full, halved, fell, dead, alive)


# ---- the windowed / plain SUM backward cases ---------------------------------------------------------------------------------------

def _ortho(view, dist, extent, WH, tiled=True):
    """orthographic_rays along `view` from `dist` off the centre, flattened in tile order."""
    import differender_amd.bundle as B
    view = np.asarray(view, np.float64)
    view = view / np.linalg.norm(view)
    up = [0.0, 1.0, 0.0] if abs(view[1]) < 0.9 else [1.0, 0.0, 0.0]
    o, d = B.orthographic_rays(torch.from_numpy(-dist * view), torch.zeros(3, dtype=torch.float64),
                               torch.tensor(up, dtype=torch.float64), extent, WH)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    if tiled:
        perm = B.tile_order((WH[1], WH[0]))
        o, d = o[perm], d[perm]
    return o.numpy().copy(), d.numpy().copy()


def _missing(P=256):
    """P rays that all miss the box: origins on the plane x = 3 running along +y."""
    rng = np.random.RandomState(17)
    o = np.stack([np.full(P, 3.0), rng.uniform(-0.5, 0.5, P), rng.uniform(-0.5, 0.5, P)], 1)
    return o, np.tile(np.array([0.0, 1.0, 0.0]), (P, 1))


def _cat(*bundles):
    return tuple(np.concatenate(parts, 0) for parts in zip(*bundles))


# name: rays, volume (field order), the user's (1, D, H, W) layout?, rate, jitter seed, the paths the case is there for
WINDOW_CASES = {
    "ortho_tiled_full": dict(rays=lambda: _ortho([0.0, 0.0, -1.0], 2.8, 1.2, (32, 32)), vshape=(48, 48, 48), user_layout=False,
                             sr=1.0, seed=0, paths=("lds_full",)),
    "oblique_user_halved": dict(rays=lambda: _ortho([0.45, -0.35, -0.82], 2.6, 1.6, (32, 32)), vshape=(40, 44, 36),
                                user_layout=True, sr=1.5, seed=123, paths=("lds_halved",)),
    "random_300_fall_through": dict(rays=lambda: BR.random_bundle(300), vshape=(64, 64, 64), user_layout=False, sr=1.0, seed=0,
                                    paths=("fall_through",)),
    "missing_group": dict(rays=lambda: _cat(_missing(256), _ortho([0.0, 0.0, -1.0], 2.8, 0.6, (8, 8), tiled=False)),
                          vshape=(32, 32, 32), user_layout=False, sr=1.0, seed=0, paths=("dead_groups", "lds_full")),
}


def window_case(name):
    """-> origins, dirs (P, 3) float32-representable float64 numpy, and the case."""
    case = WINDOW_CASES[name]
    o, d = case["rays"]()
    return F32(o), F32(d), case


def slab32(o, d, vshape, sr, t_near=None, jitter_seed=0, ray_base=0):
    """bundle_reference.slab in float32 -> entry, exit, n as numpy: what dr_bundle_setup writes, up to roundings."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    e, x, n = BR.slab(T(o), T(d), tuple(vshape), sr, t_near, jitter_seed, ray_base)
    return e.numpy(), x.numpy(), n.numpy()
