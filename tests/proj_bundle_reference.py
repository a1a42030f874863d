"""Float64 / float32 reference of the projections of a ray bundle: `bundle_reference.slab` followed by
`proj_reference.project` with one origin per ray in the camera's place, differentiated by torch.autograd with the branches
frozen (n, the jitter draw, the slab faces, the t_near clamp, the cells, the argmax). Nothing is derived by hand. For the MIP at
a given argmax: `proj_reference.sample_at`.

Beside the program: group_plan (which path the windowed SUM backward takes per group of 256 consecutive rays: a float32 model of
its decisions, not of its arithmetic, like proj_reference.window_plan) and group_trace (the same walk group by group: where a
group fell through and with how many samples taken, whether a window found one lane finished beside one not begun), and the
cases of tests/test_gpu_proj_bundle.py and tests/test_gpu_proj_bundle_edges.py, which tests/test_proj_bundle.py checks on the
CPU.
"""
import collections
import functools
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


# One group's walk: windows that went to LDS at the first depth and at a halved depth; whether the group fell through to global
# atomics, and the samples its lanes had already taken at that moment (s_cur summed over the lanes); whether some window the
# group took had a live lane that had not begun (s_end == 0) beside a live lane that had finished (s_cur == m). None: no live ray.
GroupTrace = collections.namedtuple("GroupTrace", "lds_full lds_halved fell s_cur_at_fall staggered")


def group_plan(origins, entry, exit_, dirs, n, vshape, max_samples=None, live=None):
    """project_bundle_bwd_window_kernel's choice of path for origins, dirs (P, 3) and the ray buffers entry, exit_, n (P,),
    anything numpy can read: proj_reference.window_plan's float32 model with a group of PBW_GROUP consecutive rays in the tile's
    place, each ray with its own origin, and the kernel's one departure -- a group whose box does not fit at the shallowest
    window leaves the walk (every ray with samples is taken as live). Returns GroupPlan: windows that went to LDS at the first
    depth, to LDS at a halved depth; groups that fell through to global atomics; groups without a live ray; groups with one.
    live (P,) bool: the rays whose g D is neither 0 nor NaN, where the caller knows (the others hold no lane of the walk)."""
    trace = group_trace(origins, entry, exit_, dirs, n, vshape, max_samples, live)
    walked = [t for t in trace if t is not None]
    return GroupPlan(sum(t.lds_full for t in walked), sum(t.lds_halved for t in walked), sum(t.fell for t in walked),
                     len(trace) - len(walked), len(walked))


def group_trace(origins, entry, exit_, dirs, n, vshape, max_samples=None, live=None):
    """group_plan's walk, group by group -> a list with one GroupTrace per group of PBW_GROUP consecutive rays (None for a group
    without a live ray: the kernel's uniform early return)."""
    f32 = np.float32
    K = window_constants()
    G, BOX = int(K["PBW_GROUP"]), int(K["PBW_BOX"])
    origins, dirs = np.asarray(origins, dtype=f32).reshape(-1, 3), np.asarray(dirs, dtype=f32).reshape(-1, 3)
    entry, exit_ = np.asarray(entry, dtype=f32).reshape(-1), np.asarray(exit_, dtype=f32).reshape(-1)
    n = np.asarray(n).astype(np.int64).reshape(-1)
    S = (1 << 31) - 1 if max_samples is None else int(max_samples)
    vox = f32(2.0) / f32(max(vshape) - 1)
    win_t0, win_tmin = f32(K["PBW_WIN_VOX"]) * vox, f32(K["PBW_MIN_VOX"]) * vox
    live = np.ones(n.shape, bool) if live is None else np.asarray(live, bool).reshape(-1)
    trace = []
    for g0 in range(0, n.shape[0], G):
        sl = slice(g0, g0 + G)
        nn = n[sl]
        keep = (nn > 1) & live[sl]
        if not keep.any():
            trace.append(None)
            continue
        full = halved = s_fall = 0
        fell = staggered = False
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
                fell, s_fall = True, int(s_cur.sum())
                break
            if nvox > 0:
                if d == win_t0:
                    full += 1
                else:
                    halved += 1
            staggered |= bool((s_end == 0).any() and (s_cur == m).any())
            s_cur, tw0 = s_end, tw1
            if last:
                break
        trace.append(GroupTrace(full, halved, fell, s_fall, staggered))
    return trace


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


# ---- the cases of tests/test_gpu_proj_bundle_edges.py: the windowed kernel's paths past one ray group, against float64 ---------------

# what a case can declare of its groups' walks (GroupTrace): each name a predicate of the trace, held on the CPU for the float32
# slab and on the GPU for the kernel's own buffers before anything is compared
PATHS = {
    "lds_full": lambda tr: any(t.lds_full for t in tr if t),
    "lds_halved": lambda tr: any(t.lds_halved for t in tr if t),
    "no_halving": lambda tr: not any(t.lds_halved for t in tr if t),
    "fall_through": lambda tr: any(t.fell for t in tr if t),
    "no_fall_through": lambda tr: not any(t.fell for t in tr if t),
    # every live group took LDS windows, at the first and at halved depths, and then left with samples already taken
    "every_group_fell_with_s_cur_above_0": lambda tr: all(t.fell and t.s_cur_at_fall > 0 and t.lds_full and t.lds_halved
                                                          for t in tr if t) and any(tr),
    "one_window_per_group": lambda tr: all(t.lds_full + t.lds_halved == 1 and not t.fell for t in tr if t) and any(tr),
    "staggered": lambda tr: any(t.staggered for t in tr if t),
    "dead_groups": lambda tr: any(t is None for t in tr),
}
CONE = dict(source=(0.0, 0.0, -1.3), det_center=(0.0, 0.0, -0.3), det_u=(0.03, 0.0, 0.0), det_v=(0.0, 0.03, 0.0), det=(32, 32))
# the same cone on a 16 x 16 detector, for the source gradient through the module
CONE_SMALL = dict(CONE, det_u=(0.06, 0.0, 0.0), det_v=(0.0, 0.06, 0.0), det=(16, 16))
NAN_LANE = 100
STAGGERED_CLIP = 130   # clips the rays from outside (n = 163) and none of those from inside (n <= 123)


def cone_rays(cone, source=None, normalise=True):
    """cone_beam_rays of `cone` in tile_order, flattened -> origins, dirs (P, 3) torch (float64, or `source`'s dtype, device and
    graph where a source tensor is given); normalise: the directions normalised once more, by RayBundleProjector.forward's
    own statement (what the module hands its kernels when it is given these rays with normalise=False)."""
    import differender_amd.bundle as B
    src = torch.tensor(cone["source"], dtype=torch.float64) if source is None else source
    o, d = B.cone_beam_rays(src, cone["det_center"], cone["det_u"], cone["det_v"], cone["det"])
    perm = B.tile_order(cone["det"])
    o, d = o.reshape(-1, 3)[perm], d.reshape(-1, 3)[perm]
    return o, d / torch.sqrt((d * d).sum(-1, keepdim=True)) if normalise else d


SOURCE_TORCH_SEED = 1234


def module_jitter_seed():
    """The jitter seed RayBundleProjector draws in a forward that follows torch.manual_seed(SOURCE_TORCH_SEED) (the caller's
    generator is left as it was)."""
    from differender_amd import functional as F
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(SOURCE_TORCH_SEED)
        return F.new_jitter_seed()


def source_gradient(cone, inp, mode, dtype, grad_out=None, arg=None):
    """`run`'s program behind cone_beam_rays, all of it in `dtype` with the source as the one leaf: inp gives vol, sr,
    max_samples, jitter_seed, ray_base. -> out, arg, n and, where grad_out (P,) is given, d_source (3,) of sum(out grad_out)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    src = T(F32(cone["source"])).requires_grad_(True)
    o, d = cone_rays(cone, src)
    vol = T(inp["vol"])
    e, x, n = BR.slab(o, d, tuple(inp["vol"].shape), float(inp["sr"]), inp.get("t_near"), int(inp.get("jitter_seed", 0)),
                      int(inp.get("ray_base", 0)))
    if arg is None:
        out, a = PR.project(vol, o, e, x, d, n, inp.get("max_samples"), mode)
    else:
        a = torch.as_tensor(np.asarray(arg)).long()
        out = PR.sample_at(vol, o, e, x, d, n, a)
    res = dict(out=out.detach().double().numpy(), arg=None if a is None else a.numpy().astype(np.int64),
               n=n.numpy().astype(np.int64))
    if grad_out is not None:
        (out * T(grad_out)).sum().backward()
        res["d_source"] = src.grad.double().numpy()
    return res


# ---- the ray gradients' own edge cases --------------------------------------------------------------------------------------------

CLIPS = (1, 5, "all")   # max_samples of the clipped ray gradients; "all": the largest n, which clips nothing


def clip(S, *ns):
    return int(max(int(np.asarray(n).max()) for n in ns)) if S == "all" else S


AXES = tuple((axis, sign) for axis in range(3) for sign in (1, -1))
AXIS_CLIPS = (None, 9)


def axis_inputs(axis, sign, max_samples=None, P=64):
    """P rays along sign e_axis (the two other components exactly 0) from 2.5 units off the centre, their origins strictly
    inside (-0.9, 0.9) on the two other axes (no 0 * inf in the slab test); SHAPES["sr1"], jitter seed 5."""
    rng = np.random.RandomState(10 * axis + (sign > 0))
    o = rng.uniform(-0.9, 0.9, (P, 3))
    o[:, axis] = -2.5 * sign
    d = np.zeros((P, 3))
    d[:, axis] = float(sign)
    inp = inputs("random", *SHAPES["sr1"], max_samples=max_samples, rays=(o, d))
    inp["jitter_seed"] = 5
    return inp


def _cone():
    o, d = cone_rays(CONE)
    return o.numpy().copy(), d.numpy().copy()


def _staggered(P=256):
    """One group of rays along +z over a footprint of a few voxels. Seven lanes of eight start 1.5 to 5 units in front of the
    box, all with the chord 2: two first-window depths (16 voxels of 48: 0.68 each) lie between the exit of the nearest and
    the entry of the farthest, so some window finds the one finished and the other not begun wherever the windows' grid falls.
    Every eighth starts inside the box; with t_near = 0 it is a shorter ray from its origin."""
    rng = np.random.RandomState(23)
    o = np.stack([rng.uniform(-0.2, 0.2, P), rng.uniform(-0.2, 0.2, P), -1.0 - rng.uniform(1.5, 5.0, P)], 1)
    inside = np.arange(P) % 8 == 3
    o[inside, 2] = rng.uniform(-0.5, 0.2, int(inside.sum()))
    o[np.arange(P) % 16 == 5, 0] = 1.5   # these miss the box
    return o, np.tile(np.array([0.0, 0.0, 1.0]), (P, 1))


def _staggered_grad(g):
    g[np.arange(g.shape[0]) % 16 == 9] = 0.0
    g[NAN_LANE] = np.nan
    return g


def _group_edges(r):
    """Two whole groups of one 16 x 16 orthographic tile each and a last group of r rays of which the last lane alone hits the
    box. The middle group's upstream gradient is zero (_middle_zero): it takes the kernel's uniform early return."""
    tile = _ortho([0.0, 0.0, -1.0], 2.8, 0.6, (16, 16))
    one = tuple(a[137:138] for a in tile)
    return _cat(tile, tile, _missing(r - 1), one) if r > 1 else _cat(tile, tile, one)


def _middle_zero(g):
    g[256:512] = 0.0
    return g


_OBLIQUE = WINDOW_CASES["oblique_user_halved"]
# name: rays, volume (field order), its memory layout (proj_reference.layout_volume), rate, jitter seed, t_near, what is done to
# the random upstream gradient, and per max_samples the paths (PATHS) the case is there for
EDGE_CASES = {
    "cone_spreading": dict(rays=_cone, vshape=(64, 64, 64), layout="z", sr=1.0, seed=5, clips={
        None: ("every_group_fell_with_s_cur_above_0",), 150: ("lds_full", "lds_halved", "no_fall_through"),
        100: ("lds_full", "no_halving", "no_fall_through"), 1: ("one_window_per_group",)}),
    "staggered_depths": dict(rays=_staggered, vshape=(48, 48, 48), layout="z", sr=1.0, seed=5, t_near=0.0, grad=_staggered_grad,
                             clips={None: ("staggered", "no_fall_through"), STAGGERED_CLIP: ("staggered", "no_fall_through")}),
    "layout_z": dict(_OBLIQUE, layout="z", clips={None: ("lds_halved",)}),
    "layout_x": dict(_OBLIQUE, layout="x", clips={None: ("lds_halved",)}),
    "layout_y": dict(_OBLIQUE, layout="y", clips={None: ("lds_halved",)}),
}
for _r in (1, 64, 65):
    EDGE_CASES["group_edges_%d" % _r] = dict(rays=functools.partial(_group_edges, _r), vshape=(32, 32, 32), layout="z", sr=1.0,
                                             seed=5, grad=_middle_zero, clips={None: ("lds_full", "dead_groups", "no_fall_through")})
LAYOUT_STRIDES = {"z": lambda s, V: s == (V[1] * V[2], V[2], 1), "x": lambda s, V: s == (1, V[2] * V[0], V[0]),
                  "y": lambda s, V: s == (V[1], 1, V[0] * V[1])}
MAX_CASES = (("cone_spreading", 150), ("staggered_depths", STAGGERED_CLIP))   # the MIP's d_vol under the clip


def edge_case(name):
    """-> the case with its rays made: origins, dirs (P, 3) float32-representable float64 numpy, grad_out (P,) likewise (NaN
    where the case has a NaN lane), live (P,): the rays whose upstream gradient is neither 0 nor NaN, t_near (or None)."""
    case = dict(EDGE_CASES[name])
    o, d = case["rays"]()
    g = F32(np.random.RandomState(7).standard_normal(o.shape[0]))
    g = case.get("grad", lambda a: a)(g)
    case.update(origins=F32(o), dirs=F32(d), grad_out=g, live=np.isfinite(g) & (g != 0), t_near=case.get("t_near"))
    return case


def check_paths(case, max_samples, trace):
    for path in case["clips"][max_samples]:
        assert PATHS[path](trace), (path, max_samples, trace)


def slab32(o, d, vshape, sr, t_near=None, jitter_seed=0, ray_base=0):
    """bundle_reference.slab in float32 -> entry, exit, n as numpy: what dr_bundle_setup writes, up to roundings."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    e, x, n = BR.slab(T(o), T(d), tuple(vshape), sr, t_near, jitter_seed, ray_base)
    return e.numpy(), x.numpy(), n.numpy()
