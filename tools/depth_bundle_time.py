#!/usr/bin/env python3
"""The depth march over a ray bundle beside DepthRaycaster's own kernels on the same rays, in the same process:
a 256^3 float32 volume, a 256-texel table and the 512^2 rays of one pinhole view at sampling rate 1, the forward, the backward
(d_vol + d_tf) and the ray / camera gradient, each timed for
  whole_image    march_depth_fwd / _bwd / _bwd_cam on the view (a wave is an 8 x 8 pixel tile): the yardstick
  bundle_tiles   the same rays as a bundle in bundle.tile_order (a wave is an 8 x 8 block of the image)
  bundle_rows    ... in the ray buffers' own row order (a wave is 64 consecutive pixels of one image row)
  bundle_random  ... in a random permutation
Before anything is timed the bundles' moments are checked against the view's, bit for bit. Device events around windows of at
least --min-seconds after a warm-up of every function; --rounds rounds that visit all (case, pass) pairs in turn, so the cases
alternate and share whatever else the device is doing; per pair the median, the minimum, the maximum and (max - min) / median of
the rounds' ms per call. The backward times include the zeroing of d_vol and d_tf (the wrappers allocate them), for all cases
alike.

--ab-lib PATH: the A/B of the d_vol scatter. PATH is a second build of the library (tools/patches/depth_bundle_per_sample.patch
with -DDR_DEPTH_BUNDLE_PER_SAMPLE: eight atomics after every sample); dr_march_depth_bundle_bwd of both libraries is called
through the same raw wrapper on the tile-ordered bundle, at sampling rates 1 and 4, in the same rounds: the passes `bwd_ab`
of the cases run_sums (this library) and per_sample (PATH), with `over_per_sample` in the run_sums lines.
One JSON line per (case, pass, rate), appended to --out. GPU only."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differender.utils import in_circles  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from differender_amd.bundle import tile_order  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402
from tools.rgba_time import timed  # noqa: E402


def raw_bwd(lib, vol, tf, a, S, sr, g, out):
    """dr_march_depth_bundle_bwd of `lib` on freshly zeroed d_vol and d_tf: functional.march_depth_bundle_bwd's call, for a
    library that is not the loaded one."""
    head = F._bundle_head(vol, tf, *a, S, sr)[3]
    d_vol, d_tf = torch.zeros_like(vol), torch.zeros_like(tf)
    rc = lib.dr_march_depth_bundle_bwd(*head, g.data_ptr(), out.data_ptr(), d_vol.data_ptr(), *d_vol.stride(), d_tf.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return d_vol, d_tf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=256)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--ab-lib", default="", help="a per-sample build of the library to time the backward against")
    ap.add_argument("--commit", default="", help="recorded in every line: the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bundle_time.jsonl"),
                    help="append the JSON lines to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/depth_bundle_time.py needs a ROCm device"
    dev = torch.device("cuda")
    S, R = 1 << 20, 256
    v = torch.linspace(0.0, 1.0, R, device=dev)
    tf = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.4 * torch.clamp((v - 0.3) / 0.7, 0.0, 1.0) ** 2], 1).contiguous()
    vol = synthetic_volume(args.vol, dev)[0].permute(2, 0, 1)   # the field view (W, D, H)
    cam = in_circles(1.7).float().to(dev)[None]
    WH = (args.img, args.img)
    P = WH[0] * WH[1]
    torch.manual_seed(0)
    g = torch.randn((1, *WH, 4), device=dev) * 1e-3
    orders = {"bundle_tiles": tile_order(WH).to(dev), "bundle_rows": torch.arange(P, device=dev),
              "bundle_random": torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(dev)}
    other = None
    if args.ab_lib:
        other = ctypes.CDLL(args.ab_lib)
        other.dr_march_depth_bundle_bwd.restype, other.dr_march_depth_bundle_bwd.argtypes = N.SIGNATURES["dr_march_depth_bundle_bwd"]
        other.dr_build_flags.restype = ctypes.c_int
        assert other.dr_build_flags() & N.BUILD_DIAGNOSTIC, "--ab-lib is not a marked what-if build"
        assert not N.lib().dr_build_flags() & N.BUILD_DIAGNOSTIC, "the loaded library is a what-if build itself"
    fns = {}
    for sr in (1.0, 4.0) if other else (1.0,):
        e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
        out0, steps0 = F.march_depth_fwd(vol, tf, cam, e, x, r, n, S, sr)
        if sr == 1.0:
            fns[("whole_image", "fwd", sr)] = lambda e=e, x=x, r=r, n=n: F.march_depth_fwd(vol, tf, cam, e, x, r, n, S, 1.0)
            fns[("whole_image", "bwd", sr)] = lambda e=e, x=x, r=r, n=n, o0=out0: F.march_depth_bwd(vol, tf, cam, e, x, r, n, S, 1.0, g, o0)
            fns[("whole_image", "ray_grad", sr)] = lambda e=e, x=x, r=r, n=n, o0=out0, s0=steps0: F.march_depth_bwd_cam(
                vol, tf, cam, e, x, r, n, s0, S, 1.0, g, o0)
        for name, perm in orders.items():
            if sr != 1.0 and name != "bundle_tiles":
                continue
            o = cam.expand(P, 3)[perm].contiguous()
            d = r.reshape(P, 3)[perm].contiguous()
            gb = g.reshape(P, 4)[perm].contiguous()
            eb, xb, nb = F.bundle_setup(o, d, vol.shape, sr)
            ob, sb = F.march_depth_bundle_fwd(vol, tf, o, d, eb, xb, nb, S, sr)
            # the same rays, the same moments: checked at the size that is timed
            assert torch.equal(ob.view(torch.int32), out0.reshape(P, 4)[perm].view(torch.int32)), name
            assert torch.equal(sb, steps0.reshape(P)[perm]), name
            a = (o, d, eb, xb, nb)
            if sr == 1.0:
                fns[(name, "fwd", sr)] = lambda a=a: F.march_depth_bundle_fwd(vol, tf, *a, S, 1.0)
                fns[(name, "bwd", sr)] = lambda a=a, gb=gb, ob=ob: F.march_depth_bundle_bwd(vol, tf, *a, S, 1.0, gb, ob)
                fns[(name, "ray_grad", sr)] = lambda a=a, gb=gb, ob=ob, sb=sb: F.march_depth_bundle_bwd_rays(vol, tf, *a, sb, S, 1.0, gb, ob)
            if other and name == "bundle_tiles":
                fns[("run_sums", "bwd_ab", sr)] = lambda a=a, gb=gb, ob=ob, sr=sr: raw_bwd(N.lib(), vol, tf, a, S, sr, gb, ob)
                fns[("per_sample", "bwd_ab", sr)] = lambda a=a, gb=gb, ob=ob, sr=sr: raw_bwd(other, vol, tf, a, S, sr, gb, ob)
                # both forms scatter the same gradient: their d_vol agree to the rounding of the sums' order
                dv_a, dt_a = fns[("run_sums", "bwd_ab", sr)]()
                dv_b, dt_b = fns[("per_sample", "bwd_ab", sr)]()
                assert float((dv_a - dv_b).abs().max()) <= 1e-3 * float(dv_b.abs().max()) and float(dv_b.abs().max()) > 0
                assert float((dt_a - dt_b).abs().max()) <= 1e-3 * float(dt_b.abs().max())
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, args.min_seconds))
    for (case, tag, sr), t in ms.items():
        med = statistics.median(t)
        rec = {"vol": args.vol, "img": args.img, "dtype": "f32", "R": R, "sampling_rate": sr, "case": case, "pass": tag,
               "ms_median": med, "ms_min": min(t), "ms_max": max(t), "spread": (max(t) - min(t)) / med, "rounds": len(t)}
        if tag == "bwd_ab":
            rec["over_per_sample"] = med / statistics.median(ms[("per_sample", tag, sr)])
        else:
            rec["over_whole_image"] = med / statistics.median(ms[("whole_image", tag, sr)])
        if args.commit:
            rec["commit"] = args.commit
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
