#!/usr/bin/env python3
"""The RGBA march over a ray bundle beside RaycasterRGBA's own kernels on the same rays, in the same process:
a 256^3 float32 interleaved volume and the 512^2 rays of one pinhole view at sampling rate 1, the forward, the volume backward
and the ray / camera gradient, each timed for
  whole_image    march_rgba_fwd / _bwd / _bwd_cam on the view (a wave is an 8 x 8 pixel tile): the yardstick
  bundle_tiles   the same rays as a bundle in bundle.tile_order (a wave is an 8 x 8 block of the image)
  bundle_rows    ... in the ray buffers' own row order (a wave is 64 consecutive pixels of one image row)
  bundle_random  ... in a random permutation
Before anything is timed the bundles' images are checked against the view's, bit for bit. Device events around windows of at
least --min-seconds after a warm-up of every function; --rounds rounds that visit all twelve (case, pass) pairs in turn, so the
cases alternate and share whatever else the device is doing; per pair the median, the minimum and the maximum of the rounds'
ms per call. The backward times include the zeroing of d_vol (the wrappers allocate it), for all cases alike. One JSON line per
(case, pass), appended to --out. GPU only."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from differender.utils import in_circles  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from differender_amd.bundle import tile_order  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402
from tools.rgba_time import classify, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=256)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--commit", default="", help="recorded in every line: the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_bundle_time.jsonl"),
                    help="append the JSON lines to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/rgba_bundle_time.py needs a ROCm device"
    dev = torch.device("cuda")
    S, R, sr = 1 << 20, 64, 1.0
    v = torch.linspace(0.0, 1.0, R, device=dev)
    tf1 = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.4 * torch.clamp((v - 0.3) / 0.7, 0.0, 1.0) ** 2], 1).contiguous()
    vol = synthetic_volume(args.vol, dev)[0].permute(2, 0, 1)   # the field view (W, D, H)
    vol4 = classify(vol, tf1).permute(3, 0, 1, 2)               # (4, VX, VY, VZ), channel stride 1
    assert vol4.stride(0) == 1
    cam = in_circles(1.7).float().to(dev)[None]
    WH = (args.img, args.img)
    P = WH[0] * WH[1]
    torch.manual_seed(0)
    g = torch.randn((1, *WH, 4), device=dev) * 1e-3
    e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
    out0, steps0 = F.march_rgba_fwd(vol4, cam, e, x, r, n, S, sr)
    fns = {("whole_image", "fwd"): lambda: F.march_rgba_fwd(vol4, cam, e, x, r, n, S, sr),
           ("whole_image", "bwd"): lambda: F.march_rgba_bwd(vol4, cam, e, x, r, n, S, sr, g, out0),
           ("whole_image", "ray_grad"): lambda: F.march_rgba_bwd_cam(vol4, cam, e, x, r, n, steps0, S, sr, g, out0)}
    orders = {"bundle_tiles": tile_order(WH).to(dev), "bundle_rows": torch.arange(P, device=dev),
              "bundle_random": torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(dev)}
    for name, perm in orders.items():
        o = cam.expand(P, 3)[perm].contiguous()
        d = r.reshape(P, 3)[perm].contiguous()
        gb = g.reshape(P, 4)[perm].contiguous()
        eb, xb, nb = F.bundle_setup(o, d, vol.shape, sr)
        ob, sb = F.march_rgba_bundle_fwd(vol4, o, d, eb, xb, nb, S, sr)
        # the same rays, the same image: checked at the size that is timed
        assert torch.equal(ob.view(torch.int32), out0.reshape(P, 4)[perm].view(torch.int32)), name
        assert torch.equal(sb, steps0.reshape(P)[perm]), name
        a = (o, d, eb, xb, nb)
        fns[(name, "fwd")] = lambda a=a: F.march_rgba_bundle_fwd(vol4, *a, S, sr)
        fns[(name, "bwd")] = lambda a=a, gb=gb, ob=ob: F.march_rgba_bundle_bwd(vol4, *a, S, sr, gb, ob)
        fns[(name, "ray_grad")] = lambda a=a, gb=gb, ob=ob, sb=sb: F.march_rgba_bundle_bwd_rays(vol4, *a, sb, S, sr, gb, ob)
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, args.min_seconds))
    for (case, tag), t in ms.items():
        rec = {"vol": args.vol, "img": args.img, "dtype": "f32", "layout": "interleaved", "sampling_rate": sr, "case": case,
               "pass": tag, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "rounds": len(t),
               "over_whole_image": statistics.median(t) / statistics.median(ms[("whole_image", tag)])}
        if args.commit:
            rec["commit"] = args.commit
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
