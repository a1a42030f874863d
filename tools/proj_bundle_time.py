#!/usr/bin/env python3
"""The bundle projections beside the image projections, on the same rays, in the same process: SUM forward +
d_vol of the --img x --img rays of one pinhole view on a --vol^3 f32 volume at rate 1,
  image_auto / image_baseline        project_fwd + project_bwd (the windowed / the plain backward)
  tile_auto / tile_baseline          project_bundle_fwd + project_bundle_bwd, the rays in bundle.tile_order
  random_auto / random_baseline      the same rays in a random permutation
Every configuration is timed as one unit with device events: --warmup untimed calls of every configuration first, then --reps
timed repetitions, the configurations in turn so that a drift of the device meets all alike; the median, minimum and maximum
are kept, and the spread of a configuration is (max - min) / median. The backward times include the zeroing of d_vol (the
wrappers allocate it), for all alike. One JSON line, appended to --out. GPU only."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import in_circles, synth_volume_torch  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from differender_amd.bundle import tile_order  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proj_bundle_time.jsonl"),
                    help="append the JSON line to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/proj_bundle_time.py needs a ROCm device"
    dev = torch.device("cuda")
    nv, ni = args.vol, args.img
    vol = synth_volume_torch(nv, dev)
    cam = torch.tensor([in_circles(1.7)], dtype=torch.float32, device=dev)
    e, x, r, n = F.ray_setup(cam, (ni, ni), vol.shape, 1.0)
    g = torch.randn((1, ni, ni), generator=torch.Generator().manual_seed(0)).to(dev)
    flat = lambda t: t.reshape(ni * ni, *t.shape[3:])
    orders = {"tile": tile_order((ni, ni)).to(dev), "random": torch.randperm(ni * ni, generator=torch.Generator().manual_seed(1)).to(dev)}
    fns, checks = {}, {}
    for variant, vname in ((N.DR_VARIANT_AUTO, "auto"), (N.DR_VARIANT_BASELINE, "baseline")):
        def image(variant=variant):
            F.project_fwd(vol, cam, e, x, r, n, None, "sum")
            return F.project_bwd(vol, cam, e, x, r, n, g, None, "sum", variant=variant)
        fns["image_" + vname] = image
        for oname, perm in orders.items():
            o = cam.expand(ni * ni, 3)[perm].contiguous()
            bufs = tuple(flat(t)[perm].contiguous() for t in (r, e, x, n))
            gp = flat(g)[perm].contiguous()

            def bundle(variant=variant, o=o, bufs=bufs, gp=gp):
                F.project_bundle_fwd(vol, o, *bufs, None, "sum")
                return F.project_bundle_bwd(vol, o, *bufs, gp, None, "sum", variant=variant)
            fns[f"{oname}_{vname}"] = bundle
    want = fns["image_baseline"]()
    scale = float(want.abs().max())
    for k, fn in fns.items():   # the same gradient from every configuration (float atomics reorder)
        checks[k] = float((fn() - want).abs().max()) / scale
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            runs[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in runs.items()}
    rec = {"config": f"{nv}^3 f32, rate 1, {ni}x{ni} rays of one pinhole view, SUM fwd + d_vol, ms, device events, median of "
                     f"{args.reps} after {args.warmup} warm-ups, alternating",
           "device": torch.cuda.get_device_name(0),
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(min(v), 4) for k, v in runs.items()},
           "max_ms": {k: round(max(v), 4) for k, v in runs.items()},
           "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in runs.items()},
           "d_vol_max_diff_over_scale": {k: float("%.3g" % v) for k, v in checks.items()}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
