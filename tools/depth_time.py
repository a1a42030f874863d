#!/usr/bin/env python3
"""The depth march beside the plain colour march, on the same rays, in the same process:
  base_fwd / base_bwd     march_fwd / march_bwd (volume + TF) with DR_VARIANT_BASELINE
  depth_fwd / depth_bwd   march_depth_fwd / march_depth_bwd (volume + TF)
at 512^3 f32 / 512^2 / one view / R = 256: sampling rate 1, no jitter, bench.py's TF (alpha = 3 / n_max: no early termination)
and volume. Every call is timed on its own with device events: --warmup untimed calls of every configuration first (code
objects loaded, the clocks up), then --reps timed repetitions, the configurations in turn so that a drift of the device meets
all alike; the median, minimum and maximum are kept. One JSON line per shape, appended to --out. The backward times include
the zeroing of their outputs (the wrappers allocate them), for both alike. GPU only."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import bench_tf_torch, in_circles, synth_volume_torch  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512:512:1", help="volume:image:views,...")
    ap.add_argument("--tf-res", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_time.jsonl"),
                    help="append the JSON lines to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/depth_time.py needs a ROCm device"
    assert args.reps >= 20, "at least 20 timed repetitions"
    dev = torch.device("cuda")
    S, R, sr = 1 << 20, args.tf_res, 1.0
    for spec in args.shapes.split(","):
        nv, ni, V = (int(s) for s in spec.split(":"))
        vol = synth_volume_torch(nv, dev)
        tf = bench_tf_torch(R, 3.0 / (2.0 * math.sqrt(3.0) * math.sqrt(3.0) * (nv - 1)), dev)
        cam = torch.tensor([in_circles(1.7 + 0.8 * i) for i in range(V)], dtype=torch.float32, device=dev)
        WH = (ni, ni)
        e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
        g = torch.randn((V, *WH, 4), device=dev) * 1e-3
        base = dict(variant=N.DR_VARIANT_BASELINE, workspace=None)
        out_b, steps_b = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, hints=0, **base)
        out_d, steps_d = F.march_depth_fwd(vol, tf, cam, e, x, r, n, S, sr)
        many = n != 1   # (a single-sample ray is 0 / 0 in the colour march and 0 in the depth march)
        same_alpha = bool(torch.equal(out_b[..., 3][many].view(torch.int32), out_d[..., 3][many].view(torch.int32))) and \
            bool(torch.equal(steps_b[many], steps_d[many]))
        fns = {
            "base_fwd": lambda: F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, hints=0, **base),
            "depth_fwd": lambda: F.march_depth_fwd(vol, tf, cam, e, x, r, n, S, sr),
            "base_bwd": lambda: F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out_b, **base),
            "depth_bwd": lambda: F.march_depth_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out_d),
        }
        for _ in range(args.warmup):   # every configuration the timed calls use
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                runs[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in runs.items()}
        rec = {"shape": [nv, ni, V], "dtype": "f32", "R": R, "sr": sr, "warmup": args.warmup, "reps": args.reps,
               "device": torch.cuda.get_device_name(0), "samples": int(steps_d.sum()),
               "alpha_and_steps_same_bits_as_baseline": same_alpha,
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_ms": {k: round(min(v), 4) for k, v in runs.items()},
               "max_ms": {k: round(max(v), 4) for k, v in runs.items()},
               "depth_fwd_over_base": round(med["depth_fwd"] / med["base_fwd"], 4),
               "depth_bwd_over_base": round(med["depth_bwd"] / med["base_bwd"], 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del fns, vol, out_b, out_d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
