#!/usr/bin/env python3
"""The lit march beside the plain 1-D kernels it is modelled on, on the same rays, in the same process:
  base_fwd / base_bwd   march_fwd / march_bwd (volume + TF) with DR_VARIANT_BASELINE
  lit_fwd / lit_bwd     march_lit_fwd / march_lit_bwd (volume + TF, no d_light) with the reference's lighting (default_light)
  lit_bwd_light         ... with d_light as well; lit_bwd_light_only: d_light alone (no scatter, no d_tf)
  lit_fwd_sh31.5 / lit_bwd_sh31.5 / lit_bwd_light_sh31.5   the same three with shininess 31.5: the general (double-precision) power
at 256^3 / 256^2 / 8 views and 512^3 / 512^2 / 1 view: float32, sampling rate 1, no jitter, bench.py's TF (alpha = 3 / n_max: no
early termination) and volume. Device events around windows of at least --min-seconds after a warm-up of every configuration,
the configurations timed in turn --rounds times (the minimum and the spread are kept); one JSON line per shape, appended to
--out. The backward times include the zeroing of their outputs (the wrappers allocate them), for all alike. GPU only."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import bench_tf_torch, in_circles, synth_volume_torch  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402


def timed(fn, min_s):
    """ms per call: repeat fn in windows until one lasts >= min_s."""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1000 * min_s:
            return ms / n
        n = max(n * 2, int(n * 1000 * min_s / max(ms, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:256:8,512:512:1", help="volume:image:views,...")
    ap.add_argument("--tf-res", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lit_time.jsonl"),
                    help="append the JSON lines to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/lit_time.py needs a ROCm device"
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
        light = F.default_light(cam)
        light_g = light.clone()
        light_g[:, 9] = 31.5
        base = dict(variant=N.DR_VARIANT_BASELINE, workspace=None)
        out_b, _ = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, hints=0, **base)
        out_l, _ = F.march_lit_fwd(vol, tf, cam, light, e, x, r, n, S, sr)
        out_g, _ = F.march_lit_fwd(vol, tf, cam, light_g, e, x, r, n, S, sr)
        same_bits = bool(torch.equal(out_b.view(torch.int32), out_l.view(torch.int32)))
        lit_bwd = lambda lt, out, **kw: F.march_lit_bwd(vol, tf, cam, lt, e, x, r, n, S, sr, g, out, **kw)
        fns = {
            "base_fwd": lambda: F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, hints=0, **base),
            "lit_fwd": lambda: F.march_lit_fwd(vol, tf, cam, light, e, x, r, n, S, sr),
            "lit_fwd_sh31.5": lambda: F.march_lit_fwd(vol, tf, cam, light_g, e, x, r, n, S, sr),
            "base_bwd": lambda: F.march_bwd(vol, tf, cam, e, x, r, n, S, sr, g, out_b, **base),
            "lit_bwd": lambda: lit_bwd(light, out_l, want_light=False),
            "lit_bwd_light": lambda: lit_bwd(light, out_l),
            "lit_bwd_light_only": lambda: lit_bwd(light, out_l, want_vol=False, want_tf=False),
            "lit_bwd_sh31.5": lambda: lit_bwd(light_g, out_g, want_light=False),
            "lit_bwd_light_sh31.5": lambda: lit_bwd(light_g, out_g),
        }
        for fn in fns.values():   # warm up every configuration the windows use
            fn(); fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in fns}
        for _ in range(args.rounds):   # in turn, so that a drift of the device meets every configuration alike
            for k, fn in fns.items():
                runs[k].append(timed(fn, args.min_seconds))
        ms = {k: min(v) for k, v in runs.items()}
        rec = {"shape": [nv, ni, V], "dtype": "f32", "R": R, "sr": sr, "rounds": args.rounds,
               "default_light_same_bits_as_baseline": same_bits,
               "ms": {k: round(v, 4) for k, v in ms.items()},
               "spread": {k: round(max(v) / min(v) - 1.0, 4) for k, v in runs.items()},
               "lit_fwd_over_base": round(ms["lit_fwd"] / ms["base_fwd"], 4),
               "lit_bwd_over_base": round(ms["lit_bwd"] / ms["base_bwd"], 4),
               "d_light_cost": round(ms["lit_bwd_light"] / ms["lit_bwd"], 4),
               "general_power_fwd": round(ms["lit_fwd_sh31.5"] / ms["lit_fwd"], 4),
               "general_power_bwd": round(ms["lit_bwd_sh31.5"] / ms["lit_bwd"], 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del fns, vol, out_b, out_l, out_g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
