#!/usr/bin/env python3
"""X-ray line-integral and maximum intensity projections: forward, volume backward (SUM windowed and plain, MAX)
and camera backward of both modes, against the 1-D baseline march forward (DR_VARIANT_BASELINE, the kernels of the same
one-lane-per-ray shape) on the same rays, at 256^3 / 256^2 / 8 views and 512^3 / 512^2 / 1 view (synthetic volume, user layout:
x contiguous, sampling rate 1, jittered orbit cameras). Device events around windows of at least --min-seconds after a warm-up;
one JSON line per (shape, pass) with ms per call. For kernel times run it under `rocprofv3 --kernel-trace --stats`. GPU only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def timed(fn, min_s):
    """ms per call: repeat fn in windows until one lasts >= min_s."""
    fn()
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
    ap.add_argument("--min-seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/proj_time.py needs a ROCm device"
    dev = torch.device("cuda")
    for spec in args.shapes.split(","):
        nv, ni, V = (int(t) for t in spec.split(":"))
        vol = synthetic_volume(nv, dev)[0].permute(2, 0, 1)   # (W, D, H) view of the (1, D, H, W) tensor: x contiguous
        cam = torch.stack([in_circles(0.7 * k + 0.3) for k in range(V)]).float().to(dev)
        e, x, r, n = F.ray_setup(cam, (ni, ni), vol.shape, 1.0, 30.0, 0.1, 1234)
        g = torch.randn((V, ni, ni), device=dev)
        _, arg = F.project_fwd(vol, cam, e, x, r, n, None, "max")
        v = torch.linspace(0.0, 1.0, 128, device=dev)
        tf = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.05 * v], 1).contiguous()   # thin: no early termination
        passes = {
            "fwd_sum": lambda: F.project_fwd(vol, cam, e, x, r, n, None, "sum"),
            "fwd_max": lambda: F.project_fwd(vol, cam, e, x, r, n, None, "max"),
            "bwd_sum_windowed": lambda: F.project_bwd(vol, cam, e, x, r, n, g, None, "sum", variant=N.DR_VARIANT_AUTO),
            "bwd_sum_plain": lambda: F.project_bwd(vol, cam, e, x, r, n, g, None, "sum", variant=N.DR_VARIANT_BASELINE),
            "bwd_max": lambda: F.project_bwd(vol, cam, e, x, r, n, g, None, "max", arg),
            "cam_sum": lambda: F.project_bwd_cam(vol, cam, e, x, r, n, g, None, "sum", jitter_seed=1234),
            "cam_max": lambda: F.project_bwd_cam(vol, cam, e, x, r, n, g, None, "max", arg, jitter_seed=1234),
            "base1d_fwd": lambda: F.march_fwd(vol, tf, cam, e, x, r, n, 1 << 20, 1.0, N.DR_MODE_DIFF,
                                              variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0),
            "zeros_dvol": lambda: torch.zeros_like(vol),   # what every volume backward pays for its d_vol allocation
        }
        res = {name: timed(fn, args.min_seconds) for name, fn in passes.items()}
        res["plain_over_windowed"] = res["bwd_sum_plain"] / res["bwd_sum_windowed"]
        print(json.dumps({"volume": nv, "image": ni, "views": V, "samples": int(n.clamp(min=0).sum()),
                          **{k: round(val, 4) for k, val in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
