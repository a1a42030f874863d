#!/usr/bin/env python3
"""Fused MS-SSIM + MSE loss (fused_ms_dssim_mse_loss) against the torch restatement (ms_dssim_mse_loss):
forward + backward of the loss alone at (8, 4, 256, 256) and (1, 4, 512, 512). Warm-up, then device events around --iters
iterations of each; prints one JSON line per (shape, implementation). Runs on the GPU only.
For kernel times run it under `rocprofv3 --kernel-trace --stats` (profiles/msssim_loss_kernel_stats_*.csv, one run per implementation and shape)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.utils import fused_ms_dssim_mse_loss, ms_dssim_mse_loss  # noqa: E402


def step(fn, x, y):
    x.grad = None
    loss = fn(x, y)[0]
    loss.backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--impl", choices=("both", "torch", "fused"), default="both")
    ap.add_argument("--shape", choices=("8x4x256x256", "1x4x512x512"), default=None, help="one shape only (default both)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/msssim_time.py needs a ROCm device"
    dev = torch.device("cuda")
    impls = [(n, f) for n, f in (("torch", ms_dssim_mse_loss), ("fused", fused_ms_dssim_mse_loss)) if args.impl in ("both", n)]
    shapes = ((8, 4, 256, 256), (1, 4, 512, 512))
    for shape in [s for s in shapes if args.shape in (None, "x".join(map(str, s)))]:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
        y = (0.7 * x.detach() + 0.3 * torch.rand(shape, device=dev, generator=g)).clamp(0, 1)
        for name, fn in impls:
            for _ in range(args.warmup):
                step(fn, x, y)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                step(fn, x, y)
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"shape": list(shape), "impl": name, "ms_per_fwd_bwd": e0.elapsed_time(e1) / args.iters}))


if __name__ == "__main__":
    main()
