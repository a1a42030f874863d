#!/usr/bin/env python3
"""Fused 3-D total variation (fused_tv3d_loss) against the torch definition (tv3d): forward + backward of the
regulariser alone at 256^3 and 512^3, float32 and float16, every norm. Device events around windows of at least 0.2 s after a
warm-up; prints one JSON line per configuration with the forward, backward and fused total times, the algorithmic bytes (one
read of the volume for the forward, one read and one f32 write for the backward), the effective TB/s, the share of the
6.3 TB/s achievable HBM rate, and the torch forward + backward time on the same inputs. GPU only.
For kernel times run it under `rocprofv3 --kernel-trace --stats` (profiles/tv_loss_kernel_stats.csv)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd import functional as F  # noqa: E402
from differender_amd.utils import tv3d  # noqa: E402

HBM_TBS = 6.3   # achievable HBM3E rate of an MI355X (float4 copy), TB/s


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
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--dtypes", default="float32,float16")
    ap.add_argument("--norms", default="l1,iso,sq")
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/tv_time.py needs a ROCm device"
    dev = torch.device("cuda")
    for n in (int(s) for s in args.sizes.split(",")):
        for dt in args.dtypes.split(","):
            dtype = getattr(torch, dt)
            g = torch.Generator(device=dev).manual_seed(0)
            vol = torch.rand((1, n, n, n), device=dev, generator=g).to(dtype)
            grad = torch.empty(vol.shape, dtype=torch.float32, device=dev)
            for norm in args.norms.split(","):
                fwd = lambda: F.tv3d_fwd(vol, norm, 1e-2)  # noqa: E731
                bwd = lambda: F.tv3d_bwd(vol, scale=1.0 / vol.numel(), norm=norm, eps=1e-2, out=grad)  # noqa: E731

                def both():
                    fwd(); bwd()
                for f in (fwd, bwd, both):
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                t_f, t_b, t_fb = timed(fwd, args.min_seconds), timed(bwd, args.min_seconds), timed(both, args.min_seconds)
                vb = vol.numel() * vol.element_size()
                bytes_ = 2 * vb + 4 * vol.numel()   # fwd reads vol; bwd reads vol, writes the f32 gradient
                rec = {"shape": list(vol.shape), "dtype": dt, "norm": norm, "fwd_ms": t_f, "bwd_ms": t_b, "fwd_bwd_ms": t_fb,
                       "algo_bytes": bytes_, "bound_ms": bytes_ / (HBM_TBS * 1e9),
                       "eff_TBps": bytes_ / (t_fb * 1e9), "hbm_share": bytes_ / (t_fb * 1e9) / HBM_TBS}
                if not args.no_torch:
                    v = vol.detach().requires_grad_(True)

                    def ref():
                        v.grad = None
                        tv3d(v, norm, 1e-2).backward()
                    for _ in range(2):
                        ref()
                    torch.cuda.synchronize()
                    rec["torch_fwd_bwd_ms"] = timed(ref, args.min_seconds)
                    rec["speedup"] = rec["torch_fwd_bwd_ms"] / t_fb
                    del v
                    torch.cuda.empty_cache()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
