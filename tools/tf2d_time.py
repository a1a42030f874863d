#!/usr/bin/env python3
"""2-D transfer-function march against the 1-D march on the same inputs, in the same process: the forward
(DIFF), the forward (NONDIFF) at sampling rate 8, the TF-only, the volume + TF and the volume-only backward, each timed for
  tf2d      march_tf2d_fwd / _bwd with a (RV, RG) table whose colour changes along u (its alphas are the 1-D TF's)
  base1d    march_fwd / _bwd with DR_VARIANT_BASELINE and the 1-D TF of RV entries (the kernels of the same shape)
  auto1d    march_fwd / _bwd on the default path (DR_VARIANT_AUTO, brick-centric where it applies; tape for the TF-only backward)
at 256^3 / 256^2 / 8 views (the demo's shape) and 512^3 / 512^2 / 1 view, for a 64 x 32 and a 128 x 32 table. Device events
around windows of at least --min-seconds after a warm-up; one JSON line per (shape, pass) with the three times and the ratios tf2d / base1d, tf2d / auto1d.
For kernel times run it under `rocprofv3 --kernel-trace --stats --output-format csv` (profiles/tf2d_kernel_stats.csv). GPU only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from differender_amd.tf2d import gradient_scale  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


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


def tables(RV, RG, dev):
    """The demo-like 1-D TF of RV entries (alpha ramp over the upper values) and a 2-D table with the same alphas (so both
    marches composite and terminate alike) whose colour changes with u."""
    v = torch.linspace(0.0, 1.0, RV, device=dev)
    tf1 = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.4 * torch.clamp((v - 0.3) / 0.7, 0.0, 1.0) ** 2], 1).contiguous()
    u = torch.linspace(0.0, 1.0, RG, device=dev)
    tf2 = tf1[:, None, :].repeat(1, RG, 1)
    tf2[..., 0] = tf2[..., 0] * (0.5 + 0.5 * u[None, :])
    return tf1, tf2.clamp(0.0, 1.0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:256:8,512:512:1", help="volume:image:views,...")
    ap.add_argument("--tfs", default="64x32,128x32", help="RVxRG,...: P = 2048 keeps d_tf2d in LDS (tier 2), 4096 does not (tier 1)")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/tf2d_time.py needs a ROCm device"
    dev = torch.device("cuda")
    S = 1 << 20
    for spec, tfspec in [(a, b) for a in args.shapes.split(",") for b in args.tfs.split(",")]:
        RV, RG = (int(v) for v in tfspec.split("x"))
        nv, ni, V = (int(s) for s in spec.split(":"))
        vol = synthetic_volume(nv, dev)[0].permute(2, 0, 1)   # (1,D,H,W) -> the field view (W,D,H), as Raycaster hands it over
        g_scale = gradient_scale(vol, q=0.99)
        tf1, tf2 = tables(RV, RG, dev)
        cam = torch.stack([in_circles(1.7 + 0.8 * i).float() for i in range(V)]).to(dev)
        WH = (ni, ni)
        g = torch.randn((V, *WH, 4), device=dev) * 1e-3
        for sr, mode, tag in ((1.0, N.DR_MODE_DIFF, "fwd_diff"), (8.0, N.DR_MODE_NONDIFF, "fwd_nondiff_sr8")):
            e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
            ws = F.alloc_workspace(V, WH, vol.shape, RV, dev)
            fns = {
                "tf2d": lambda: F.march_tf2d_fwd(vol, tf2, cam, e, x, r, n, S, sr, g_scale, mode=mode),
                "base1d": lambda: F.march_fwd(vol, tf1, cam, e, x, r, n, S, sr, mode=mode, variant=N.DR_VARIANT_BASELINE,
                                              workspace=None, hints=0),
                "auto1d": lambda: F.march_fwd(vol, tf1, cam, e, x, r, n, S, sr, mode=mode, workspace=ws, hints=0),
            }
            for k, fn in fns.items():
                fn(); fn()
            torch.cuda.synchronize()
            rec = {"shape": [nv, ni, V], "tf": [RV, RG], "pass": tag}
            for k, fn in fns.items():
                rec[k + "_ms"] = timed(fn, args.min_seconds)
            rec["tf2d_over_base1d"] = rec["tf2d_ms"] / rec["base1d_ms"]
            rec["tf2d_over_auto1d"] = rec["tf2d_ms"] / rec["auto1d_ms"]
            print(json.dumps(rec), flush=True)
            del ws
        # backward passes at sampling rate 1 (DIFF)
        e, x, r, n = F.ray_setup(cam, WH, vol.shape, 1.0)
        out2, _ = F.march_tf2d_fwd(vol, tf2, cam, e, x, r, n, S, 1.0, g_scale)
        outb, _ = F.march_fwd(vol, tf1, cam, e, x, r, n, S, 1.0, variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0)
        ws = F.alloc_workspace(V, WH, vol.shape, RV, dev)
        wst = F.alloc_workspace(V, WH, vol.shape, RV, dev, tape=(S, 1.0))
        outa, _ = F.march_fwd(vol, tf1, cam, e, x, r, n, S, 1.0, workspace=ws, hints=0)
        outt, _ = F.march_fwd(vol, tf1, cam, e, x, r, n, S, 1.0, workspace=wst, hints=0, tape=True) if wst is not None else (None, None)
        for want_vol, want_tf, tag in ((False, True, "bwd_tf_only"), (True, True, "bwd_vol_tf"), (True, False, "bwd_vol_only")):
            fns = {
                "tf2d": lambda: F.march_tf2d_bwd(vol, tf2, cam, e, x, r, n, S, 1.0, g_scale, g, out2, want_vol=want_vol,
                                                 want_tf=want_tf),
                "base1d": lambda: F.march_bwd(vol, tf1, cam, e, x, r, n, S, 1.0, g, outb, want_vol=want_vol, want_tf=want_tf,
                                              variant=N.DR_VARIANT_BASELINE, workspace=None),
            }
            if want_vol or wst is None:
                fns["auto1d"] = lambda: F.march_bwd(vol, tf1, cam, e, x, r, n, S, 1.0, g, outa, want_vol=want_vol,
                                                    want_tf=want_tf, workspace=ws)
            else:   # the default TF-only path: the per-sample tape the forward left (Raycaster's choice when it fits)
                fns["auto1d"] = lambda: F.march_bwd(vol, tf1, cam, e, x, r, n, S, 1.0, g, outt, want_vol=False, workspace=wst,
                                                    tape=True)
            for k, fn in fns.items():
                fn(); fn()
            torch.cuda.synchronize()
            rec = {"shape": [nv, ni, V], "tf": [RV, RG], "pass": tag}
            for k, fn in fns.items():
                rec[k + "_ms"] = timed(fn, args.min_seconds)
            rec["tf2d_over_base1d"] = rec["tf2d_ms"] / rec["base1d_ms"]
            rec["tf2d_over_auto1d"] = rec["tf2d_ms"] / rec["auto1d_ms"]
            print(json.dumps(rec), flush=True)
        del ws, wst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
