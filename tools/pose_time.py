#!/usr/bin/env python3
"""The brick-centric march under a free camera at the headline size: forward and volume + TF backward for the
fixed camera, for the default pose handed in as a pose (the same rays through the pose's branch), and for a panned + rolled
(+ zoomed) camera, on a synthetic 512^3 volume, a 512^2 image, one view, rate 1, a thin TF (no early termination). Device
events around windows of at least --min-seconds after a warm-up; one JSON line per case with ms per call and the forward's
workspace header (words 0, 2, 5, 15: repaired rays, rays marched one by one, overflow items, D4-recomputed rays). For kernel
times run ONE case under `rocprofv3 --kernel-trace --stats` (--case NAME). GPU only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402
from tools.proj_time import timed  # noqa: E402

CASES = {
    "fixed": None,
    "default_pose": ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), None),
    "panned_rolled": ((0.2, -0.15, 0.1), (0.35, 1.0, -0.2), None),
    "panned_rolled_zoomed": ((0.2, -0.15, 0.1), (0.35, 1.0, -0.2), 24.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=512)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--case", default="all", choices=["all", *CASES])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/pose_time.py needs a ROCm device"
    dev = torch.device("cuda")
    vol = synthetic_volume(args.vol, dev)[0].permute(2, 0, 1)   # (W, D, H) view of the (1, D, H, W) tensor: x contiguous
    v = torch.linspace(0.0, 1.0, 256, device=dev)
    tf = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.01 + 0.0 * v], 1).contiguous()
    cam = in_circles(0.3).float().to(dev).reshape(1, 3)
    WH, S = (args.img, args.img), 1 << 20
    g = torch.randn((1, *WH, 4), device=dev)
    for name in (CASES if args.case == "all" else [args.case]):
        kw = {}
        if CASES[name] is None:
            rays = F.ray_setup(cam, WH, vol.shape, 1.0)
        else:
            look_at, up, fov = CASES[name]
            pose = F.pack_pose(cam, torch.tensor(look_at, device=dev), torch.tensor(up, device=dev))
            fov_v = None if fov is None else torch.deg2rad(torch.tensor([fov], device=dev))
            rays = F.ray_setup_pose(pose, WH, vol.shape, 1.0, fov_v=fov_v)
            kw = dict(pose=pose, fov_v=fov_v)
        ws = F.alloc_workspace(1, WH, vol.shape, tf.shape[0], dev)
        fwd = lambda: F.march_fwd(vol, tf, cam, *rays, S, 1.0, workspace=ws, hints=0, **kw)
        out, _ = fwd()
        stats = F.workspace_stats(ws)
        bwd = lambda: F.march_bwd(vol, tf, cam, *rays, S, 1.0, g, out, workspace=ws, **kw)
        line = {"case": name, "volume": args.vol, "image": args.img, "samples": int(rays[3].clamp(min=0).sum()),
                "rays_hit": int((rays[3] > 1).sum()), "repaired": int(stats[0]), "marched_one_by_one": int(stats[2]),
                "overflow_items": int(stats[5]), "exact": int(stats[15]),
                "fwd_ms": round(timed(fwd, args.min_seconds), 4), "bwd_ms": round(timed(bwd, args.min_seconds), 4)}
        line["ns_per_sample_fwd"] = round(1e6 * line["fwd_ms"] / max(line["samples"], 1), 4)
        line["ns_per_sample_bwd"] = round(1e6 * line["bwd_ms"] / max(line["samples"], 1), 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
