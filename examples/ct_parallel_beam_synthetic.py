#!/usr/bin/env python3
"""Parallel-beam CT on synthetic data: reconstruct examples.render_nondiff_synthetic.synthetic_volume from K parallel-beam
projections taken on a circle around the y axis -- a geometry without a pinhole, drawn with bundle.orthographic_rays and
projected by differender_amd.projection.RayBundleProjector. Every view's detector pixels are handed over in
bundle.tile_order, so that 256 consecutive rays are one 16 x 16 detector tile (what the volume backward collects in LDS). The
volume starts at a constant; each step projects all K views and minimises mse(projections, measured) + lam *
fused_tv3d_loss(vol) with Adam, clamping the volume to [0, 1]. Prints the first and the last loss and the
volume's MSE to the ground truth; `--lam 0` runs the same loop without the prior."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.bundle import orthographic_rays, tile_order  # noqa: E402
from differender_amd.projection import RayBundleProjector  # noqa: E402
from differender_amd.utils import fused_tv3d_loss  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def parallel_beam(views, det, extent, dev):
    """The rays of `views` parallel-beam projections over half a turn, each a det x det detector `extent` world units wide, in
    tile order -> origins, directions (views, det * det, 3)."""
    perm = tile_order((det, det)).to(dev)
    at, up = torch.zeros(3, device=dev), torch.tensor([0.0, 1.0, 0.0], device=dev)
    rays = []
    for k in range(views):
        phi = math.pi * (k + 0.5) / views
        src = 3.0 * torch.tensor([math.sin(phi), 0.0, math.cos(phi)], device=dev)
        o, d = orthographic_rays(src, at, up, extent, (det, det))
        rays.append((o.reshape(-1, 3)[perm], d.reshape(-1, 3)[perm]))
    return torch.stack([o for o, _ in rays]), torch.stack([d for _, d in rays])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--det", type=int, default=128, help="detector pixels per side")
    ap.add_argument("--views", type=int, default=24, help="K: number of measured projections")
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--lam", type=float, default=1e-3, help="weight of the TV term (0: off)")
    ap.add_argument("--lr", type=float, default=2e-2)
    args = ap.parse_args()
    dev = torch.device("cuda")
    vol_gt = synthetic_volume(args.vol, dev)
    origins, dirs = parallel_beam(args.views, args.det, 2.0 * math.sqrt(2.0), dev)
    proj = RayBundleProjector(vol_gt.shape[-3:], mode="sum", jitter=False)
    proj_gt = RayBundleProjector(vol_gt.shape[-3:], mode="sum", sampling_rate=4.0, jitter=False)
    with torch.no_grad():
        measured = proj_gt(vol_gt, origins, dirs)
    vol = torch.full_like(vol_gt, float(vol_gt.mean())).requires_grad_(True)
    opt = torch.optim.Adam([vol], lr=args.lr)
    vol_mse0 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    first = last = None
    for i in range(args.iterations):
        opt.zero_grad()
        mse = torch.nn.functional.mse_loss(proj(vol, origins, dirs), measured)
        tv = fused_tv3d_loss(vol)
        loss = mse + args.lam * tv if args.lam else mse
        loss.backward()
        last = loss.item()
        first = last if first is None else first
        if i % 25 == 0 or i == args.iterations - 1:
            print(f"Step {i:03d}:   Loss: {last:0.6f}   MSE: {mse.item():0.6f}   TV: {tv.item():0.5f}")
        opt.step()
        with torch.no_grad():
            vol.clamp_(0.0, 1.0)
    vol_mse1 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    print(f"loss: first {first:.6f}  last {last:.6f}")
    print(f"volume MSE to ground truth: start {vol_mse0:.6f}  end {vol_mse1:.6f}")


if __name__ == "__main__":
    main()
