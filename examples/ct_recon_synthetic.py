#!/usr/bin/env python3
"""Sparse-view CT on synthetic data: reconstruct examples.render_nondiff_synthetic.synthetic_volume from K X-ray line-integral
projections (differender_amd.projection.Projector) taken on random orbits. The volume starts at a constant; each
step renders a batch of the K views and minimises mse(projections, measured) + lam * fused_tv3d_loss(vol) with
Adam, clamping the volume to [0, 1]. Prints the volume's MSE to the ground truth at the start and at the end; `--lam 0` runs the
same loop without the prior."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import get_rand_pos  # noqa: E402
from differender_amd.projection import Projector  # noqa: E402
from differender_amd.utils import fused_tv3d_loss  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--views", type=int, default=24, help="K: number of measured projections")
    ap.add_argument("--batch", type=int, default=8, help="projections per step")
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--lam", type=float, default=1e-3, help="weight of the TV term (0: off)")
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    vol_gt = synthetic_volume(args.vol, dev)
    proj = Projector(vol_gt.shape[-3:], (args.img, args.img), mode="sum", jitter=True)
    proj_gt = Projector(vol_gt.shape[-3:], (args.img, args.img), mode="sum", sampling_rate=4.0, jitter=False)
    lf_all = get_rand_pos(args.views).float().to(dev)
    with torch.no_grad():
        measured = proj_gt(vol_gt.expand(args.views, -1, -1, -1, -1), lf_all)
    vol = torch.full_like(vol_gt, float(vol_gt.mean())).requires_grad_(True)
    opt = torch.optim.Adam([vol], lr=args.lr)
    vol_mse0 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    for i in range(args.iterations):
        pick = torch.randperm(args.views, device=dev)[:args.batch]
        opt.zero_grad()
        res = proj(vol, lf_all[pick])
        mse = torch.nn.functional.mse_loss(res, measured[pick])
        tv = fused_tv3d_loss(vol)
        loss = mse + args.lam * tv if args.lam else mse
        loss.backward()
        if i % 25 == 0 or i == args.iterations - 1:
            print(f"Step {i:03d}:   Loss: {loss.item():0.6f}   MSE: {mse.item():0.6f}   TV: {tv.item():0.5f}")
        opt.step()
        with torch.no_grad():
            vol.clamp_(0.0, 1.0)
    vol_mse1 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    print(f"volume MSE to ground truth: start {vol_mse0:.6f}  end {vol_mse1:.6f}")


if __name__ == "__main__":
    main()
