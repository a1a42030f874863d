#!/usr/bin/env python3
"""Recover a pre-classified RGBA volume from images alone, with no transfer function to guess.

The ground truth is the synthetic scalar volume of examples/render_nondiff_synthetic.py classified per voxel with the shipped
preset "tf1"; K views of it are rendered once with RaycasterRGBA.raycast_nondiff. A free RGBA volume (interleaved, so that the
kernels fetch a voxel with one load) is then fitted to those images: loss = mse of the renders + lam * fused_tv3d_loss(volume),
Adam, clamp to [0, 1] after each step. Prints the first and the last loss."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.rgba import RaycasterRGBA, interleaved  # noqa: E402
from differender_amd.utils import fused_tv3d_loss, get_tf, in_circles  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def classify(vol, tf):
    """vol (1, D, H, W) in [0, 1], tf (4, R) -> (4, D, H, W): the TF's linear interpolation at every voxel."""
    R = tf.shape[1]
    x = vol[0].clamp(0.0, 1.0) * (R - 1)
    lo = x.floor().long().clamp(max=R - 1)
    hi = (lo + 1).clamp(max=R - 1)
    fr = x - lo
    return tf[:, lo] * (1.0 - fr) + tf[:, hi] * fr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=64)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lam", type=float, default=0.05, help="weight of the TV term (0: off)")
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    vol_gt = classify(synthetic_volume(args.vol, dev), get_tf("tf1", 128).to(dev).float())
    raycast = RaycasterRGBA(vol_gt.shape[-3:], (args.img, args.img), jitter=True, max_samples=1024)
    lf = torch.stack([in_circles(6.2831853 * k / args.views) for k in range(args.views)]).float().to(dev)
    gt = raycast.raycast_nondiff(vol_gt, lf, sampling_rate=8.0)
    start = torch.full_like(vol_gt, 0.5)
    start[3] = 0.05
    vol = interleaved(start).detach().requires_grad_(True)
    opt = torch.optim.Adam([vol], lr=args.lr)
    first = last = None
    for i in range(args.steps):
        opt.zero_grad()
        res = raycast(vol, lf)
        mse = torch.nn.functional.mse_loss(res, gt)
        loss = mse + args.lam * fused_tv3d_loss(vol) if args.lam else mse
        loss.backward()
        opt.step()
        with torch.no_grad():
            vol.clamp_(0.0, 1.0)
        last = float(loss)
        first = last if first is None else first
        if i % 20 == 0 or i == args.steps - 1:
            print(f"Step {i:03d}:   Loss: {last:0.6f}   MSE: {float(mse):0.6f}")
    vol_mse = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    print(f"first loss {first:.6e} last loss {last:.6e}   volume mse to the ground truth {vol_mse:.6e}")


if __name__ == "__main__":
    main()
