#!/usr/bin/env python3
"""The volume reconstruction loop of examples/test_opt_synthetic.py (the reference's examples/test_opt_tf.py on synthetic data:
5 % of the voxels randomised, 8 views per step, AdamW + OneCycle on `vol`, clamp to [0, 1]) with a 3-D total-variation prior on
the volume: loss = dssim + mse of the renders + lam * fused_tv3d_loss(vol). Prints the volume's MSE to vol_gt
at the start and at the end; `--lam 0` runs the same loop without the prior."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import get_tf, in_circles, get_rand_pos  # noqa: E402
from differender.volume_raycaster import Raycaster  # noqa: E402
from differender_amd.utils import fused_dssim_mse_loss, fused_tv3d_loss  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=128)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--lam", type=float, default=1.0, help="weight of the TV term (0: off)")
    ap.add_argument("--norm", default="l1", choices=("l1", "iso", "sq"))
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--lr", type=float, default=1e-3, help="OneCycle max_lr")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    TF_RES, BS = 128, 8
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    tf = get_tf("tf1", TF_RES)
    tf_gt = get_tf("tf1", TF_RES).to(dev).expand(BS, -1, -1).float()
    vol_gt = synthetic_volume(args.vol, dev)
    vol = vol_gt.clone()
    mask = torch.rand_like(vol) < 0.05
    vol[mask] = torch.rand_like(vol[mask])
    raycast = Raycaster(vol.shape[-3:], (args.img, args.img), TF_RES, jitter=True, max_samples=1024)
    vol = vol.float().requires_grad_(True)
    tf = tf.to(dev).float().requires_grad_(True)
    opt = torch.optim.AdamW([vol], weight_decay=0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr, total_steps=args.iterations)
    vol_mse0 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    for i in range(args.iterations):
        lf = torch.cat([in_circles(0.1 * i)[None], get_rand_pos(BS - 1)], dim=0).float().to(dev)
        with torch.no_grad():
            gt = raycast.raycast_nondiff(vol_gt.detach(), tf_gt.detach(), lf.detach(), sampling_rate=8.0)
        opt.zero_grad()
        res = raycast(vol, tf, lf)
        loss, dssim, mse = fused_dssim_mse_loss(res, gt)
        tv = fused_tv3d_loss(vol, norm=args.norm, eps=args.eps)
        if args.lam:
            loss = loss + args.lam * tv
        loss.backward()
        if i % 10 == 0 or i == args.iterations - 1:
            print(f"Step {i:03d}:   Loss: {loss.item():0.4f}   DSSIM: {dssim.item():0.4f}   MSE: {mse.item():0.5f}   "
                  f"TV: {tv.item():0.5f}   LR: {sched.get_last_lr()[0]:.1e}")
        opt.step(); sched.step()
        with torch.no_grad():
            tf.clamp_(0.0, 1.0); vol.clamp_(0.0, 1.0)
    vol_mse1 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    print(f"volume mse to vol_gt (lam {args.lam:g}): {vol_mse0:.6e} -> {vol_mse1:.6e}")


if __name__ == "__main__":
    main()
