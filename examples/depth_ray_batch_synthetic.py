#!/usr/bin/env python3
"""Volume reconstruction from range data: ray_batch_recon_synthetic.py with depth rays in the colour rays'
place. The rays of K pinhole views come from pinhole_rays once, the targets from the depth moments of vol_gt along them, and a
step renders `--rays` of the K H W rays, drawn across ALL views, with RayBundleDepthRaycaster.
loss = mse of the premultiplied moments (M1, A) + lam * fused_tv3d_loss(vol): the premultiplied first moment rather than the
quotient M1 / A, whose gradient blows up where a ray collects almost nothing (examples/depth_pose_synthetic.py argues the same).
Prints the first and the last loss and the volume's MSE to vol_gt at the start and at the end."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import get_tf, in_circles  # noqa: E402
from differender_amd.bundle import pinhole_rays  # noqa: E402
from differender_amd.depth import RayBundleDepthRaycaster  # noqa: E402
from differender_amd.utils import fused_tv3d_loss  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=32)
    ap.add_argument("--img", type=int, default=48)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--rays", type=int, default=4096, help="rays per step, drawn across all views")
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--lam", type=float, default=0.05, help="weight of the TV term (0: off)")
    ap.add_argument("--lr", type=float, default=2e-2, help="OneCycle max_lr")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    TF_RES = 64
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    tf = get_tf("tf1", TF_RES).to(dev).float()
    vol_gt = synthetic_volume(args.vol, dev).float()
    zero, up = torch.zeros(3, device=dev), torch.tensor([0.0, 1.0, 0.0], device=dev)
    rays = [pinhole_rays(in_circles(6.283 * k / args.views).float().to(dev), zero, up, 30.0, (args.img, args.img))
            for k in range(args.views)]
    origins = torch.cat([o.reshape(-1, 3) for o, _ in rays])
    directions = torch.cat([d.reshape(-1, 3) for _, d in rays])
    # t_near = 0: a sensor's ray starts at the sensor, and M1 / A is a range
    raycast = RayBundleDepthRaycaster(vol_gt.shape[-3:], TF_RES, jitter=True, max_samples=1024, t_near=0.0)
    with torch.no_grad():
        target = RayBundleDepthRaycaster(vol_gt.shape[-3:], TF_RES, sampling_rate=4.0, jitter=False, max_samples=4096, t_near=0.0)(
            vol_gt, tf, origins, directions)[..., (0, 2)]
    vol = (0.1 + 0.5 * torch.rand_like(vol_gt)).requires_grad_(True)
    opt = torch.optim.AdamW([vol], weight_decay=0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr, total_steps=args.iterations)
    vol_mse0 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    losses = []
    for i in range(args.iterations):
        pick = torch.randint(0, origins.shape[0], (args.rays,), device=dev)
        opt.zero_grad()
        res = raycast(vol, tf, origins[pick], directions[pick])[..., (0, 2)]
        mse = torch.nn.functional.mse_loss(res, target[pick])
        tv = fused_tv3d_loss(vol)
        loss = mse + args.lam * tv if args.lam else mse
        loss.backward()
        losses.append(loss.item())
        if not args.quiet and (i % 25 == 0 or i == args.iterations - 1):
            print(f"Step {i:03d}:   Loss: {losses[-1]:0.5f}   MSE: {mse.item():0.5f}   TV: {tv.item():0.5f}   "
                  f"LR: {sched.get_last_lr()[0]:.1e}")
        opt.step(); sched.step()
        with torch.no_grad():
            vol.clamp_(0.0, 1.0)
    vol_mse1 = float(torch.nn.functional.mse_loss(vol.detach(), vol_gt))
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f} on {args.rays} of {origins.shape[0]} rays per step")
    print(f"volume mse to vol_gt: {vol_mse0:.6e} -> {vol_mse1:.6e}")
    return dict(losses=losses, vol_mse=(vol_mse0, vol_mse1))


if __name__ == "__main__":
    main()
