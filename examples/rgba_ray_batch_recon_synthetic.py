#!/usr/bin/env python3
"""Recovery of an RGBA volume (a per-voxel radiance grid: no transfer function) from K pinhole views, each step on a random
minibatch of rays drawn across ALL views: the rays of every view come from pinhole_rays once, the targets from
rendering vol_gt along them, and a step renders `--rays` of the K H W rays with RayBundleRaycasterRGBA.
loss = mse of the ray colours + lam * fused_tv3d_loss(alpha channel). Prints the loss trajectory and, at the start and at the
end, the image error of whole held-out views (cameras between the training ones), rendered with RaycasterRGBA."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd.bundle import pinhole_rays  # noqa: E402
from differender_amd.rgba import RayBundleRaycasterRGBA, RaycasterRGBA, interleaved  # noqa: E402
from differender_amd.utils import fused_tv3d_loss  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def synthetic_rgba(n, device):
    """(4, D, H, W): the synthetic scalar volume's shells coloured by position, its alpha a soft threshold of the scalar."""
    s = synthetic_volume(n, device)[0]
    ax = torch.linspace(-1, 1, n, device=device)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    rgb = torch.stack([0.5 + 0.45 * x, 0.5 + 0.45 * y, 0.5 + 0.45 * z])
    alpha = 0.25 * torch.clamp((s - 0.2) / 0.5, 0.0, 1.0) ** 2
    return torch.cat([rgb * (alpha > 0), alpha[None]]).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=32)
    ap.add_argument("--img", type=int, default=48)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--held-out", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096, help="rays per step, drawn across all views")
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--lam", type=float, default=0.05, help="weight of the TV term on alpha (0: off)")
    ap.add_argument("--lr", type=float, default=3e-2, help="OneCycle max_lr")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    vol_gt = synthetic_rgba(args.vol, dev)
    zero, up = torch.zeros(3, device=dev), torch.tensor([0.0, 1.0, 0.0], device=dev)
    angle = lambda k: 2.0 * math.pi * k / args.views
    rays = [pinhole_rays(in_circles(angle(k)).float().to(dev), zero, up, 30.0, (args.img, args.img)) for k in range(args.views)]
    origins = torch.cat([o.reshape(-1, 3) for o, _ in rays])
    directions = torch.cat([d.reshape(-1, 3) for _, d in rays])
    raycast = RayBundleRaycasterRGBA(vol_gt.shape[-3:], jitter=True, max_samples=1024)
    with torch.no_grad():
        target = RayBundleRaycasterRGBA(vol_gt.shape[-3:], sampling_rate=4.0, jitter=False, max_samples=4096)(
            vol_gt, origins, directions)
    # whole held-out views, halfway between training cameras
    whole = RaycasterRGBA(vol_gt.shape[-3:], (args.img, args.img), sampling_rate=2.0, jitter=False, max_samples=4096)
    held = torch.stack([in_circles(angle(k * (args.views // max(args.held_out, 1)) + 0.5)).float() for k in range(args.held_out)]).to(dev)

    def held_out_error(v):
        with torch.no_grad():
            return float(sum(torch.nn.functional.mse_loss(whole(v, c), whole(vol_gt, c)) for c in held) / len(held))

    # the channels of a voxel next to each other: one load per corner (same values, same bits)
    vol = interleaved(torch.cat([torch.full((3, *vol_gt.shape[-3:]), 0.5, device=dev),
                                 0.02 + 0.02 * torch.rand((1, *vol_gt.shape[-3:]), device=dev)])).requires_grad_(True)
    opt = torch.optim.AdamW([vol], weight_decay=0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr, total_steps=args.iterations)
    err0 = held_out_error(vol.detach())
    first = last = None
    for i in range(args.iterations):
        pick = torch.randint(0, origins.shape[0], (args.rays,), device=dev)
        opt.zero_grad()
        res = raycast(vol, origins[pick], directions[pick])
        mse = torch.nn.functional.mse_loss(res, target[pick])
        tv = fused_tv3d_loss(vol[3])
        loss = mse + args.lam * tv if args.lam else mse
        loss.backward()
        last = loss.item()
        first = last if first is None else first
        if i % 25 == 0 or i == args.iterations - 1:
            print(f"Step {i:03d}:   Loss: {last:0.5f}   MSE: {mse.item():0.5f}   TV(alpha): {tv.item():0.5f}   "
                  f"LR: {sched.get_last_lr()[0]:.1e}")
        opt.step(); sched.step()
        with torch.no_grad():
            vol.clamp_(0.0, 1.0)
    err1 = held_out_error(vol.detach())
    print(f"loss {first:.5f} -> {last:.5f} on {args.rays} of {origins.shape[0]} rays per step")
    print(f"image mse on {args.held_out} held-out views: {err0:.6e} -> {err1:.6e}")


if __name__ == "__main__":
    main()
