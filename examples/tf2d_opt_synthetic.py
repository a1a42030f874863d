#!/usr/bin/env python3
"""Fit a 2-D (value, gradient-magnitude) transfer function to renders of a scene in which boundaries and
interiors share intensities: a sphere of value 1 holding a sphere of value 0.5. The outer boundary ramps from 0 to 1 and crosses
0.5 with a steep gradient; the inner sphere IS 0.5, with none. No 1-D TF can colour the two differently. The targets are
rendered with a 2-D table that paints high-u samples (boundaries) orange and low-u ones (interiors) translucent blue; a grey
table is then fitted to them, TF only, through differender_amd.tf2d.Raycaster2D and torch.optim.Adam.
Prints the first and the last loss."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd.tf2d import Raycaster2D, gradient_scale  # noqa: E402


def nested_spheres(n, dev):
    """(1, n, n, n): value 1 inside radius 0.75, 0.5 inside radius 0.35, edges smoothed over ~1.5 voxels."""
    c = torch.linspace(-1.0, 1.0, n, device=dev)
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    w = 1.5 * 2.0 / (n - 1)
    outer = torch.sigmoid((0.75 - r) / w)
    inner = torch.sigmoid((0.35 - r) / w)
    return (outer - 0.5 * inner)[None]


def target_tf(RV, RG, dev):
    """(4, RV, RG): nothing below value 0.2; above it orange and fairly opaque at high u, faint blue at low u."""
    v = torch.linspace(0.0, 1.0, RV, device=dev)[:, None]
    u = torch.linspace(0.0, 1.0, RG, device=dev)[None, :]
    edge = torch.clamp((u - 0.2) / 0.4, 0.0, 1.0)
    on = (v > 0.2).float()
    r = 0.2 + 0.8 * edge
    g = 0.3 + 0.3 * edge
    b = 0.9 - 0.8 * edge
    a = on * (0.02 + 0.3 * edge)
    return torch.stack([r.expand(RV, RG), g.expand(RV, RG), b.expand(RV, RG), a], 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--tf-res", type=int, nargs=2, default=(32, 16), metavar=("RV", "RG"))
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.05)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    RV, RG = args.tf_res
    vol = nested_spheres(args.vol, dev)
    g_scale = gradient_scale(vol, q=0.99)
    rc = Raycaster2D(vol.shape[-3:], (args.img, args.img), (RV, RG), g_scale, sampling_rate=1.0, jitter=True)
    cams = torch.stack([in_circles(1.7 + 1.3 * i).float() for i in range(args.views)]).to(dev)
    with torch.no_grad():
        targets = rc(vol, target_tf(RV, RG, dev), cams)
    tf = torch.full((4, RV, RG), 0.5, device=dev)
    tf[3] = 0.05
    tf.requires_grad_(True)
    opt = torch.optim.Adam([tf], lr=args.lr)
    losses = []
    for i in range(args.iters):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rc(vol, tf, cams), targets)
        loss.backward()
        opt.step()
        with torch.no_grad():
            tf.clamp_(0.0, 1.0)
        losses.append(loss.detach())
        if i % 25 == 0 or i == args.iters - 1:
            print(f"[{i:04d}] loss {float(loss):.6e}")
    print(f"first loss {float(losses[0]):.6e}")
    print(f"last loss {float(losses[-1]):.6e}")
