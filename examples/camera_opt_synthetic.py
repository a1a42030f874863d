#!/usr/bin/env python3
"""Recover a camera position from an image (pose recovery through the camera gradient): render a ground truth
at in_circles(t) without jitter, start 12 degrees further along the same orbit, and fit look_from with Adam on the MSE
between the renders, through Raycaster and look_from.grad. Prints the camera error per iteration."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.utils import get_tf, in_circles  # noqa: E402
from differender_amd.volume_raycaster import Raycaster  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=128)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--tf-res", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--angle", type=float, default=1.0, help="orbit angle of the ground-truth camera (radians)")
    ap.add_argument("--offset-deg", type=float, default=12.0, help="where the fit starts: this far along the orbit")
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    vol = synthetic_volume(args.vol, dev)                       # (1, D, H, W)
    tf = get_tf("tf1", args.tf_res).float().to(dev)             # (4, R)
    rc = Raycaster(vol.shape[-3:], (args.img, args.img), args.tf_res, jitter=False, max_samples=1 << 20)
    cam_gt = in_circles(args.angle).to(dev)
    with torch.no_grad():
        ref = rc(vol, tf, cam_gt)
    cam = in_circles(args.angle + math.radians(args.offset_deg)).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([cam], lr=args.lr)
    errors, losses = [], []
    for i in range(args.iterations):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rc(vol, tf, cam), ref)
        loss.backward()
        errors.append(float((cam.detach() - cam_gt).norm()))
        losses.append(float(loss))
        if not args.quiet:
            print(f"iter {i:3d}  loss {losses[-1]:.4e}  camera error {errors[-1]:.4f}")
        opt.step()
    errors.append(float((cam.detach() - cam_gt).norm()))
    if not args.quiet:
        print(f"camera error {errors[0]:.4f} -> {errors[-1]:.4f}; final camera {cam.detach().cpu().tolist()}, "
              f"ground truth {cam_gt.cpu().tolist()}")
    return {"errors": errors, "losses": losses}


if __name__ == "__main__":
    main()
