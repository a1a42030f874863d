#!/usr/bin/env python3
"""Register a free camera against a known RGBA volume: examples/pose_opt_synthetic.py without a transfer
function. The volume is the ground truth of examples/rgba_recon_synthetic.py (the synthetic scalar volume classified per voxel
with the preset "tf1"); one image of it is rendered from a panned, rolled, zoomed camera without jitter, and look_from, look_at,
up and fov are fitted from a perturbed pose with Adam on the MSE between the renders, through
RaycasterRGBA(camera_grad=True) and the four tensors' gradients. Prints the pose error per iteration, measured as
pose_opt_synthetic.pose_error measures it (the reprojection error of the box's corners is the figure that says how far the
fitted camera is from the true one as a camera).

The classified volume constrains the roll weakly (it is close to a solid of revolution): the start is nearer the truth
(--offset 3 degrees along the orbit) and the steps smaller (--lr 0.004, the fov's 10x that) than pose_opt_synthetic.py's, and
the recovery in 60-80 iterations is partial."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.rgba import RaycasterRGBA, interleaved  # noqa: E402
from differender_amd.utils import get_tf, in_circles  # noqa: E402
from examples.pose_opt_synthetic import pose_error  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402
from examples.rgba_recon_synthetic import classify  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=96)
    ap.add_argument("--iterations", type=int, default=80)
    ap.add_argument("--angle", type=float, default=1.0, help="orbit angle of the ground-truth camera position (radians)")
    ap.add_argument("--offset", type=float, default=3.0, help="the start's distance along the orbit from the truth (degrees)")
    ap.add_argument("--lr", type=float, default=0.004)
    ap.add_argument("--fov-lr-scale", type=float, default=10.0, help="the fov's step size as a multiple of --lr")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    vol = interleaved(classify(synthetic_volume(args.vol, dev), get_tf("tf1", 128).to(dev).float()))   # (4, D, H, W)
    rc = RaycasterRGBA(vol.shape[-3:], (args.img, args.img), jitter=False, max_samples=1 << 20, camera_grad=True)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    # ground truth: panned off the object's centre, rolled by ~15 degrees, zoomed in from the module's 30 to 26 degrees
    gt = (in_circles(args.angle).float().to(dev), t([0.15, -0.1, 0.1]), t([0.26, 0.97, 0.0]), t(26.0))
    with torch.no_grad():
        ref = rc(vol, gt[0], look_at=gt[1], up=gt[2], fov=gt[3])
    # start: --offset degrees further along the orbit, looking at the centre, upright, the module's fov
    pose = [in_circles(args.angle + math.radians(args.offset)).float().to(dev), t([0.0, 0.0, 0.0]), t([0.0, 1.0, 0.0]), t(30.0)]
    pose = [p.requires_grad_(True) for p in pose]
    # (a degree of fov moves the image about as much as 0.03 world units of look_at: its own step size)
    opt = torch.optim.Adam([{"params": pose[:3]}, {"params": pose[3:], "lr": args.fov_lr_scale * args.lr}], lr=args.lr)
    errors, losses = [], []
    for i in range(args.iterations):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rc(vol, pose[0], look_at=pose[1], up=pose[2], fov=pose[3]), ref)
        loss.backward()
        errors.append(pose_error([p.detach() for p in pose], gt))
        losses.append(float(loss.detach()))
        if not args.quiet:
            print(f"iter {i:3d}  loss {losses[-1]:.4e}  reprojection {errors[-1][0]:.4f}  position {errors[-1][1]:.4f}  "
                  f"rotation {errors[-1][2]:.3f} deg  fov {errors[-1][3]:.3f} deg")
        opt.step()
    errors.append(pose_error([p.detach() for p in pose], gt))
    if not args.quiet:
        print("pose error (reprojection, position, rotation deg, fov deg): "
              f"{tuple(round(v, 4) for v in errors[0])} -> {tuple(round(v, 4) for v in errors[-1])}")
    return {"errors": errors, "losses": losses}


if __name__ == "__main__":
    main()
