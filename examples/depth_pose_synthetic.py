#!/usr/bin/env python3
"""Register a free camera against ONE depth image of a known volume: the counterpart of
examples/pose_opt_synthetic.py, which can only use colour. The synthetic volume and the preset "tf1" are known; a depth image
(the expected ray depth where the ray meets anything, and the opacity that says where it does) is rendered from a panned,
rolled, zoomed camera without jitter, and look_from, look_at, up and fov are fitted from a perturbed pose with Adam, through
DepthRaycaster(camera_grad=True) and the four tensors' gradients. The loss is the MSE between the depth images in
premultiplied form, (opacity x depth, opacity): that is the first moment M1 itself, which falls to 0 with the opacity at a
silhouette, where the depth alone jumps from the object's distance to the background's and has no gradient to offer. Prints the
pose error per iteration, measured as pose_opt_synthetic.pose_error measures it (the reprojection error of the box's corners is
the figure that says how far the fitted camera is from the true one as a camera).

One depth image of this nearly round object pins the roll weakly, and the recovery in 60-80 iterations is partial (DESIGN.md
D18): the reprojection, rotation and fov errors and the loss fall, the position error is printed, not promised."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.depth import DepthRaycaster, expected_depth  # noqa: E402
from differender_amd.utils import get_tf, in_circles  # noqa: E402
from examples.pose_opt_synthetic import pose_error  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def depth_image(m):
    """What a range sensor hands over, from the moments ([BS,]3,H,W): the depth (0 where nothing was met) and the opacity."""
    return expected_depth(m), m[..., 2, :, :]


def premultiplied(depth, opacity):
    """A depth image as the loss compares it: (opacity x depth, opacity), continuous across silhouettes."""
    return torch.stack([opacity * depth, opacity], dim=-3)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=96)
    ap.add_argument("--tf-res", type=int, default=64)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--angle", type=float, default=1.0, help="orbit angle of the ground-truth camera position (radians)")
    ap.add_argument("--offset", type=float, default=6.0, help="the start's distance along the orbit from the truth (degrees)")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--fov-lr-scale", type=float, default=10.0, help="the fov's step size as a multiple of --lr")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    vol = synthetic_volume(args.vol, dev)                       # (1, D, H, W)
    tf = get_tf("tf1", args.tf_res).float().to(dev)             # (4, R)
    rc = DepthRaycaster(vol.shape[-3:], (args.img, args.img), args.tf_res, jitter=False, max_samples=1 << 20, camera_grad=True)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    # ground truth: panned off the object's centre, rolled by ~15 degrees, zoomed in from the module's 30 to 26 degrees
    gt = (in_circles(args.angle).float().to(dev), t([0.15, -0.1, 0.1]), t([0.26, 0.97, 0.0]), t(26.0))
    with torch.no_grad():
        ref = premultiplied(*depth_image(rc(vol, tf, gt[0], look_at=gt[1], up=gt[2], fov=gt[3])))   # the sensor's image
    # start: --offset degrees further along the orbit, looking at the centre, upright, the module's fov
    pose = [in_circles(args.angle + math.radians(args.offset)).float().to(dev), t([0.0, 0.0, 0.0]), t([0.0, 1.0, 0.0]), t(30.0)]
    pose = [p.requires_grad_(True) for p in pose]
    # (a degree of fov moves the image about as much as 0.03 world units of look_at: its own step size)
    opt = torch.optim.Adam([{"params": pose[:3]}, {"params": pose[3:], "lr": args.fov_lr_scale * args.lr}], lr=args.lr)
    errors, losses = [], []

    def objective():
        m = rc(vol, tf, pose[0], look_at=pose[1], up=pose[2], fov=pose[3])
        return torch.nn.functional.mse_loss(torch.stack([m[..., 0, :, :], m[..., 2, :, :]], dim=-3), ref)   # (M1, A)

    for i in range(args.iters):
        opt.zero_grad()
        loss = objective()
        loss.backward()
        errors.append(pose_error([p.detach() for p in pose], gt))
        losses.append(float(loss.detach()))
        if not args.quiet:
            print(f"iter {i:3d}  loss {losses[-1]:.4e}  reprojection {errors[-1][0]:.4f}  position {errors[-1][1]:.4f}  "
                  f"rotation {errors[-1][2]:.3f} deg  fov {errors[-1][3]:.3f} deg")
        opt.step()
    errors.append(pose_error([p.detach() for p in pose], gt))
    with torch.no_grad():
        losses.append(float(objective()))
    if not args.quiet:
        print("pose error (reprojection, position, rotation deg, fov deg): "
              f"{tuple(round(v, 4) for v in errors[0])} -> {tuple(round(v, 4) for v in errors[-1])}")
    return {"errors": errors, "losses": losses}


if __name__ == "__main__":
    main()
