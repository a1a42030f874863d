#!/usr/bin/env python3
"""Recover a free camera from an image: render a ground truth from a panned, rolled, zoomed camera without
jitter, start from a perturbed pose, and fit look_from, look_at, up and fov together with Adam on the MSE between the renders,
through Raycaster and the four tensors' gradients. Prints the pose error per iteration.

look_at may slide along the viewing direction and up may change its length or lean towards the viewer without moving a single
ray, so the error is measured on what the pose means: the camera position, the rotation between the two camera frames
(right, up', view_dir), and the field of view. From ONE image the distance along the viewing direction and the field of view
are only weakly separable (a dolly zoom: stepping back while zooming in moves the picture little), so the position error alone
can stall or grow while the picture converges; the figure that says how far the fitted camera is from the true one AS A CAMERA
is the reprojection error: the RMS distance on the image plane, in image heights, between where the two cameras see the eight
corners of the volume's box."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender_amd.utils import get_tf, in_circles  # noqa: E402
from differender_amd.volume_raycaster import Raycaster  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def camera_frame(look_from, look_at, up):
    """The rows right, up', view_dir of the camera model (ray_setup): a rotation matrix."""
    n = torch.nn.functional.normalize
    view_dir = n(look_at - look_from, dim=-1)
    right = n(torch.linalg.cross(view_dir, up), dim=-1)
    return torch.stack([right, n(torch.linalg.cross(right, view_dir), dim=-1), view_dir])


def project_corners(look_from, look_at, up, fov):
    """Image-plane coordinates (u, v), in image heights from the centre (square image), of the box's eight corners (8, 2)."""
    corners = torch.tensor([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)], device=look_from.device)
    p = (corners - look_from) @ camera_frame(look_from, look_at, up).T          # along right, up', view_dir
    return p[:, :2] / (p[:, 2:] * 2.0 * torch.tan(torch.deg2rad(fov)))


def pose_error(pose, pose_gt):
    """(reprojection error of the box's corners in image heights, position error in world units, rotation between the two
    camera frames in degrees, fov error in degrees)"""
    (lf, la, up, fov), (lf0, la0, up0, fov0) = pose, pose_gt
    rot = camera_frame(lf, la, up) @ camera_frame(lf0, la0, up0).T
    angle = math.degrees(math.acos(max(-1.0, min(1.0, (float(torch.trace(rot)) - 1.0) / 2.0))))
    reproj = float((project_corners(lf, la, up, fov) - project_corners(lf0, la0, up0, fov0)).square().sum(-1).mean().sqrt())
    return reproj, float((lf - lf0).norm()), angle, abs(float(fov - fov0))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=96)
    ap.add_argument("--tf-res", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=80)
    ap.add_argument("--angle", type=float, default=1.0, help="orbit angle of the ground-truth camera position (radians)")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    vol = synthetic_volume(args.vol, dev)                       # (1, D, H, W)
    tf = get_tf("tf1", args.tf_res).float().to(dev)             # (4, R)
    rc = Raycaster(vol.shape[-3:], (args.img, args.img), args.tf_res, jitter=False, max_samples=1 << 20)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    # ground truth: panned off the object's centre, rolled by ~15 degrees, zoomed in from the module's 30 to 26 degrees
    gt = (in_circles(args.angle).to(dev), t([0.15, -0.1, 0.1]), t([0.26, 0.97, 0.0]), t(26.0))
    with torch.no_grad():
        ref = rc(vol, tf, gt[0], look_at=gt[1], up=gt[2], fov=gt[3])
    # start: 6 degrees further along the orbit, looking at the centre, upright, the module's fov
    pose = [in_circles(args.angle + math.radians(6.0)).to(dev), t([0.0, 0.0, 0.0]), t([0.0, 1.0, 0.0]), t(30.0)]
    pose = [p.requires_grad_(True) for p in pose]
    # (a degree of fov moves the image about as much as 0.03 world units of look_at: its own step size)
    opt = torch.optim.Adam([{"params": pose[:3]}, {"params": pose[3:], "lr": 30.0 * args.lr}], lr=args.lr)
    errors, losses = [], []
    for i in range(args.iterations):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rc(vol, tf, pose[0], look_at=pose[1], up=pose[2], fov=pose[3]), ref)
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
