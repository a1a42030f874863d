#!/usr/bin/env python3
"""Inverse lighting: recover a light and a Phong material from renders.
The targets are rendered through differender_amd.lighting.RaycasterLit with a warm light off to the side of the volume, fixed
in the world, and a glossy material; starting from the reference's white headlight-like light above the volume and its
material (0.4 / 0.8 / 0.3 / 32), the light's position and colour and the four material scalars are then fitted to the targets
by torch.optim.Adam -- the volume and the transfer function stay as they are.
Prints the first and the last loss, and each parameter group's distance from the truth at the start and at the end."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd.lighting import RaycasterLit  # noqa: E402

TRUTH = dict(light_pos=(2.2, 1.4, -1.3), light_color=(1.0, 0.75, 0.5), ambient=0.2, diffuse=0.65, specular=0.55, shininess=10.0)
START = dict(light_pos=(0.0, 2.5, 0.5), light_color=(0.8, 0.8, 0.8), ambient=0.4, diffuse=0.8, specular=0.3, shininess=32.0)
GROUPS = dict(position=("light_pos",), colour=("light_color",), material=("ambient", "diffuse", "specular", "shininess"))


def bumpy_ball(n, dev):
    """(1, n, n, n): a ball of radius ~0.7 with a rippled surface (normals in every direction), edges smoothed over ~1.5 voxels."""
    c = torch.linspace(-1.0, 1.0, n, device=dev)
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    ripple = 0.06 * torch.sin(7.0 * x) * torch.sin(6.0 * y + 0.5) * torch.sin(8.0 * z + 1.0)
    return torch.sigmoid((0.7 + ripple - r) / (1.5 * 2.0 / (n - 1)))[None]


def surface_tf(R, dev):
    """(4, R): nothing below value 0.3, then a grey-green surface that turns opaque quickly."""
    v = torch.linspace(0.0, 1.0, R, device=dev)
    a = torch.clamp((v - 0.3) / 0.4, 0.0, 1.0) * 0.6
    return torch.stack([0.7 + 0.0 * v, 0.8 + 0.0 * v, 0.7 + 0.0 * v, a], 0)


def distance(params, names):
    """Relative distance of the named parameters from the truth (each by its own magnitude)."""
    d = [torch.linalg.vector_norm(params[k].detach().cpu() - torch.tensor(TRUTH[k])) / torch.linalg.vector_norm(torch.tensor(TRUTH[k]))
         for k in names]
    return float(torch.stack(d).max())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a 32^3 volume, 32x32 images, 3 views: seconds")
    ap.add_argument("--vol", type=int, default=96)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--lr", type=float, default=0.03)
    args = ap.parse_args()
    if args.small:
        args.vol, args.img, args.views = 32, 32, 3
    dev = torch.device("cuda")
    torch.manual_seed(0)
    R = 32
    vol, tf = bumpy_ball(args.vol, dev), surface_tf(R, dev)
    rc = RaycasterLit(vol.shape[-3:], (args.img, args.img), R, sampling_rate=1.0, jitter=False, headlight=False)
    cams = torch.stack([in_circles(0.9 + 6.28 * i / args.views).float() for i in range(args.views)]).to(dev)
    with torch.no_grad():
        targets = rc(vol, tf, cams, **{k: torch.tensor(v, device=dev) for k, v in TRUTH.items()})
    params = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in START.items()}
    # (the shininess lives on a scale of tens, the position of units, the rest of tenths: each steps by its own scale)
    opt = torch.optim.Adam([dict(params=[params[k]], lr=args.lr * s) for k, s in
                            (("light_pos", 3.0), ("light_color", 1.0), ("ambient", 1.0), ("diffuse", 1.0), ("specular", 1.0),
                             ("shininess", 20.0))])
    start = {g: distance(params, names) for g, names in GROUPS.items()}
    losses = []
    for i in range(args.iters):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(rc(vol, tf, cams, **params), targets)
        loss.backward()
        opt.step()
        with torch.no_grad():
            params["shininess"].clamp_(min=1.0)
            for k in ("light_color", "ambient", "diffuse", "specular"):
                params[k].clamp_(min=0.0)
        losses.append(loss.detach())
        if i % 50 == 0 or i == args.iters - 1:
            print(f"[{i:04d}] loss {float(loss):.6e}")
    print(f"first loss {float(losses[0]):.6e}")
    print(f"last loss {float(losses[-1]):.6e}")
    for g, names in GROUPS.items():
        print(f"{g} error {start[g]:.4f} -> {distance(params, names):.4f}")
    for k, p in params.items():
        print(f"  {k}: {[round(float(x), 3) for x in p.detach().reshape(-1)]}  (truth {TRUTH[k]})")
