#!/usr/bin/env python3
"""The march through a pre-classified RGBA volume beside the one-tap and the seven-tap kernels of the same shape,
on the same rays, in the same process: the forward (DIFF) at sampling rate 1, the forward (NONDIFF) at rate 8 and the backward
at rates 1 and 4, and the camera gradients (cam_sr1: d look_from, pose_sr1: the ten pose parameters) at rate 1 on
the forward's live samples, each timed for
  rgba      march_rgba_fwd / _bwd / _bwd_cam / _bwd_pose, the volume = the scalar volume classified per voxel with the 1-D TF below, planar
            ((4, VX, VY, VZ) contiguous) and interleaved (channel stride 1), float32 and float16
  proj      project_fwd "sum" / project_bwd DR_VARIANT_BASELINE (one tap per sample, one channel)
  base1d    march_fwd / _bwd (volume only) with DR_VARIANT_BASELINE and the 1-D TF (seven taps per sample); for the camera
            passes march_bwd_cam / march_bwd_pose on the steps of that forward (cam1d_ms; there is no projection yardstick)
at 256^3 / 256^2 / 8 views and 512^3 / 512^2 / 1 view. Device events around windows of at least --min-seconds after a warm-up;
one JSON line per (shape, dtype, layout, pass), appended to --out. The backward times include the zeroing of d_vol (the wrappers
allocate it), for all three alike. With DIFFERENDER_HIP_LIB pointing at a build of tools/patches/rgba_per_sample.patch with
-DDR_RGBA_PER_SAMPLE (32 atomics per sample instead of the run sums; the library marks itself as a diagnostic build) and
`--passes bwd_sr1,bwd_sr4 --no-yardsticks --tag per_sample_atomics`, the same lines for that backward. GPU only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differender.utils import in_circles  # noqa: E402
from differender_amd import _native as N  # noqa: E402
from differender_amd import functional as F  # noqa: E402
from examples.render_nondiff_synthetic import synthetic_volume  # noqa: E402


def timed(fn, min_s):
    """ms per call: repeat fn in windows until one lasts >= min_s."""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1000 * min_s:
            return ms / n
        n = max(n * 2, int(n * 1000 * min_s / max(ms, 1e-3)) + 1)


def classify(vol, tf):
    """vol (VX, VY, VZ) in [0, 1], tf (R, 4) -> (VX, VY, VZ, 4), in slabs (the 512^3 intermediate would be several GB)."""
    R = tf.shape[0]
    out = torch.empty((*vol.shape, 4), device=vol.device)
    for k in range(0, vol.shape[0], 32):
        x = vol[k:k + 32].clamp(0.0, 1.0) * (R - 1)
        lo = x.floor().long().clamp(max=R - 1)
        hi = (lo + 1).clamp(max=R - 1)
        fr = (x - lo)[..., None]
        out[k:k + 32] = tf[lo] * (1.0 - fr) + tf[hi] * fr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:256:8,512:512:1", help="volume:image:views,...")
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--passes", default="fwd_diff,fwd_nondiff_sr8,bwd_sr1,bwd_sr4,cam_sr1,pose_sr1")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--tag", default="", help="recorded in every line (a what-if build)")
    ap.add_argument("--no-yardsticks", action="store_true", help="time the RGBA kernels alone")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rgba_time.jsonl"), help="append the JSON lines to this file as well ('' = no file)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/rgba_time.py needs a ROCm device"
    dev = torch.device("cuda")
    S, R = 1 << 20, 64
    passes = {"fwd_diff": (1.0, "fwd", N.DR_MODE_DIFF), "fwd_nondiff_sr8": (8.0, "fwd", N.DR_MODE_NONDIFF),
              "bwd_sr1": (1.0, "bwd", N.DR_MODE_DIFF), "bwd_sr4": (4.0, "bwd", N.DR_MODE_DIFF),
              "cam_sr1": (1.0, "cam", N.DR_MODE_DIFF), "pose_sr1": (1.0, "pose", N.DR_MODE_DIFF)}
    v = torch.linspace(0.0, 1.0, R, device=dev)
    tf1 = torch.stack([v, 1.0 - v, 0.5 + 0.0 * v, 0.4 * torch.clamp((v - 0.3) / 0.7, 0.0, 1.0) ** 2], 1).contiguous()
    lines = []
    for spec in args.shapes.split(","):
        nv, ni, V = (int(s) for s in spec.split(":"))
        vol = synthetic_volume(nv, dev)[0].permute(2, 0, 1)   # the field view (W, D, H), as Raycaster hands it over
        inter32 = classify(vol, tf1).permute(3, 0, 1, 2)     # (4, VX, VY, VZ), channel stride 1
        cam = torch.stack([in_circles(1.7 + 0.8 * i).float() for i in range(V)]).to(dev)
        WH = (ni, ni)
        g = torch.randn((V, *WH, 4), device=dev) * 1e-3
        g1 = g[..., 0].contiguous()
        for dt in args.dtypes.split(","):
            tdt = torch.float16 if dt == "f16" else torch.float32
            vols = {"interleaved": inter32.to(tdt)}
            vols["planar"] = vols["interleaved"].contiguous()
            assert vols["interleaved"].stride(-4) == 1 and vols["planar"].stride(-4) != 1   # two layouts, not one timed twice
            vol1 = vol.to(tdt)
            for tag in args.passes.split(","):
                sr, kind, mode = passes[tag]
                e, x, r, n = F.ray_setup(cam, WH, vol.shape, sr)
                fns = {}
                if kind == "fwd":
                    for lay, v4 in vols.items():
                        fns[lay] = lambda v4=v4: F.march_rgba_fwd(v4, cam, e, x, r, n, S, sr, mode=mode)
                    if not args.no_yardsticks:
                        fns["proj"] = lambda: F.project_fwd(vol1, cam, e, x, r, n, None, "sum")
                        fns["base1d"] = lambda: F.march_fwd(vol1, tf1, cam, e, x, r, n, S, sr, mode=mode,
                                                            variant=N.DR_VARIANT_BASELINE, workspace=None, hints=0)
                elif kind in ("cam", "pose"):   # (the default pose: ray_setup's buffers are ray_setup_pose's, bit for bit)
                    pose = F.pack_pose(cam)
                    for lay, v4 in vols.items():
                        out4, st4 = F.march_rgba_fwd(v4, cam, e, x, r, n, S, sr)
                        if kind == "cam":
                            fns[lay] = lambda v4=v4, out4=out4, st4=st4: F.march_rgba_bwd_cam(v4, cam, e, x, r, n, st4, S, sr, g, out4)
                        else:
                            fns[lay] = lambda v4=v4, out4=out4, st4=st4: F.march_rgba_bwd_pose(v4, pose, e, x, r, n, st4, S, sr, g, out4)
                    if not args.no_yardsticks:
                        outb, stb = F.march_fwd(vol1, tf1, cam, e, x, r, n, S, sr, variant=N.DR_VARIANT_BASELINE, workspace=None,
                                                hints=0)
                        if kind == "cam":
                            fns["cam1d"] = lambda: F.march_bwd_cam(vol1, tf1, cam, e, x, r, n, stb, S, sr, g, outb)
                        else:
                            fns["cam1d"] = lambda: F.march_bwd_pose(vol1, tf1, pose, e, x, r, n, stb, S, sr, g, outb)
                else:
                    for lay, v4 in vols.items():
                        out4, _ = F.march_rgba_fwd(v4, cam, e, x, r, n, S, sr)
                        fns[lay] = lambda v4=v4, out4=out4: F.march_rgba_bwd(v4, cam, e, x, r, n, S, sr, g, out4)
                    if not args.no_yardsticks:
                        outb, _ = F.march_fwd(vol1, tf1, cam, e, x, r, n, S, sr, variant=N.DR_VARIANT_BASELINE, workspace=None,
                                              hints=0)
                        fns["proj"] = lambda: F.project_bwd(vol1, cam, e, x, r, n, g1, None, "sum", variant=N.DR_VARIANT_BASELINE)
                        fns["base1d"] = lambda: F.march_bwd(vol1, tf1, cam, e, x, r, n, S, sr, g, outb, want_vol=True,
                                                            want_tf=False, variant=N.DR_VARIANT_BASELINE, workspace=None)
                for fn in fns.values():
                    fn(); fn()
                torch.cuda.synchronize()
                ms = {k: timed(fn, args.min_seconds) for k, fn in fns.items()}
                for lay in vols:
                    rec = {"shape": [nv, ni, V], "dtype": dt, "layout": lay, "pass": tag, "rgba_ms": ms[lay]}
                    if args.tag:
                        rec["tag"] = args.tag
                    if not args.no_yardsticks and "cam1d" in ms:
                        rec.update(cam1d_ms=ms["cam1d"], rgba_over_cam1d=ms[lay] / ms["cam1d"])
                    elif not args.no_yardsticks:
                        rec.update(proj_ms=ms["proj"], base1d_ms=ms["base1d"], rgba_over_proj=ms[lay] / ms["proj"],
                                   rgba_over_base1d=ms[lay] / ms["base1d"])
                    rec["interleaved_over_planar"] = ms["interleaved"] / ms["planar"]
                    lines.append(json.dumps(rec))
                    print(lines[-1], flush=True)
                    if args.out:
                        with open(args.out, "a") as fh:
                            fh.write(lines[-1] + "\n")
                del fns
                torch.cuda.empty_cache()
        del vol, inter32, vols, vol1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
