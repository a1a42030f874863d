"""bench.py --dump-outputs on a small configuration: the files hold what the LAST timed step computed (its image, sample counts and
gradients, recomputed here through the same calls for that step's camera -- every step has its own camera), and the result line
reports the timed steps it was asked for. A plain run leaves the untimed extras out; --full runs them."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, IMG, R, WARMUP, STEPS = 64, 64, 32, 1, 3


def test_dump_outputs_hold_the_last_timed_step(hiplib, tmp_path):
    import bench
    from differender_amd import functional as F
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--vol", str(N), "--img", str(IMG), "--tf-res", str(R),
           "--steps", str(STEPS), "--warmup", str(WARMUP), "--no-cpu-baseline", "--pmc", "off", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    files = line["dumped_outputs"]["files"]
    assert set(files) == {"image.npy", "sample_counts.npy", "d_volume.npy", "d_tf.npy"}
    got = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float32 and list(a.shape) == files[f + ".npy"] for f, a in got.items())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES

    # the last timed step, through the same calls (bench.main's inputs: seeded volume and target, constant-alpha TF)
    dev = torch.device("cuda:0")
    vol = bench.synth_volume_torch(N, dev)
    tf = bench.bench_tf_torch(R, 3.0 / (2.0 * math.sqrt(3.0) * math.sqrt(3.0) * (N - 1)), dev)
    target = torch.rand((1, IMG, IMG, 4), generator=torch.Generator(device="cpu").manual_seed(4321)).to(dev)
    ws = F.alloc_workspace(1, (IMG, IMG), (N, N, N), R, dev)

    def render(k):
        cam = torch.tensor([bench.in_circles(0.1 * k)], dtype=torch.float32, device=dev)
        e, x, r, n = F.ray_setup(cam, (IMG, IMG), (N, N, N), 1.0, view_base=k)
        out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, 1 << 20, 1.0, workspace=ws)
        return cam, (e, x, r, n), out, steps

    k = WARMUP + STEPS - 1
    cam, rays, out, steps = render(k)
    _, grad_out = F.mse_loss_grad(out, target)
    dv, dt = F.march_bwd(vol, tf, cam, *rays, 1 << 20, 1.0, grad_out, out, workspace=ws)
    torch.cuda.synchronize()
    err = float(np.abs(got["image"] - out.cpu().numpy()).max())
    assert err <= 1e-5, err
    assert np.array_equal(got["sample_counts"], steps.cpu().numpy().astype(np.float32))
    dv, dt = dv.cpu().numpy(), dt.cpu().numpy()
    assert np.abs(got["d_volume"] - dv).max() <= 1e-5 * np.abs(dv).max() and np.abs(dv).max() > 0
    assert np.abs(got["d_tf"] - dt).max() <= 1e-5 * np.abs(dt).max() and np.abs(dt).max() > 0
    # ... and not an earlier step's: the camera of step k - 1 renders a visibly different image
    prev = render(k - 1)[2].cpu().numpy()
    assert float(np.abs(got["image"] - prev).max()) > 100 * max(err, 1e-6)


def test_plain_run_stops_at_the_headline_and_full_adds_the_rest(hiplib, tmp_path):
    """A plain run times its steps and prints the line, nothing more; --full adds the evaluated-sample step and the CPU
    baseline with its parity check (at this size --pmc auto collects no counters either way). Both time the same work."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--vol", str(N), "--img", str(IMG), "--tf-res", str(R),
            "--steps", str(STEPS), "--warmup", str(WARMUP)]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        out = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, p.stdout
        lines[name] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["roofline_fwd"]["avg_launch_ms"] > 0 and line["roofline_bwd"]["avg_launch_ms"] > 0
    assert plain["voxel_steps_per_step"] == full["voxel_steps_per_step"] > 0
    assert plain["evaluated_voxel_steps"] is None and plain["cpu_baseline"] is None and plain["traffic_source"] is None
    ev = full["evaluated_voxel_steps"]
    assert ev["marched"] > 0 and ev["march_fwd"] > 0 and ev["march_bwd"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["parity_vs_gpu"]["within_north_star_bars"]
    assert full["traffic_source"] is None
