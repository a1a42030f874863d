"""The fused 3-D total variation on the GPU (tv_loss.hip) against tv3d in float64, with the D8 tolerance rule
(3x what torch's own float32 evaluation is off by, with a floor); strided inputs, determinism, accumulate / upstream / scale,
the full 512^3 size, the renderer, a denoising trajectory and the example."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

import tv_gpu
from differender_amd import functional as F
from differender_amd.utils import fused_tv3d_loss, tv3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NORMS = tv_gpu.NORMS
_check, _vol = tv_gpu.check, tv_gpu.volume   # (shared with test_gpu_tv_edges.py)


SHAPES = [(1, 1, 1, 1), (1, 1, 2, 3), (2, 1, 5, 33, 65), (1, 37, 129, 70), (1, 1, 64, 64, 64), (3, 17, 1, 9), (1, 70, 18, 5)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("norm,eps", NORMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_matches_float64_tv3d(shape, norm, eps, dtype):
    _check(_vol(shape, seed=len(shape), dtype=dtype), norm, eps)


@pytest.mark.parametrize("norm,eps", NORMS)
def test_constant_regions_and_sum(norm, eps):
    vol = _vol((2, 1, 20, 35, 67), seed=3, flat=True)
    _check(vol, norm, eps, reduction="sum")
    _check(vol, norm, eps, reduction="mean")


def _strided(kind):
    g = torch.Generator().manual_seed(11)
    if kind == "raycaster":     # Raycaster's (W, D, H) view of the user's (1, D, H, W) volume
        return torch.rand(1, 40, 50, 68, generator=g).to(DEV).squeeze(0).permute(2, 0, 1)
    if kind == "sliced":
        return torch.rand(1, 30, 40, 140, generator=g).to(DEV)[..., ::2]
    if kind == "batch_last":    # batch axis of stride 1
        return torch.rand(1, 20, 24, 36, 3, generator=g).to(DEV).permute(4, 0, 1, 2, 3)
    if kind == "transposed_batch":   # leading axes that do not collapse into one stride
        return torch.rand(3, 2, 9, 21, 70, generator=g).to(DEV).transpose(0, 1)
    if kind == "offset":        # a storage offset that breaks the 16-byte alignment
        return torch.rand(1 + 8 * 9 * 68, generator=g).to(DEV)[1:].view(1, 8, 9, 68)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["raycaster", "sliced", "batch_last", "transposed_batch", "offset"])
@pytest.mark.parametrize("norm,eps", [("l1", 1e-3), ("iso", 1e-2), ("sq", 1e-3)])
def test_strided_equals_contiguous(kind, norm, eps):
    vol = _strided(kind)
    got = []
    for v in (vol, vol.contiguous()):
        v = v.detach().clone() if v is not vol else v.detach()
        v = v.requires_grad_(True)
        loss = fused_tv3d_loss(v, norm, eps)
        loss.backward()
        got.append((float(loss.detach()), v.grad.clone()))
    (l0, g0), (l1, g1) = got
    assert abs(l0 - l1) <= 1e-6 * abs(l1)
    assert float((g0 - g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    _check(vol, norm, eps, loss=torch.tensor(l0), grad=g0)


@pytest.mark.parametrize("norm,eps", NORMS)
def test_deterministic_accumulate_upstream(norm, eps):
    vol = _vol((2, 1, 21, 50, 77), seed=5)
    s0, s1 = F.tv3d_fwd(vol, norm, eps), F.tv3d_fwd(vol, norm, eps)
    assert abs(float(s0) - float(s1)) <= 1e-12 * abs(float(s0))
    a = F.tv3d_bwd(vol, norm=norm, eps=eps)
    b = F.tv3d_bwd(vol, norm=norm, eps=eps)
    assert torch.equal(a, b)
    grad0 = torch.randn(vol.shape, device=DEV)
    out = grad0.clone()
    F.tv3d_bwd(vol, norm=norm, eps=eps, out=out, accumulate=True)
    assert torch.equal(out, grad0 + a)
    up = torch.tensor(2.5, device=DEV)
    scaled = F.tv3d_bwd(vol, upstream=up, scale=0.125, norm=norm, eps=eps)
    assert float((scaled - 0.3125 * a).abs().max()) <= 1e-6 * float(0.3125 * a.abs().max())
    v = vol.clone().requires_grad_(True)
    (2.5 * fused_tv3d_loss(v, norm, eps)).backward()
    want = 2.5 / vol.numel() * a
    assert float((v.grad - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_nan_gives_nan_sum():
    vol = _vol((1, 9, 10, 11))
    vol[0, 4, 5, 6] = float("nan")
    for norm in ("l1", "iso", "sq"):
        assert torch.isnan(F.tv3d_fwd(vol, norm, 1e-2))


def test_errors():
    vol = _vol((1, 4, 5, 6))
    with pytest.raises(TypeError):
        fused_tv3d_loss(vol.double())
    with pytest.raises(ValueError):
        fused_tv3d_loss(vol[0, 0])
    with pytest.raises(ValueError):
        fused_tv3d_loss(vol, "iso", eps=0.0)
    with pytest.raises(ValueError):
        F.tv3d_bwd(vol, out=torch.zeros(100, device=DEV).as_strided(vol.shape, (0, 6, 1, 1)))   # overlapping elements


@pytest.mark.parametrize("norm,eps", [("l1", 1e-3), ("iso", 1e-2), ("sq", 1e-3)])
def test_full_size_512(norm, eps):
    g = torch.Generator(device=DEV).manual_seed(0)
    vol = torch.rand((1, 512, 512, 512), device=DEV, generator=g)
    _check(vol, norm, eps, device=DEV)
    torch.cuda.empty_cache()


def test_through_the_renderer():
    from differender_amd.volume_raycaster import Raycaster
    from differender.utils import get_tf, in_circles
    from examples.render_nondiff_synthetic import synthetic_volume
    vol0 = synthetic_volume(48, DEV)
    rc = Raycaster(vol0.shape[-3:], (64, 64), 64, jitter=False, max_samples=2048)
    cams = torch.stack([in_circles(0.4), in_circles(2.1)]).float().to(DEV)
    with torch.no_grad():
        gt = rc(vol0, get_tf("tf1", 64).to(DEV).float(), cams).detach()
    lam = 0.5
    noisy = (vol0 + 0.05 * torch.randn(vol0.shape, generator=torch.Generator().manual_seed(0)).to(DEV)).clamp(0, 1)
    grads = []
    for with_tv in (False, True):
        vol = noisy.clone().float().requires_grad_(True)
        tf = get_tf("gray", 64).to(DEV).float()
        loss = TF.mse_loss(rc(vol, tf, cams), gt)
        if with_tv:
            loss = loss + lam * fused_tv3d_loss(vol, "iso", 1e-2)
        loss.backward()
        grads.append(vol.grad.clone())
    tv_grad = F.tv3d_bwd(noisy.float(), scale=1.0 / noisy.numel(), norm="iso", eps=1e-2)
    want = grads[0] + lam * tv_grad
    scale = max(float(grads[0].abs().max()), float((lam * tv_grad).abs().max()))
    assert float((grads[1] - want).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize("norm,lam", [("l1", 0.2), ("iso", 0.2), ("sq", 0.3)])
def test_denoising_trajectory(norm, lam):
    from examples.render_nondiff_synthetic import synthetic_volume
    clean = synthetic_volume(64, DEV)
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(clean.shape, generator=g) < 0.05).to(DEV)
    salt = torch.rand(clean.shape, generator=g).to(DEV)
    noisy = torch.where(mask, salt, clean)
    finals = []
    for tv in (tv3d, fused_tv3d_loss):
        v = noisy.clone().requires_grad_(True)
        opt = torch.optim.Adam([v], lr=1e-2)
        for _ in range(200):
            opt.zero_grad()
            loss = TF.mse_loss(v, noisy) + lam * tv(v, norm, 1e-2)
            loss.backward()
            opt.step()
        finals.append(v.detach())
    e0 = float(TF.mse_loss(noisy, clean))
    e_torch, e_hip = (float(TF.mse_loss(f, clean)) for f in finals)
    assert e_hip < 0.5 * e0, (e0, e_hip)
    assert abs(e_hip - e_torch) <= 0.02 * e_torch, (e_hip, e_torch)
    # with "l1" Adam turns last-bit differences of the sign fluxes into oscillations of the step size: the two trajectories
    # agree to well within it
    assert float((finals[0] - finals[1]).abs().mean()) <= 0.5e-2


def test_example_tv_beats_no_tv():
    errs = []
    for lam in ("1.0", "0"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "vol_denoise_tv_synthetic.py"), "--vol", "48",
                            "--img", "96", "--iterations", "40", "--lr", "1e-2", "--lam", lam],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        m = re.search(r"volume mse to vol_gt \(lam [^)]*\): (\S+) -> (\S+)", r.stdout)
        assert m, r.stdout[-2000:]
        errs.append((float(m.group(1)), float(m.group(2))))
    (a0, a1), (b0, b1) = errs
    assert a0 == b0
    assert a1 < b1, errs
