"""DESIGN.md D4, the dim-behind-bright case: samples of ORDINARY opacity (>= DR_D4_TINY_OP) whose TF colour is so dark that,
behind a bright shell, each one adds less than half an ulp to the running colour (oracle.dark_shell_scene). The reference's
sequential float32 loop (VR.py:300-302; the oracle) drops every one of them; the brick kernels' partials keep them. Per ray that is
up to a few 1e-5 -- above the 1e-5 bar -- so the per-ray passes must see it in their bound and recompute those rays sample by
sample (F3), and take their backward from the sequential composites (B3) where the bound says so.

Each case first checks its own premise on the CPU: some pixel whose step counts agree is more than 1e-5 away from the same march
composited in double (oracle.march_fwd(accum64=True), what summing the samples first comes close to). A scene that stopped showing
the effect would make the case pointless: it fails instead of passing quietly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
S = 1 << 20
WH = (48, 48)
R = 64


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def grad_close(a, b, tol=GRAD_TOL):
    scale = max(float(np.abs(b).max()), 1e-12)
    err = float(np.abs(a - b).max()) / scale
    return err <= tol, err


# 96^3, noisy body: 1.007e-5 / 1.001e-5 on the worst pixel (modes 0 / 1) -- segments whose mean the lit samples lift above half an
# ulp keep their dim samples out of the bound ("Not covered"; the brick passes would have to count such samples)
_MIXED = pytest.mark.xfail(reason="D4 does not cover dim samples in segments whose mean is above half an ulp", strict=False)
CASES = [(96, 8.0, "flat", False), pytest.param((96, 8.0, "noisy", False), marks=_MIXED), (96, 8.0, "rounded", False),
         (192, 4.0, "flat", False), (192, 4.0, "noisy", False), (192, 8.0, "flat", False), (192, 8.0, "rounded", False),
         (192, 4.0, "flat", True)]


def _id(c):
    c = c.values[0] if hasattr(c, "values") else c
    return f"{c[0]}^3-sr{c[1]:g}-{c[2]}" + ("-f16" if c[3] else "")


@pytest.mark.parametrize("mode", [0, 1], ids=["diff", "nondiff"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dim_samples_behind_a_bright_shell_D4(oracle, hiplib, case, mode):
    from differender_amd import functional as Fn
    N, sr, body, f16 = case
    vol_h, tf_h = oracle.dark_shell_scene(N, sr, body)
    vol_o = vol_h.astype(np.float16).astype(np.float32) if f16 else vol_h   # what the kernels read from an f16 volume
    vol = T(vol_h.astype(np.float16)) if f16 else T(vol_h)
    cam_h = oracle.in_circles(2.1)
    e0, x0, r0, n0 = oracle.ray_setup(cam_h, *WH, vol_h.shape, sr=sr)
    ref, sref = oracle.march_fwd(vol_o, tf_h, cam_h, e0, x0, r0, n0, S, sr, mode)
    acc, sacc = oracle.march_fwd(vol_o, tf_h, cam_h, e0, x0, r0, n0, S, sr, mode, accum64=True)
    same = sref == sacc
    gap = np.abs(ref - acc).max(-1)[same]
    assert gap.max() > FWD_TOL, f"premise: the sequential rounding moves no pixel beyond the bar ({gap.max():.3g})"

    tf, cam = T(tf_h), T(cam_h[None])
    e, x, r, n = Fn.ray_setup(cam, WH, vol_h.shape, sr)
    assert np.array_equal(n[0].cpu().numpy(), n0)
    ws = Fn.alloc_workspace(1, WH, vol_h.shape, R, dev())
    out, steps = Fn.march_fwd(vol, tf, cam, e, x, r, n, S, sr, mode, workspace=ws)
    st = Fn.workspace_stats(ws)
    assert np.array_equal(steps[0].cpu().numpy(), sref), int((steps[0].cpu().numpy() != sref).sum())
    d = float(np.abs(out[0].cpu().numpy() - ref).max())
    assert d <= FWD_TOL, d
    assert int(st[0]) == 0, "rays failed their sample count and were marched one by one"
    assert int(st[15]) > 0, "no ray went through the exact pass (F3)"
    if mode == 1:
        return

    # gradients of the same call against the oracle's adjoint of the sequential march (VR.py:460-461,470-471)
    g = np.random.RandomState(N + int(sr)).randn(*WH, 4).astype(np.float32)
    dv0, dt0 = oracle.march_bwd(vol_o, tf_h, cam_h, e0, x0, r0, n0, S, sr, g)
    dv, dt = Fn.march_bwd(vol, tf, cam, e, x, r, n, S, sr, T(g[None]), out, workspace=ws)
    ok, err = grad_close(dv.float().cpu().numpy(), dv0); assert ok, ("d_volume", err)
    ok, err = grad_close(dt.cpu().numpy(), dt0); assert ok, ("d_tf", err)
    # the TF-only backward, from the brick workspace ...
    out_b, _ = Fn.march_fwd(vol, tf, cam, e, x, r, n, S, sr, workspace=ws)
    _, dt_b = Fn.march_bwd(vol, tf, cam, e, x, r, n, S, sr, T(g[None]), out_b, want_vol=False, workspace=ws)
    ok, err = grad_close(dt_b.cpu().numpy(), dt0); assert ok, ("d_tf, TF only", err)
    # ... and over the per-sample tape (DR_TAPE_TF)
    ws_t = Fn.alloc_workspace(1, WH, vol_h.shape, R, dev(), tape=(S, sr))
    out_t, steps_t = Fn.march_fwd(vol, tf, cam, e, x, r, n, S, sr, workspace=ws_t, tape=True)
    assert np.array_equal(steps_t[0].cpu().numpy(), sref)
    assert float(np.abs(out_t[0].cpu().numpy() - ref).max()) <= FWD_TOL
    _, dt_t = Fn.march_bwd(vol, tf, cam, e, x, r, n, S, sr, T(g[None]), out_t, want_vol=False, workspace=ws_t, tape=True)
    assert int(Fn.workspace_stats(ws_t)[9]) == 0, "the tape backward did not find its forward's tape"
    ok, err = grad_close(dt_t.cpu().numpy(), dt0); assert ok, ("d_tf, tape", err)
