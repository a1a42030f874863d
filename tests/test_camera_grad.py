"""Camera-position gradient (d look_from): the C-ABI entry point and the reference that pins it. No GPU needed."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "camgrad_*.npz")))


def test_fixtures_are_there():
    import make_camgrad_golden as CG
    assert [os.path.basename(p) for p in FIXTURES] == [f"camgrad_{c}.npz" for c in sorted(CG.CASES)]


def test_entry_point_is_declared_exported_and_validates_without_gpu(hiplib):
    import ctypes
    from differender_amd import _native as N
    header = open(os.path.join(ROOT, "include", "differender_hip.h")).read()
    assert "int dr_march_bwd_cam(" in header
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "dr_march_bwd_cam")
    assert "dr_march_bwd_cam" in N.SIGNATURES and N.ABI_VERSION == 9
    f = hiplib.dr_march_bwd_cam
    P = ctypes.c_void_p(16)   # never dereferenced: validation fails first

    def call(vol=P, VX=8, n_views=1, W=8, H=8, steps=P, grad_out=P, out=P, d_cam=P, img_W=8, row0=0, sr=1.0, fov=0.5, near=0.1):
        return f(vol, 0, VX, 8, 8, 1, 8, 64, 0, P, 4, 0, P, P, P, P, P, n_views, W, H, 64, sr, fov, near, 0, 0, img_W, row0,
                 steps, grad_out, out, d_cam, None, None)
    assert call(vol=None) == -1
    assert call(steps=None) == -1
    assert call(grad_out=None) == -1
    assert call(out=None) == -1
    assert call(d_cam=None) == -1
    assert call(n_views=0) == -1
    assert call(W=0) == -1
    assert call(VX=1) == -1
    assert call(img_W=4) == -1
    assert call(row0=1) == -1
    assert call(sr=0.0) == -1
    assert call(near=0.0) == -1


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_torch_ray_setup_matches_the_oracle(oracle, path):
    import make_camgrad_golden as CG
    d = np.load(path)
    W, H = d["grad_out"].shape[:2]
    e, x, r, n = oracle.ray_setup(d["cam"], W, H, d["vol"].shape, sr=float(d["sr"]), jitter_seed=int(d["jitter_seed"]),
                                  view=int(d["view"]), dtype=np.float64)
    te, tx, tr, tn = CG.ray_setup(torch.from_numpy(d["cam"]), W, H, d["vol"].shape, float(d["sr"]),
                                  jitter_seed=int(d["jitter_seed"]), view=int(d["view"]))
    assert np.array_equal(tn.numpy().reshape(W, H), n)
    hit = n > 0
    assert np.abs(te.numpy().reshape(W, H) - e)[hit].max() <= 1e-12
    assert np.abs(tx.numpy().reshape(W, H) - x)[hit].max() <= 1e-12
    assert np.abs(tr.numpy().reshape(W, H, 3) - r)[hit].max() <= 1e-12
    assert np.array_equal(d["n"], n)


def test_cases_cover_what_they_are_named_for():
    import make_camgrad_golden as CG
    d = {os.path.basename(p)[8:-4]: np.load(p) for p in FIXTURES}
    live = lambda c: d[c]["n"] > 1
    assert ((d["b_sr2_ert"]["steps"] < d["b_sr2_ert"]["n"]) & live("b_sr2_ert")).sum() > 20
    assert (d["c_clip"]["n"] > d["c_clip"]["max_samples"]).sum() > 20
    assert int(d["d_jitter"]["jitter_seed"]) != 0
    assert d["e_nonsquare"]["n"].shape[0] != d["e_nonsquare"]["n"].shape[1]
    f = d["f_near_face"]
    t = np.minimum((-1 - f["cam"]) / f["rays"], (1 - f["cam"]) / f["rays"]).argmax(-1)[live("f_near_face")]
    assert len(np.unique(t)) >= 2   # tmin switches faces across the image
    # rays along a coordinate plane: a direction component of exactly 0 (two on the centre ray of the camera on the x axis)
    axial = lambda c: (d[c]["rays"] == 0).sum(-1) * live(c)
    assert (axial("g_plane_y0") > 0).sum() > 0 and (d["g_plane_y0"]["rays"][..., 1] == 0)[live("g_plane_y0")].sum() > 0
    assert (axial("h_plane_x0") > 0).sum() > 0 and (d["h_plane_x0"]["rays"][..., 0] == 0)[live("h_plane_x0")].sum() > 0
    assert (axial("i_on_x_axis") > 0).sum() > 0 and axial("i_on_x_axis").max() == 2
    for c in ("g_plane_y0", "h_plane_x0", "i_on_x_axis"):
        assert np.isfinite(d[c]["dcam_ray"]).all() and np.abs(d[c]["dcam_ray"][axial(c) > 0]).min() > 0
    for c in ("j_inside", "k_inside_sr2_ert"):   # the camera inside the box
        assert live(c).sum() > 0 and (d[c]["entry"][live(c)] < 0).all()
    k = d["k_inside_sr2_ert"]
    assert ((k["steps"] < k["n"]) & live("k_inside_sr2_ert")).sum() > 20 and int(k["jitter_seed"]) != 0 and float(k["sr"]) == 2.0
    sc = d["l_anisotropic"]["vol"].shape
    assert max(sc) >= 3 * min(sc)
    flat, _ = CG.sample_stats(d["m_object_in_air"], d["m_object_in_air"])
    m_live = live("m_object_in_air")
    assert flat[m_live].sum() > 0.2 * d["m_object_in_air"]["steps"][m_live].sum()
    assert (flat[m_live] < d["m_object_in_air"]["steps"][m_live]).mean() > 0.5   # and most rays meet structure as well
    assert float(d["m_object_in_air"]["tf"][0, 3]) == 0.0
    o = d["o_edge_grazing"]
    last = o["cam"] + o["exit"][..., None] * o["rays"]   # the last sample: on one face, and within a tap (1e-3) of a second
    grazing = ((1.0 - np.abs(last) < 1e-3).sum(-1) >= 2) & (np.abs(last).max(-1) - np.sort(np.abs(last), -1)[..., 1] > 2e-4)
    assert (grazing & live("o_edge_grazing")).sum() >= 6
    _, outside = CG.sample_stats(d["n_out_of_range"], d["n_out_of_range"])
    assert outside[live("n_out_of_range")].sum() > 0
    v = d["n_out_of_range"]["vol"]
    assert (v > 1).sum() >= 12 and (v < 0).sum() >= 12 and np.array_equal(np.clip(v, 0, 1)[(v >= 0) & (v <= 1)], d["a_orbit_sr1"]["vol"][(v >= 0) & (v <= 1)])


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_autograd_matches_finite_differences_of_the_f64_oracle(oracle, path):
    d = np.load(path)
    W, H = d["grad_out"].shape[:2]
    h = 1e-6
    fd = np.zeros((W, H, 3))
    same = d["n"] > 1
    for k in range(3):
        vals = []
        for sgn in (1.0, -1.0):
            cam = d["cam"].copy(); cam[k] += sgn * h
            e, x, r, n = oracle.ray_setup(cam, W, H, d["vol"].shape, sr=float(d["sr"]), jitter_seed=int(d["jitter_seed"]),
                                          view=int(d["view"]), dtype=np.float64)
            rgba, steps = oracle.march_fwd(d["vol"], d["tf"], cam, e, x, r, n, int(d["max_samples"]), float(d["sr"]), 0)
            same &= (n == d["n"]) & (steps == d["steps"])
            vals.append((np.nan_to_num(rgba) * d["grad_out"]).sum(-1))
        fd[..., k] = (vals[0] - vals[1]) / (2 * h)
    scale = np.abs(d["dcam_ray"]).max()
    err = np.abs(fd - d["dcam_ray"]).max(-1)[same]
    assert same.sum() > 0.8 * (d["n"] > 1).sum()
    assert (err <= 1e-5 * scale).mean() >= 0.99, (np.sort(err)[-5:] / scale, same.sum())


# ---- the conditioned pass of the GPU tests (camgrad_gpu.well_conditioned): its conditions, and that it bites -------------------

def _conditioned_cases():
    """Everything test_gpu_camera_grad.py and test_gpu_camera_grad_edges.py feed to the conditioned pass: id -> a function that
    returns [(ref, ref32, keep, row bands or None)]. The fixtures with the float32 volume and with its float16 rounding."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_camera_grad as TG
    import test_gpu_camera_grad_edges as TE
    cases = {}
    for p in FIXTURES:
        for f16 in (False, True):
            cases["%s_%s" % (os.path.basename(p)[8:-4], "f16" if f16 else "f32")] = \
                lambda p=p, f16=f16: [TG.fixture_case(p, f16)[1:] + (None,)]
    cases.update(TE.CONDITIONED)
    return cases


CONDITIONED = _conditioned_cases()


@pytest.mark.parametrize("case", sorted(CONDITIONED))
def test_cases_keep_enough_well_conditioned_rays(case):
    """The rays on which the float32 and the float64 reference agree to 1e-4 of the scale are at least 80 % of the n > 1 rays
    (in every row band where the rule is applied band by band), and err32 over them is within 1e-4 of the scale: the second
    pass of the GPU tests then bounds every ray by 4e-4 of it."""
    import camgrad_gpu as K
    K.check_conditions(CONDITIONED[case]())


def test_grazing_cases_keep_their_grazing_rays_well_conditioned():
    import test_gpu_camera_grad_edges as TE
    for name in sorted(TE.GRAZING):
        inp, ref, ref32 = TE._grazing_case(name)
        assert (TE._grazing_rays(name, inp, ref) & TE._good(ref, ref32)).sum() >= 6, name


def test_the_conditioned_rule_rejects_a_one_percent_error():
    """a_orbit_sr1: one ray next to a lighting kink puts err32 at 3 % of the scale, and D8's rule over all rays accepts a
    gradient that is 1 % off everywhere. Over the well-conditioned rays it does not."""
    import camgrad_gpu as K
    import test_gpu_camera_grad as TG
    path = os.path.join(GOLDEN, "camgrad_a_orbit_sr1.npz")
    for f16 in (False, True):
        _, ref, ref32, keep = TG.fixture_case(path, f16)
        good = K.well_conditioned(ref, ref32, keep)
        assert good.sum() < (keep & (ref["n"] > 1)).sum()   # there are ill-conditioned rays to leave out
        K.mutation_check(K.d8_rule, ref["dcam_ray"], ref32["dcam_ray"], ref, ref32, keep, good)


def test_generator_reproduces_its_fixture():
    import make_camgrad_golden as CG
    name = "d_jitter"
    d = np.load(os.path.join(GOLDEN, f"camgrad_{name}.npz"))
    inp = CG.make_inputs(name)
    for k in inp:
        assert np.array_equal(inp[k], d[k]), k
    res = CG.run_case(inp)
    assert np.array_equal(res["n"], d["n"]) and np.array_equal(res["steps"], d["steps"])
    assert np.allclose(res["dcam_ray"], d["dcam_ray"], rtol=0, atol=1e-12 * np.abs(d["dcam_ray"]).max())
