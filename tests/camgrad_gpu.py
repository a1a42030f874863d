"""What the GPU tests of the camera gradient share (test_gpu_camera_grad.py, test_gpu_camera_grad_edges.py): one launch of
F.march_fwd + F.march_bwd_cam on the ray buffers of the float64 reference (tests/golden/make_camgrad_golden.py), and D8's rule."""
import math

import numpy as np
import torch


def launch(vol, tf, cams, refs, grad_outs, keeps, S, sr, seed=0, view_base=0, rows=None, upstream=None):
    """One launch over len(refs) views. vol, tf: device tensors as the kernels get them (shared or one item per view); cams
    (V, 3); refs: per view the reference's entry, exit, rays, n, steps; grad_outs (W, H, 4) and keeps (W, H) per view: only the
    rays in `keep` whose march stops where the reference's does get an upstream gradient. upstream: a function of the masked
    (V, W, H, 4) device tensor that returns the tensor to hand in instead.
    -> per-ray d_cam (V, W, H, 3) float64, totals (V, 3) float64, masks (V, W, H), the upstream gradient handed in."""
    from differender_amd import functional as F
    dev = torch.device("cuda")
    T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    stack = lambda k, dt=torch.float32: T(np.stack([np.asarray(r[k]) for r in refs]), dt)
    cam = T(np.asarray(cams, np.float64).reshape(-1, 3))
    e, x, r, n = stack("entry"), stack("exit"), stack("rays"), stack("n", torch.int32)
    out, steps = F.march_fwd(vol, tf, cam, e, x, r, n, S, sr, rows=rows)
    got = steps.cpu().numpy()
    masks = np.stack([(got[v] == refs[v]["steps"]) & (refs[v]["n"] > 1) & keeps[v] for v in range(len(refs))])
    # rays whose f32 march stops elsewhere, and n == 1 rays: zero upstream
    g = T(np.stack([grad_outs[v] * masks[v][..., None] for v in range(len(refs))]))
    if upstream is not None:
        g = upstream(g)
    d, d_ray = F.march_bwd_cam(vol, tf, cam, e, x, r, n, steps, S, sr, g, out, jitter_seed=seed, view_base=view_base, rows=rows,
                               per_ray=True)
    torch.cuda.synchronize()
    return d_ray.double().cpu().numpy(), d.double().cpu().numpy(), masks, g


def hip_per_ray(inp, ref, vol_dtype, keep):
    """(per-ray d_cam (W,H,3), total (3,), mask of the compared rays) of F.march_bwd_cam on the reference's ray buffers; only
    the rays in `keep` get an upstream gradient."""
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float32)
    ray, total, mask, _ = launch(T(inp["vol"]).to(vol_dtype), T(inp["tf"]), inp["cam"], [ref], [inp["grad_out"]], [keep],
                                 int(inp["max_samples"]), float(inp["sr"]), int(inp["jitter_seed"]), int(inp["view"]))
    return ray[0], total[0], mask[0]


FLOOR = 1e-4   # the rule's own floor: the share of the scale every ray is allowed on top of 3 err32
LOOK_FROM = (("look_from", slice(0, 3)),)


def _shading(vol, look_from, ref, dtype):
    """The lighting of every live sample of the reference's march, evaluated in `dtype` on that reference's own ray buffers
    (make_autograd_golden's sample positions, trilinear sample and lighting literals; the outputs are this diagnostic's own): per
    sample (S, P) the norm of the central differences, the unit normal (S, P, 3), n.l, max(r.v, 0), L before min(1, .), and `lit`: live and not flat (D1)."""
    import make_autograd_golden as G
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)
    v, cam = T(vol), T(look_from)
    e, x, r = T(ref["entry"]).reshape(-1), T(ref["exit"]).reshape(-1), T(ref["rays"]).reshape(-1, 3)
    n, steps = torch.from_numpy(ref["n"].reshape(-1)).long(), torch.from_numpy(ref["steps"].reshape(-1)).long()
    light = G.light_position(cam)
    out = {k: [] for k in ("lit", "norm", "nrm", "ndl", "rdv", "L")}
    for s in range(int(steps.max()) if len(steps) else 0):
        live = (s < steps) & (n > 1)
        pos = G.sample_pos(cam, e, x, r, n, s, live)
        g = torch.stack([G.sample_volume_trilinear(v, pos + ax) - G.sample_volume_trilinear(v, pos - ax)
                         for ax in 1e-3 * torch.eye(3, dtype=dtype)], 1)
        norm = g.norm(dim=1)
        lit = live & (norm > 0)
        nrm = g / torch.where(lit, norm, torch.ones_like(norm))[:, None]
        ld = pos - light[None]
        ld = ld / ld.norm(dim=1, keepdim=True)
        ndl = (nrm * ld).sum(1)
        rdv = ((ld - 2.0 * ndl[:, None] * nrm) * (-r)).sum(1).clamp(min=0.0)
        L = G.DIFFUSE * ndl.clamp(min=0.0) + G.SPECULAR * rdv ** G.SHININESS + G.AMBIENT
        for k, t in (("lit", lit), ("norm", norm), ("nrm", nrm), ("ndl", ndl), ("rdv", rdv), ("L", L)):
            out[k].append(t if k == "lit" else t.double())
    return {k: torch.stack(t) for k, t in out.items()} if out["lit"] else None


def near_lighting_kink(vol, look_from, ref):
    """The rays with a live sample whose float64 shading lies within float32 rounding of a kink of D7 -- max(n.l, 0) or
    min(1, L) -- from the float64 reference alone. On such a ray any float32 evaluation may take the other branch; where the
    transliteration happens to follow float64 and the kernel does not, err32 says nothing about the kernel's error (measured
    on the MI355X: one ray in each of five cases, the kernel 2e-3 ... 7e-3 of the scale off, the transliteration 1e-5).
    The bound, from float32's spacing and first order: a tap's value good to one ulp (2^-24 below 1, the spacing under
    max|vol| otherwise), a central difference of two taps to 2 ulp, the vector g of the three differences to sqrt(3) 2 ulp,
    the unit normal g / |g| to dn = sqrt(3) 2 ulp / |g| (the taps are 2e-3 apart: |g| is small), n.l with |l| = 1 to dn,
    r = l - 2 (n.l) n and r.v to 4 dn, and L = 0.8 max(n.l, 0) + 0.3 max(r.v, 0)^32 + 0.4 to (0.8 + 0.3 * 32 *
    max(r.v, 0)^31 * 4) dn. A sample is near a kink iff |n.l| <= dn or |L - 1| <= that. One ulp per tap is what a float32
    evaluation typically makes, not a worst case: the transliteration's own |normal32 - normal64| |g| has its median at
    2.5e-8 and its 99th percentile at 1.3e-7 ... 5.7e-7 over the cases here, around sqrt(3) 2 ulp = 2.1e-7.
    max(r.v, 0)^32 is no kink (31 continuous derivatives at 0); flat samples (D1) have no normal.
    vol: the volume the kernel reads; ref: entry, exit, rays, n, steps of the float64 reference. -> mask (W, H)."""
    import make_autograd_golden as G
    W, H = ref["n"].shape
    a = _shading(vol, look_from, ref, torch.float64)
    if a is None:
        return np.zeros((W, H), bool)
    top = np.float32(max(1.0, float(np.abs(vol).max())))
    ulp = float(top - np.nextafter(top, np.float32(0.0)))
    dn = math.sqrt(3.0) * 2.0 * ulp / torch.where(a["lit"], a["norm"], torch.ones_like(a["norm"]))
    slope = G.DIFFUSE + G.SPECULAR * G.SHININESS * 4.0 * a["rdv"] ** (G.SHININESS - 1.0)
    near = a["lit"] & ((a["ndl"].abs() <= dn) | ((a["L"] - 1.0).abs() <= slope * dn))
    return near.any(0).numpy().reshape(W, H)


def with_kinks(inp, ref, cam_key="cam"):
    """The float64 reference of a lit march with near_lighting_kink's mask under "near_kink", where well_conditioned reads it."""
    return dict(ref, near_kink=near_lighting_kink(inp["vol"], inp[cam_key], ref))


def well_conditioned(ref, ref32, keep, key="dcam_ray", columns=LOOK_FROM, what=None, lit=True):
    """The rays on which the two references agree, from the references alone: for each tensor T of `columns`, scale_T is the
    largest |float64 component| over the kept n > 1 rays, and a ray is good iff its float32 transliteration is within
    FLOOR * scale_T of the float64 one in every column of every T. On the others (a ray within rounding distance of a frozen
    switch: a lighting kink of D7, a tap's cell, a slab face) the float32 program itself is percents off, and err32, a maximum
    over all compared rays, would excuse every ray. lit (the TF march, not the RGBA one): the rays of ref["near_kink"]
    (with_kinks) are left out too -- there the float32 transliteration is right by luck. The case must keep 80 % of its
    n > 1 rays, d8_rule's own cap. -> mask (W, H), a subset of keep & (n > 1)."""
    live = ref["n"] > 1
    base = keep & live
    assert base.any(), "ill-conditioned case: move the camera"
    good = base & ~ref["near_kink"] if lit else base.copy()
    for _, sl in columns:
        want = ref[key][..., sl]
        good &= np.abs(ref32[key][..., sl] - want).max(-1) <= FLOOR * np.abs(want[base]).max()
    if what is not None:
        print("conditioned", what, "good %d of %d n > 1 rays" % (good.sum(), live.sum()), "err32/scale_T",
              " ".join("%s %.3g" % (name, conditioned_err32(ref, ref32, keep, good, key, sl)) for name, sl in columns))
    assert good.sum() >= 0.8 * live.sum(), ("ill-conditioned case: move the camera", what, good.sum(), live.sum())
    return good


def conditioned_err32(ref, ref32, keep, good, key, sl):
    """err32 over the good rays as a share of scale_T, the scale well_conditioned judged them by. (d8_rule prints err32 over
    its own scale, the largest component of the rays it compares, which is smaller once the steepest rays -- the ones next to
    a kink -- are gone.)"""
    want = ref[key][..., sl]
    err, scale = np.abs(ref32[key][..., sl] - want)[good].max(), np.abs(want[keep & (ref["n"] > 1)]).max()
    return err / scale if scale > 0 else (0.0 if err == 0 else np.inf)   # (d up and d fov of a centre ray are exactly 0)


def check_conditions(entries, key="dcam_ray", columns=LOOK_FROM, lit=True):
    """What a case owes the conditioned pass, checked from the references alone (no GPU): for each (ref, ref32, keep, row
    bands or None) the 80 % cap of well_conditioned -- in every band too, where d8_rule is applied band by band -- and err32 over
    the good rays within FLOOR of each tensor's scale."""
    for ref, ref32, keep, bands in entries:
        good = well_conditioned(ref, ref32, keep, key, columns, lit=lit)
        assert not (good & ~(keep & (ref["n"] > 1))).any()
        for _, sl in columns:
            assert conditioned_err32(ref, ref32, keep, good, key, sl) <= FLOOR
        for rows in bands or ():
            assert good[rows].sum() > 0.8 * (ref["n"][rows] > 1).sum(), ("ill-conditioned band: move the camera", rows)


def mutation_check(rule, ray64, ray32, ref, ref32, keep, good):
    """That the conditioned pass bites, with arrays in the kernel's place: with every per-ray gradient 1 % too large, and the
    total their sum, the rule over all kept rays passes and the rule over the well-conditioned ones raises; with the float32
    reference as the answer both pass. rule(ray, total, ref, ref32, mask)."""
    for mask, bites in ((keep & (ref["n"] > 1), False), (good, True)):
        m = mask[..., None]
        rule(ray32 * m, (ray32 * m).sum((0, 1)), ref, ref32, mask)
        wrong = 1.01 * ray64 * m
        try:
            rule(wrong, wrong.sum((0, 1)), ref, ref32, mask)
            raised = False
        except AssertionError:
            raised = True
        assert raised == bites, "a 1 % error " + ("passes the conditioned rule" if bites else "fails the rule over all rays")


def d8_total_rule(total, want_ray, ref32_ray, mask, what=None):
    """The total against the float64 sum: 3x the float32 transliteration's own error in that sum + 1e-4 of the sum of magnitudes."""
    err32_total = np.abs((ref32_ray - want_ray)[mask].sum(0)).max()
    want = want_ray * mask[..., None]
    err = np.abs(total - want.reshape(-1, 3).sum(0)).max()
    assert err <= 3.0 * err32_total + 1e-4 * np.abs(want).sum(), (what, err, err32_total, np.abs(want).sum())


def d8_rule(ray, total, ref, ref32, mask, what=None):
    """D8's rule as test_march_bwd_cam_matches_the_f64_reference states it, for one view (or one band of rows):
    per ray err <= 3 err32 + 1e-4 scale; the total equals the rays' sum to 1e-5 of their magnitudes, and the float64 sum to
    3x the f32 transliteration's error in that sum + 1e-4 of the sum of magnitudes. -> (err / scale, err32 / scale)."""
    assert mask.sum() > 0.8 * (ref["n"] > 1).sum(), (what, mask.sum(), (ref["n"] > 1).sum())
    want = ref["dcam_ray"] * mask[..., None]
    scale = np.abs(want).max()
    err = np.abs(ray - want)[mask].max()
    err32 = np.abs(ref32["dcam_ray"] - ref["dcam_ray"])[mask].max()
    print("camgrad", what, "err/scale %.3g err32/scale %.3g rays %d" % (err / scale, err32 / scale, mask.sum()))
    assert np.isfinite(ray).all() and np.isfinite(total).all(), what
    assert (ray[~mask] == 0).all(), what
    assert err <= 3.0 * err32 + 1e-4 * scale, (what, err / scale, err32 / scale)
    assert np.abs(total - ray.sum((0, 1))).max() <= 1e-5 * np.abs(ray).sum(), what
    d8_total_rule(total, ref["dcam_ray"], ref32["dcam_ray"], mask, what)
    return err / scale, err32 / scale
