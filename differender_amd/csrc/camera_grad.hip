// camera_grad.hip -- gradient of the differentiable march w.r.t. the camera position look_from, gfx950.
// The reference defines no such gradient (RaycastFunction.backward returns None, VR.py:465,473-476); this is the reverse-mode
// derivative of its forward program with the usual frozen branches: the sample count n, the live-sample count (the forward's
// `steps`), the jitter draw u, the slab faces fmaxf/fminf picked for tmin and tmax (VR.py:44-45), every tap's trilinear cell
// and every max/min/clamp predicate (Taichi's rules, as in tests/golden/make_autograd_golden.py).
//
// The camera enters in four places: the ray direction (VR.py:127-151), the slab entry/exit (VR.py:28-53) and the jitter offset
// built from them (VR.py:245-256), every sample position pos_s = look_from + t_s vd with t_s = mix(t0, tmax, s/(n-1))
// (VR.py:273-280), and the Phong terms light_pos = look_from + e_y and r.(-vd) (VR.py:281-297). With, per sample,
//   P_s = dL/dpos_s through the 7 taps, H_s = dL/d(pos_s - light_pos), D_s = dL/dvd through r.(-vd), G_s = P_s + H_s,
// the chain collapses (the H_s of pos_s and of light_pos cancel in the direct term) to
//   d look_from = sum P_s + J_vd^T (sum t_s G_s + sum D_s) + sum (1-f_s)(G_s.vd) grad t0 + sum f_s (G_s.vd) grad tmax,
//   grad t0 = A grad tmin + (1-A) grad tmax,  A = (1 - u/n)(1 - 0.5/n),  f_s = s/(n-1),
// so a ray keeps four running sums over its samples and evaluates the 3x3 Jacobian J_vd = d vd / d look_from and the slab rows
// grad tmin, grad tmax once.
//
// Shape: one lane per ray, a wave per 8x8 pixel tile, a sequential march -- march_bwd_baseline_kernel's walk. The per-sample
// adjoint needs the composite in front of the sample, which the sequential walk has for free; the wave-per-ray alternative
// (DPP scans over 64 samples) would be faster on long rays but needs its own tap/adjoint pipeline. Sums: f32 per ray, f64 per
// workgroup (LDS), then ONE f64 atomic per component per workgroup into d_cam[view][3] (no per-sample or per-ray atomics).
#include "dr_camera.h"
#include "dr_tile.h"

namespace dr {

template <typename VT>
struct CamParams : RayParams<VT> {
    const int32_t *fwd_steps;   // the forward's live samples per ray
    int img_W, row0;
    CamFields cf;               // (aspect: img_W / H)
};

// POSE: the gradient w.r.t. the free camera's ten parameters (look_from, look_at, up, fov) from the same four sums -- only the
// once-per-ray tail and the reduction differ (dr_camera.h: pose_ray_grad, pose_reduce); d_cam is [views][10], d_cam_ray [..][10].
template <typename VT, bool TF_LDS, bool POSE = false>
__global__ __launch_bounds__(256) void camera_grad_kernel(CamParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    __shared__ double red[3][256];
    const int view = blockIdx.y;
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, P.R);

    f3 dcam = make_f3(0.f, 0.f, 0.f);
    PoseGrad dpose = pose_zero();
    int i, j;
    const bool in_img = tile_pixel(P.W, P.H, i, j);
    const size_t p = ray_index(P.W, P.H, view, i, j);
    // H6: a single-sample ray sits at 0/0 in the reference and contributes nothing
    if (in_img && P.nsamp[p] > 1) {
        Ray<VT> ray;   // (open_ray's parts: the loads keep the order they had, which the generated code follows)
        open_view(ray, view, P.vol, P.vol_vs, P.cam);
        const VolView<VT> &vol = ray.vol;
        const f3 lf = ray.cam;
        const f3 light = make_f3(lf.x + 0.0f, lf.y + 1.0f, lf.z + 0.0f);
        open_geom<false>(ray, p, P.entry, P.exit_, P.rays, P.nsamp);
        const RayGeom &rg = ray.rg;
        const f3 vd = ray.vd;
        int nmarch = rg.n > P.S ? P.S : rg.n;
        nmarch = min(nmarch, P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        const float4 go = ray.go, of = ray.of;
        const float delta = 1e-3f;
        f3 sP = make_f3(0.f, 0.f, 0.f), sTG = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f;
        Composite c;
        for (int s = 0; s < nmarch; ++s) {
            Sample sm;
            sample_pos(rg, lf.x, lf.y, lf.z, s, sm.px, sm.py, sm.pz);
            f3 gI, gp, gm, ddx, ddy, ddz;   // slopes of the intensity tap and of the three central differences
            sm.I = tri_sample_grad(vol, sm.px, sm.py, sm.pz, gI);
            classify_from_I(tf, P.R, P.tf_len, P.inv_sr, sm);
            float vp = tri_sample_grad(vol, sm.px + delta, sm.py, sm.pz, gp), vm = tri_sample_grad(vol, sm.px - delta, sm.py, sm.pz, gm);
            const float dx = vp - vm;
            ddx = make_f3(gp.x - gm.x, gp.y - gm.y, gp.z - gm.z);
            vp = tri_sample_grad(vol, sm.px, sm.py + delta, sm.pz, gp); vm = tri_sample_grad(vol, sm.px, sm.py - delta, sm.pz, gm);
            const float dy = vp - vm;
            ddy = make_f3(gp.x - gm.x, gp.y - gm.y, gp.z - gm.z);
            vp = tri_sample_grad(vol, sm.px, sm.py, sm.pz + delta, gp); vm = tri_sample_grad(vol, sm.px, sm.py, sm.pz - delta, gm);
            const float dz = vp - vm;
            ddz = make_f3(gp.x - gm.x, gp.y - gm.y, gp.z - gm.z);
            shade_from_grad<false>(dx, dy, dz, light, vd, true, sm);
            const float T = c.add(sm);
            const bool last = s == nmarch - 1;
            SampleAdj ad;
            sample_adjoint(sm, vd, T, c.suffix(go, of), last, go, P.inv_sr, ad);
            const float I_bar = intensity_adjoint(sm, tf[sm.lo], tf[sm.hi], ad, P.tf_len);
            // dL/dpos through the taps: the intensity tap and the central differences of the normal (0 when flat, D1)
            f3 Ps = f3_scale(I_bar, gI);
            Ps = f3_fma(ad.gx, ddx, Ps);
            Ps = f3_fma(ad.gy, ddy, Ps);
            Ps = f3_fma(ad.gz, ddz, Ps);
            // dL/d(pos - light_pos) through light_dir, dL/dvd through r.(-vd): the tail of sample_adjoint's lighting chain
            f3 Hs = make_f3(0.f, 0.f, 0.f), Ds = make_f3(0.f, 0.f, 0.f);
            if (!sm.flat) {
                const float rgbdot = go.x * sm.r + go.y * sm.g + go.z * sm.b;
                const float L_bar = sm.op * T * rgbdot;
                const float Lraw_bar = (1.0f < sm.Lraw) ? 0.0f : L_bar;
                const float rdv_bar = 0.3f * 32.0f * pow31(sm.rdv) * Lraw_bar;
                const float q_bar = (0.0f < sm.q) ? rdv_bar : 0.0f;
                const f3 rf_bar = make_f3(-vd.x * q_bar, -vd.y * q_bar, -vd.z * q_bar);
                const float m_bar = ((0.0f < sm.m) ? 0.8f * Lraw_bar : 0.0f) - 2.0f * dot3(sm.nrm, rf_bar);
                const f3 ld_bar = f3_fma(m_bar, sm.nrm, rf_bar);
                const f3 lv = make_f3(sm.px - light.x, sm.py - light.y, sm.pz - light.z);
                const float il = inv_norm3(lv);
                Hs = f3_scale(il, f3_fma(-dot3(sm.ld, ld_bar), sm.ld, ld_bar));
                Ds = f3_scale(-q_bar, sm.rf);
            }
            const float f = (float)s / (float)(rg.n - 1);
            const float t = mixf(rg.t0, rg.exit_, f);
            const f3 Gs = f3_add(Ps, Hs);
            const float gv = dot3(Gs, vd);
            sP = f3_add(sP, Ps);
            sTG = f3_add(sTG, f3_fma(t, Gs, Ds));
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }

        if (POSE) {
            // once per ray: the ten pose gradients from the four sums (dr_camera.h), then D5
            const PoseRay q = pose_ray(P.cf.pose, P.cf.fov_v, view, P.cf.near_d, P.cf.aspect, P.cf.near_w, P.cf.near_h, i + P.row0,
                                       P.img_W, j, P.H, rg.n, P.cf.jitter_seed, P.cf.view_base + (uint32_t)view);
            dpose = pose_finite(pose_ray_grad(lf, q, vd, P.cf.near_, sP, sTG, s0 * q.A, fmaf(s0, 1.0f - q.A, s1)));
        } else {
            // once per ray: J_vd, the rows of the slab faces the forward picked and the jitter draw behind grad t0
            M3 J;
            f3 g_tmin, g_tmax, g_t0;
            float u;
            camera_ray_tail(lf, vd, i + P.row0, P.img_W, j, P.H, P.cf.near_, P.cf.near_w, P.cf.near_h, rg.n, P.cf.jitter_seed,
                            P.cf.view_base + (uint32_t)view, J, g_tmin, g_tmax, g_t0, u);
            dcam = f3_add(sP, mul_t(J, sTG));
            dcam = f3_fma(s0, g_t0, dcam);
            dcam = f3_fma(s1, g_tmax, dcam);
            // D5: a NaN ray (NaN upstream gradient) contributes nothing, infinities are clamped
            dcam = make_f3(finite_or_zero(dcam.x), finite_or_zero(dcam.y), finite_or_zero(dcam.z));
        }
    }
    if (POSE) pose_reduce(dpose, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
    else camera_reduce(dcam, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
}

template <typename VT>
static int cam_dispatch(const MarchArgs &a, const CamArgs &c, hipStream_t stream) {
    CamParams<VT> P{make_ray_params<VT>(a)};
    P.fwd_steps = c.steps; P.img_W = a.img_W; P.row0 = a.row0;
    P.cf = fill_cam_fields(a, c.jitter_seed, c.view_base, c.d_cam, c.d_cam_ray);
    // (not dr_tile.h's table_tier: tests/test_gpu_camera_grad_edges.py reads the limit from the statement below)
    if (a.pose) {   // (the table tiers of the fixed camera, below)
        const size_t lds_p = (size_t)a.R * sizeof(float4);
        if (lds_p <= 48 * 1024) return launch_tiles(camera_grad_kernel<VT, true, true>, a, lds_p, stream, P);
        return launch_tiles(camera_grad_kernel<VT, false, true>, a, 0, stream, P);
    }
    const size_t lds = (size_t)a.R * sizeof(float4);
    if (lds <= 48 * 1024) return launch_tiles(camera_grad_kernel<VT, true>, a, lds, stream, P);
    return launch_tiles(camera_grad_kernel<VT, false>, a, 0, stream, P);   // a large TF is read where it lies
}

int launch_camera_grad(const MarchArgs &a, const CamArgs &c, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? cam_dispatch<__half>(a, c, stream) : cam_dispatch<float>(a, c, stream);
}

}  // namespace dr
