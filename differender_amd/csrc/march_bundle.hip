// march_bundle.hip -- the differentiable 1-D TF march over an arbitrary bundle of rays, gfx950.
// Every other renderer draws its rays from one pinhole camera per view (ray_setup.hip); here a ray is an input: origins [N][3]
// and unit directions [N][3] in look_from's world coordinates, with gradients back to both. The per-sample work is the plain
// kernels' (march_baseline.hip, camera_grad.hip), statement for statement, with the ray's origin where they read the view's
// camera and the light at origin + e_y per ray: a bundle made of a pinhole camera's rays is that camera's image, bit for bit.
// One departure: the backwards project a sample's adjoint with a normal from double taps (shade_for_adjoint; the ray gradient
// around the sample's position in double as well, shade_for_ray_adjoint).
//
// Shape: dr_bundle.h's -- one lane per ray over the linear ray index, the coherence of a bundle being the caller's ray order.
//
// Like ray_setup.hip this translation unit is built with -ffp-contract=off: bundle_setup_kernel's sample count
// n = floor(sr * len * diag) + 1 is then ray_setup_kernel's for the same origin and direction.
#include "dr_bundle.h"
#include "dr_camera.h"

namespace dr {

template <typename VT>
struct BundleParams : RayParams<VT> {   // (cam: the origins [N][3]; rays: the directions [N][3]; W = N, H = 1)
    int N;
    const int32_t *fwd_steps;           // ray gradient: the forward's live samples per ray
    float t_near;
    uint32_t jitter_seed, ray_base;
    float *d_origins, *d_dirs;
};

struct BundleSetupParams {
    const float *origins, *dirs;
    int N;
    float vol_diag, sr, t_near;
    uint32_t jitter_seed, ray_base;
    float *entry, *exit_;
    int32_t *nsamp;
};

// ray_setup_kernel's statements from the slab test on, in its order, for the ray (o, vd) as given. t_near (-INFINITY: off)
// clamps the entry distance before the hit test and the sample count: 0 makes a ray a ray, where the reference marches the
// whole line through a camera inside the box.
__global__ __launch_bounds__(256) void bundle_setup_kernel(BundleSetupParams P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    const f3 lf = load_f3(P.origins, p), vd = load_f3(P.dirs, p);

    // slab test against [-1,1]^3
    const float fx = 1.0f / vd.x, fy = 1.0f / vd.y, fz = 1.0f / vd.z;
    const float t1 = (-1.0f - lf.x) * fx, t2 = (1.0f - lf.x) * fx;
    const float t3 = (-1.0f - lf.y) * fy, t4 = (1.0f - lf.y) * fy;
    const float t5 = (-1.0f - lf.z) * fz, t6 = (1.0f - lf.z) * fz;
    float tmin = fmaxf(fmaxf(fminf(t1, t2), fminf(t3, t4)), fminf(t5, t6));
    const float tmax = fminf(fminf(fmaxf(t1, t2), fmaxf(t3, t4)), fmaxf(t5, t6));
    if (P.t_near > -INFINITY) tmin = fmaxf(tmin, P.t_near);
    const bool hit = !(tmax < 0.0f || tmin > tmax);

    const float ray_len = tmax - tmin;
    const float n_samples = (hit ? 1.0f : 0.0f) * (floorf(P.sr * ray_len * P.vol_diag) + 1.0f);
    if (P.jitter_seed != 0u) {
        const float uu = jitter_u(P.jitter_seed, P.ray_base, (uint32_t)p);
        tmin += uu * ray_len / n_samples;
    }
    P.entry[p] = tmin;
    P.exit_[p] = tmax;
    P.nsamp[p] = (int32_t)n_samples;
}

// march_fwd_baseline_kernel in DR_MODE_DIFF
template <typename VT, bool TF_LDS>
__global__ __launch_bounds__(256) void march_bundle_fwd_kernel(BundleParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const float4 *lds_tf = stage_table<TF_LDS>(lds_tf_, P.tf, P.R);

    const int p = bundle_ray();
    if (p >= P.N) return;
    Ray<VT> ray;
    open_bundle_ray<false>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const f3 light = make_f3(ray.cam.x + 0.0f, ray.cam.y + 1.0f, ray.cam.z + 0.0f);
    const int nmarch = ray.rg.n > P.S ? P.S : ray.rg.n;

    Composite c;
    int cnt = 0;
    for (int s = 0; s < nmarch; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        classify(ray.vol, lds_tf, P.R, P.tf_len, P.inv_sr, sm);
        ++cnt;
        shade(ray.vol, light, ray.vd, true, sm);
        c.add(sm);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(false);
    if (P.steps) P.steps[p] = cnt;
}

// tri_sample in double: the clamp, the scale shape - 1 - 1e-4 (VR.py:165, not rounded to float first), the split and the
// lerps (x -> y -> z) of dr_device.h's tri_cell / tri_sample on the same voxels, every operation in double
template <typename VT>
__device__ __forceinline__ double tri_sample_f64(const VolView<VT> &v, double px, double py, double pz) {
    const double qx = fmin(1.0, fmax(0.0, 0.5 * px + 0.5)) * ((double)v.VX - 1.0 - 1e-4);
    const double qy = fmin(1.0, fmax(0.0, 0.5 * py + 0.5)) * ((double)v.VY - 1.0 - 1e-4);
    const double qz = fmin(1.0, fmax(0.0, 0.5 * pz + 0.5)) * ((double)v.VZ - 1.0 - 1e-4);
    const double lx = floor(qx), ly = floor(qy), lz = floor(qz);
    const double fx = qx - lx, fy = qy - ly, fz = qz - lz;
    const int x0 = min((int)lx, v.VX - 1), y0 = min((int)ly, v.VY - 1), z0 = min((int)lz, v.VZ - 1);
    const int x1 = min(x0 + 1, v.VX - 1), y1 = min(y0 + 1, v.VY - 1), z1 = min(z0 + 1, v.VZ - 1);
    const VT *b00 = v.p + x0 * v.sx + y0 * v.sy, *b10 = v.p + x1 * v.sx + y0 * v.sy;
    const VT *b01 = v.p + x0 * v.sx + y1 * v.sy, *b11 = v.p + x1 * v.sx + y1 * v.sy;
    const int64_t o0 = z0 * v.sz, o1 = z1 * v.sz;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double zl = ((double)ld_voxel(b00 + o0) * gx + (double)ld_voxel(b10 + o0) * fx) * gy +
                      ((double)ld_voxel(b01 + o0) * gx + (double)ld_voxel(b11 + o0) * fx) * fy;
    const double zh = ((double)ld_voxel(b00 + o1) * gx + (double)ld_voxel(b10 + o1) * fx) * gy +
                      ((double)ld_voxel(b01 + o1) * gx + (double)ld_voxel(b11 + o1) * fx) * fy;
    return zl * (1.0 - fz) + zh * fz;
}

// The sample `sm` shaded again for the adjoint, its three central differences taken from taps in double and rounded once. A
// tap is a number near the voxel values, good to half an ulp of THAT in float32 (3e-8 for values near 0.5), and the central
// difference of two taps 2e-3 apart is 1e-3 .. 1e-4 of it: where the volume is nearly flat the float32 difference, and with
// it the unit normal and everything its adjoint is projected with (which scales with 1 / |g|), carries 1e-3 of rounding noise
// -- measured on a ray of tests/test_gpu_bundle.py: 7.6e-4 of the scale of d_vol from one sample, five times what the float32
// transliteration happened to draw. The differences of double taps are good to 1e-9 of the taps, and their rounding to float is
// relative. The composite stays the forward's (float32 shading, the forward's bits): only the adjoint is projected with the
// better normal.
template <typename VT>
__device__ __forceinline__ Sample shade_for_adjoint(const VolView<VT> &v, f3 light, f3 vd, const Sample &sm) {
    const double px = (double)sm.px, py = (double)sm.py, pz = (double)sm.pz, delta = 1e-3;
    const float dx = (float)(tri_sample_f64(v, px + delta, py, pz) - tri_sample_f64(v, px - delta, py, pz));
    const float dy = (float)(tri_sample_f64(v, px, py + delta, pz) - tri_sample_f64(v, px, py - delta, pz));
    const float dz = (float)(tri_sample_f64(v, px, py, pz + delta) - tri_sample_f64(v, px, py, pz - delta));
    Sample sa = sm;
    shade_from_grad<false>(dx, dy, dz, light, vd, true, sa);
    return sa;
}

// A ray's sample distances in double, from the origin and direction the kernels read: bundle_setup_kernel's slab test, t_near
// clamp and jitter offset and load_ray's t0, every operation in double (n is the forward's). For the ray gradient's normal.
struct GeomF64 { double t0, exit_; };
__device__ __forceinline__ GeomF64 bundle_geom_f64(f3 lf, f3 vd, int n, float t_near, float u) {
    const double fx = 1.0 / (double)vd.x, fy = 1.0 / (double)vd.y, fz = 1.0 / (double)vd.z;
    const double t1 = (-1.0 - (double)lf.x) * fx, t2 = (1.0 - (double)lf.x) * fx;
    const double t3 = (-1.0 - (double)lf.y) * fy, t4 = (1.0 - (double)lf.y) * fy;
    const double t5 = (-1.0 - (double)lf.z) * fz, t6 = (1.0 - (double)lf.z) * fz;
    double tmin = fmax(fmax(fmin(t1, t2), fmin(t3, t4)), fmin(t5, t6));
    const double tmax = fmin(fmin(fmax(t1, t2), fmax(t3, t4)), fmax(t5, t6));
    if (t_near > -INFINITY) tmin = fmax(tmin, (double)t_near);
    const double entry = tmin + (double)u * (tmax - tmin) / (double)n;
    GeomF64 g;
    g.t0 = entry + 0.5 * (tmax - entry) / (double)n;
    g.exit_ = tmax;
    return g;
}

// The sample `sm` of a ray gradient shaded again for the adjoint: shade_for_adjoint's double taps, taken around sample s's
// position in double (GeomF64) rather than around the float32 position. A sample whose normal taps straddle a cell boundary
// where |grad| is 1e-4 can carry a ray's whole d_origin and d_dir (the slope's jump across the boundary over |grad|), and its
// normal then moves by 5e-4 with the 1e-7 of a float32 position as it does with the 6e-8 of two float32 taps (measured:
// tests/test_gpu_bundle_edges.py, the f16 volume's ray 1 and c_clip x ortho's ray 33).
template <typename VT>
__device__ __forceinline__ Sample shade_for_ray_adjoint(const VolView<VT> &v, f3 lf, f3 light, f3 vd, const GeomF64 &gd, int n,
                                                        int s, const Sample &sm) {
    const double f = (double)s / (double)(n - 1), t = gd.t0 * (1.0 - f) + gd.exit_ * f, delta = 1e-3;
    const double px = (double)lf.x + t * (double)vd.x, py = (double)lf.y + t * (double)vd.y, pz = (double)lf.z + t * (double)vd.z;
    const float dx = (float)(tri_sample_f64(v, px + delta, py, pz) - tri_sample_f64(v, px - delta, py, pz));
    const float dy = (float)(tri_sample_f64(v, px, py + delta, pz) - tri_sample_f64(v, px, py - delta, pz));
    const float dz = (float)(tri_sample_f64(v, px, py, pz + delta) - tri_sample_f64(v, px, py, pz - delta));
    Sample sa = sm;
    shade_from_grad<false>(dx, dy, dz, light, vd, true, sa);
    return sa;
}

// march_bwd_baseline_kernel without the RayFilter machinery, the adjoint projected with shade_for_adjoint's normal; TABLES: its
// three tiers (dr_tile.h's table_tier)
template <typename VT, int TABLES>
__global__ __launch_bounds__(256) void march_bundle_bwd_kernel(BundleParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    double *lds_dtf = reinterpret_cast<double *>(lds_tf_ + P.R);
    const float4 *lds_tf = stage_table<TABLES >= 1>(lds_tf_, P.tf, P.R, lds_dtf, TABLES == 2 ? 4 * P.R : 0);
    float *dtf_g = P.d_tf;

    const int p = bundle_ray();
    if (p < P.N) {
        const GradView dv = P.dvol;
        const bool want_vol = dv.p != nullptr;
        const bool want_tf = P.d_tf != nullptr;
        Ray<VT> ray;
        open_bundle_ray<true>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd);
        const f3 light = make_f3(ray.cam.x + 0.0f, ray.cam.y + 1.0f, ray.cam.z + 0.0f);
        const int nmarch = ray.rg.n > P.S ? P.S : ray.rg.n;

        Composite c;
        for (int s = 0; s < nmarch; ++s) {
            if (!(c.A < 0.99f)) break;
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            classify(ray.vol, lds_tf, P.R, P.tf_len, P.inv_sr, sm);
            shade(ray.vol, light, ray.vd, true, sm);
            const float T = c.add(sm);
            const bool last = (s == nmarch - 1) || !(c.A < 0.99f);
            const Sample sa = shade_for_adjoint(ray.vol, light, ray.vd, sm);
            SampleAdj ad;
            sample_adjoint(sa, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
            const float I_bar = want_vol ? intensity_adjoint(sa, lds_tf[sa.lo], lds_tf[sa.hi], ad, P.tf_len) : 0.0f;
            if (want_tf && TABLES < 2) dtf_add(dtf_g, sa, ad, false);
            else if (want_tf) dtf_add(lds_dtf, sa, ad);
            if (want_vol) scatter_taps(ray.vol, dv, sa, I_bar, ad.gx, ad.gy, ad.gz);
        }
    }
    if (P.d_tf && TABLES == 2) {
        __syncthreads();
        for (int k = threadIdx.x; k < 4 * P.R; k += 256) {
            const float v = (float)lds_dtf[k];
            if (v == 0.0f) continue;
            unsafeAtomicAdd(dtf_g + k, v);
        }
    }
}

// d origin and d direction of one ray: camera_grad_kernel's walk and its four sums (sP, sTG, s0, s1; the same frozen branches),
// then the bundle's own once-per-ray tail. With tmin = (f_a - o_a) / d_a on the face axis a the forward picked, tmax likewise on
// b, t0 = A tmin + (1 - A) tmax and A = (1 - u/n)(1 - 0.5/n) (D8):
//   d origin = sP  + k_min grad_o tmin + k_max grad_o tmax,   grad_o tmin = -e_a / d_a,
//   d dir    = sTG + k_min grad_d tmin + k_max grad_d tmax,   grad_d tmin = -(tmin / d_a) e_a,
// k_min = s0 A, k_max = s0 (1 - A) + s1; where the t_near clamp was taken tmin is a constant and its rows are 0. d dir is the
// gradient w.r.t. the direction as a free 3-vector: the caller normalises in torch, and autograd carries it through. No
// reduction, no atomic: each lane stores its six floats.
template <typename VT, bool TF_LDS>
__global__ __launch_bounds__(256) void bundle_ray_grad_kernel(BundleParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf, P.R);

    const int p = bundle_ray();
    if (p >= P.N) return;
    f3 d_o = make_f3(0.f, 0.f, 0.f), d_d = make_f3(0.f, 0.f, 0.f);
    // H6: a single-sample ray sits at 0/0 in the reference and contributes nothing
    if (P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_bundle_ray<false>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const f3 lf = ray.cam;
        const f3 light = make_f3(lf.x + 0.0f, lf.y + 1.0f, lf.z + 0.0f);
        const RayGeom &rg = ray.rg;
        const f3 vd = ray.vd;
        int nmarch = rg.n > P.S ? P.S : rg.n;
        nmarch = min(nmarch, P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        const float4 go = ray.go, of = ray.of;
        const float delta = 1e-3f;
        const float u = P.jitter_seed != 0u ? jitter_u(P.jitter_seed, P.ray_base, (uint32_t)p) : 0.0f;
        const GeomF64 gd = bundle_geom_f64(lf, vd, rg.n, P.t_near, u);
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
            const float T = c.add(sm);   // (the forward's composite, its bits)
            const bool last = s == nmarch - 1;
            sm = shade_for_ray_adjoint(vol, lf, light, vd, gd, rg.n, s, sm);   // from here on: the adjoint's normal
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

        // once per ray: the faces the forward picked, the t_near clamp it took, the jitter draw behind A
        const SlabFaces sf = slab_faces(lf, vd);
        const bool clamped = P.t_near > -INFINITY && sf.tmin < P.t_near;
        const float nf = (float)rg.n;
        const float Acoef = (1.0f - u / nf) * (1.0f - 0.5f / nf);
        const float k_min = clamped ? 0.0f : s0 * Acoef, k_max = fmaf(s0, 1.0f - Acoef, s1);
        const f3 emin = make_f3(sf.amin == 0 ? 1.0f : 0.0f, sf.amin == 1 ? 1.0f : 0.0f, sf.amin == 2 ? 1.0f : 0.0f);
        const f3 emax = make_f3(sf.amax == 0 ? 1.0f : 0.0f, sf.amax == 1 ? 1.0f : 0.0f, sf.amax == 2 ? 1.0f : 0.0f);
        const float cmin = -k_min * sf.ivmin, cmax = -k_max * sf.ivmax;
        d_o = f3_fma(cmax, emax, f3_fma(cmin, emin, sP));
        d_d = f3_fma(cmax * sf.tmax, emax, f3_fma(cmin * sf.tmin, emin, sTG));
        // D5: a NaN ray (NaN upstream gradient) contributes nothing, infinities are clamped
        d_o = make_f3(finite_or_zero(d_o.x), finite_or_zero(d_o.y), finite_or_zero(d_o.z));
        d_d = make_f3(finite_or_zero(d_d.x), finite_or_zero(d_d.y), finite_or_zero(d_d.z));
    }
    const size_t q = 3 * (size_t)p;
    P.d_origins[q] = d_o.x; P.d_origins[q + 1] = d_o.y; P.d_origins[q + 2] = d_o.z;
    P.d_dirs[q] = d_d.x; P.d_dirs[q + 1] = d_d.y; P.d_dirs[q + 2] = d_d.z;
}

template <typename VT>
static BundleParams<VT> make_bundle_params(const MarchArgs &a, const BundleArgs &b) {
    BundleParams<VT> P{make_ray_params<VT>(a)};
    P.cam = b.origins;
    P.N = b.N; P.fwd_steps = b.steps; P.t_near = b.t_near; P.jitter_seed = b.jitter_seed; P.ray_base = b.ray_base;
    P.d_origins = b.d_origins; P.d_dirs = b.d_dirs;
    return P;
}

int launch_bundle_setup(const BundleArgs &b, const float *dirs, int VX, int VY, int VZ, float sr, float *entry, float *exit_,
                        int32_t *nsamp, hipStream_t stream) {
    BundleSetupParams P;
    P.origins = b.origins; P.dirs = dirs; P.N = b.N;
    P.vol_diag = (float)sqrt((double)(VX - 1) * (VX - 1) + (double)(VY - 1) * (VY - 1) + (double)(VZ - 1) * (VZ - 1));
    P.sr = sr; P.t_near = b.t_near; P.jitter_seed = b.jitter_seed; P.ray_base = b.ray_base;
    P.entry = entry; P.exit_ = exit_; P.nsamp = nsamp;
    hipLaunchKernelGGL(bundle_setup_kernel, bundle_grid(b.N), dim3(256), 0, stream, P);
    return (int)hipGetLastError();
}

template <typename VT>
static int bundle_fwd_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);
    const BundleParams<VT> P = make_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 1 ? march_bundle_fwd_kernel<VT, true> : march_bundle_fwd_kernel<VT, false>, b.N, t.lds, stream, P);
}

int launch_march_bundle_fwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? bundle_fwd_dispatch<__half>(a, b, stream) : bundle_fwd_dispatch<float>(a, b, stream);
}

template <typename VT>
static int bundle_bwd_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, true);
    const BundleParams<VT> P = make_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 2 ? march_bundle_bwd_kernel<VT, 2> : (t.tables == 1 ? march_bundle_bwd_kernel<VT, 1> : march_bundle_bwd_kernel<VT, 0>),
                         b.N, t.lds, stream, P);
}

int launch_march_bundle_bwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? bundle_bwd_dispatch<__half>(a, b, stream) : bundle_bwd_dispatch<float>(a, b, stream);
}

template <typename VT>
static int bundle_ray_grad_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);
    const BundleParams<VT> P = make_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 1 ? bundle_ray_grad_kernel<VT, true> : bundle_ray_grad_kernel<VT, false>, b.N, t.lds, stream, P);
}

int launch_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? bundle_ray_grad_dispatch<__half>(a, b, stream) : bundle_ray_grad_dispatch<float>(a, b, stream);
}

}  // namespace dr
