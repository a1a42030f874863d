// march_rgba_bundle.hip -- the differentiable march through a pre-classified RGBA volume over an arbitrary bundle of rays
// (DESIGN.md D21), gfx950. march_rgba.hip's three kernels with a ray as an input, as march_bundle.hip's are the 1-D TF march's:
// origins [N][3] and unit directions [N][3] in look_from's world coordinates, the ray buffers of bundle_setup_kernel
// (march_bundle.hip), gradients back to the four channels of the volume and to both ray arrays. The per-sample work is
// march_rgba.hip's, statement for statement, with the lane's own origin where those kernels read the view's camera: a bundle
// made of a pinhole camera's rays is that camera's image, bit for bit. There is no shading, so nothing here needs the double
// normals of march_bundle.hip's backwards: all arithmetic is float32.
//
// Shape: dr_bundle.h's -- one lane per ray over the linear ray index, the coherence of a bundle being the caller's ray order.
#include "dr_bundle.h"
#include "dr_camera.h"
#include "dr_rgba.h"

namespace dr {

template <typename VT>
struct RgbaBundleParams {
    VolView<VT> vol; int64_t sc;
    const float *origins, *dirs, *entry, *exit_; const int32_t *nsamp;
    int N, S; float inv_sr;
    float *out; int32_t *steps;
    const float *grad_out, *out_fwd;
    GradView dvol; int64_t dsc;
    // ray gradient
    const int32_t *fwd_steps;           // the forward's live samples per ray
    float t_near;
    uint32_t jitter_seed, ray_base;
    float *d_origins, *d_dirs;
};

// march_rgba_fwd_kernel in DR_MODE_DIFF
template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void march_rgba_bundle_fwd_kernel(RgbaBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    Ray<VT> ray;
    open_bundle_ray<false>(ray, p, P.vol, P.origins, P.entry, P.exit_, P.dirs, P.nsamp);
    const VolView<VT> &vol = ray.vol;
    const int m = rgba_samples(ray.rg.n, P.S, false);

    Composite c;
    int cnt = 0;
    for (int s = 0; s < m; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        Cell cell;
        tri_cell(vol, sm.px, sm.py, sm.pz, cell);
        const float4 v = tri_sample4<VT, VEC>(vol, P.sc, cell);
        ++cnt;
        sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w; sm.L = 1.0f;
        sm.op = opacity_of_alpha(sm.a, P.inv_sr);
        c.add(sm);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(false);
    if (P.steps) P.steps[p] = cnt;
}

// march_rgba_bwd_kernel: the tape-free adjoint, a cell's 32 sums sent when the ray leaves the cell (dr_rgba.h's VoxelRun)
template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void march_rgba_bundle_bwd_kernel(RgbaBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    const GradView dv = P.dvol;
    Ray<VT> ray;
    open_bundle_ray<true>(ray, p, P.vol, P.origins, P.entry, P.exit_, P.dirs, P.nsamp, P.grad_out, P.out_fwd);
    const VolView<VT> &vol = ray.vol;
    const int m = rgba_samples(ray.rg.n, P.S, false);

    Composite c;
    VoxelRun run;
    for (int s = 0; s < m; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        Cell cell;
        tri_cell(vol, sm.px, sm.py, sm.pz, cell);
        const float4 v = tri_sample4<VT, VEC>(vol, P.sc, cell);
        sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w;
        sm.L = sm.Lraw = 1.0f; sm.flat = true;   // no shading: sample_adjoint's normal path is off
        sm.op = opacity_of_alpha(sm.a, P.inv_sr);
        const float T = c.add(sm);
        const bool last = (s == m - 1) || !(c.A < 0.99f);
        SampleAdj ad;
        sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
        const float adj[4] = {ad.r_bar, ad.g_bar, ad.b_bar, ad.a_bar};
        if (!run.same(cell)) { run.flush(dv, P.dsc, vol.VX, vol.VY, vol.VZ); run.start(cell); }
        run.add(cell, adj);
    }
    run.flush(dv, P.dsc, vol.VX, vol.VY, vol.VZ);
}

// d origin and d direction of one ray: march_rgba_cam_kernel's walk, frozen branches and four sums (sP, sTP, s0, s1; no
// lighting, so D8's H_s = D_s = 0 and G_s = P_s), then bundle_ray_grad_kernel's once-per-ray tail (march_bundle.hip):
//   d origin = sP  + c_min e_min + c_max e_max,   d dir = sTP + c_min tmin e_min + c_max tmax e_max,
// c_min = -k_min / d_a, c_max = -k_max / d_b on the face axes a, b the forward picked, k_min = s0 A (0 where the t_near clamp
// was taken), k_max = s0 (1 - A) + s1, A = (1 - u/n)(1 - 0.5/n). d dir is the gradient w.r.t. the direction as a free 3-vector.
// No reduction, no atomic: each lane stores its six floats.
template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void rgba_bundle_ray_grad_kernel(RgbaBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    f3 d_o = make_f3(0.f, 0.f, 0.f), d_d = make_f3(0.f, 0.f, 0.f);
    // H6: a single-sample ray sits at 0/0 in the reference and contributes nothing
    if (P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_bundle_ray<false>(ray, p, P.vol, P.origins, P.entry, P.exit_, P.dirs, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = min(rgba_samples(rg.n, P.S, false), P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        f3 sP = make_f3(0.f, 0.f, 0.f), sTP = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f;
        Composite c;
        for (int s = 0; s < m; ++s) {
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            Cell cell;
            tri_cell(vol, sm.px, sm.py, sm.pz, cell);
            float4 gx, gy, gz;
            const float4 v = tri_sample4_grad<VT, VEC>(vol, P.sc, cell, sm.px, sm.py, sm.pz, gx, gy, gz);
            sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w;
            sm.L = sm.Lraw = 1.0f; sm.flat = true;   // no shading, as march_rgba_bundle_bwd_kernel
            sm.op = opacity_of_alpha(sm.a, P.inv_sr);
            const float T = c.add(sm);
            const bool last = s == m - 1;
            SampleAdj ad;
            sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
            const f3 Ps = make_f3(ad.r_bar * gx.x + ad.g_bar * gx.y + ad.b_bar * gx.z + ad.a_bar * gx.w,
                                  ad.r_bar * gy.x + ad.g_bar * gy.y + ad.b_bar * gy.z + ad.a_bar * gy.w,
                                  ad.r_bar * gz.x + ad.g_bar * gz.y + ad.b_bar * gz.z + ad.a_bar * gz.w);
            const float f = (float)s / (float)(rg.n - 1);
            const float t = mixf(rg.t0, rg.exit_, f);
            const float gv = dot3(Ps, vd);
            sP = f3_add(sP, Ps);
            sTP = f3_fma(t, Ps, sTP);
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }

        // once per ray: the faces the forward picked, the t_near clamp it took, the jitter draw behind A
        const float u = P.jitter_seed != 0u ? jitter_u(P.jitter_seed, P.ray_base, (uint32_t)p) : 0.0f;
        const SlabFaces sf = slab_faces(lf, vd);
        const bool clamped = P.t_near > -INFINITY && sf.tmin < P.t_near;
        const float nf = (float)rg.n;
        const float Acoef = (1.0f - u / nf) * (1.0f - 0.5f / nf);
        const float k_min = clamped ? 0.0f : s0 * Acoef, k_max = fmaf(s0, 1.0f - Acoef, s1);
        const f3 emin = make_f3(sf.amin == 0 ? 1.0f : 0.0f, sf.amin == 1 ? 1.0f : 0.0f, sf.amin == 2 ? 1.0f : 0.0f);
        const f3 emax = make_f3(sf.amax == 0 ? 1.0f : 0.0f, sf.amax == 1 ? 1.0f : 0.0f, sf.amax == 2 ? 1.0f : 0.0f);
        const float cmin = -k_min * sf.ivmin, cmax = -k_max * sf.ivmax;
        d_o = f3_fma(cmax, emax, f3_fma(cmin, emin, sP));
        d_d = f3_fma(cmax * sf.tmax, emax, f3_fma(cmin * sf.tmin, emin, sTP));
        // D5: a NaN ray (NaN upstream gradient) contributes nothing, infinities are clamped
        d_o = make_f3(finite_or_zero(d_o.x), finite_or_zero(d_o.y), finite_or_zero(d_o.z));
        d_d = make_f3(finite_or_zero(d_d.x), finite_or_zero(d_d.y), finite_or_zero(d_d.z));
    }
    const size_t q = 3 * (size_t)p;
    P.d_origins[q] = d_o.x; P.d_origins[q + 1] = d_o.y; P.d_origins[q + 2] = d_o.z;
    P.d_dirs[q] = d_d.x; P.d_dirs[q + 1] = d_d.y; P.d_dirs[q + 2] = d_d.z;
}

template <typename VT>
static RgbaBundleParams<VT> make_rgba_bundle_params(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b) {
    RgbaBundleParams<VT> P;
    P.vol = make_vol_view<VT>(a); P.sc = q.sc;
    P.origins = b.origins; P.dirs = a.rays; P.entry = a.entry; P.exit_ = a.exit_; P.nsamp = a.nsamp;
    P.N = b.N; P.S = a.S; P.inv_sr = 1.0f / a.sr;
    P.out = a.out; P.steps = a.steps;
    P.grad_out = a.grad_out; P.out_fwd = a.out_fwd;
    P.dvol.p = a.d_vol; P.dvol.sx = a.dsx; P.dvol.sy = a.dsy; P.dvol.sz = a.dsz; P.dsc = q.dsc;
    P.fwd_steps = b.steps; P.t_near = b.t_near; P.jitter_seed = b.jitter_seed; P.ray_base = b.ray_base;
    P.d_origins = b.d_origins; P.d_dirs = b.d_dirs;
    return P;
}

// f32 or f16, VEC decided once per launch (rgba_vec_ok), as march_rgba.hip
template <typename VT>
static int rgba_bundle_fwd_dispatch(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    const RgbaBundleParams<VT> P = make_rgba_bundle_params<VT>(a, q, b);
    return launch_bundle(rgba_vec_ok(a, q) ? march_rgba_bundle_fwd_kernel<VT, true> : march_rgba_bundle_fwd_kernel<VT, false>, b.N, 0,
                         stream, P);
}

template <typename VT>
static int rgba_bundle_bwd_dispatch(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    const RgbaBundleParams<VT> P = make_rgba_bundle_params<VT>(a, q, b);
    return launch_bundle(rgba_vec_ok(a, q) ? march_rgba_bundle_bwd_kernel<VT, true> : march_rgba_bundle_bwd_kernel<VT, false>, b.N, 0,
                         stream, P);
}

template <typename VT>
static int rgba_bundle_ray_grad_dispatch(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    const RgbaBundleParams<VT> P = make_rgba_bundle_params<VT>(a, q, b);
    return launch_bundle(rgba_vec_ok(a, q) ? rgba_bundle_ray_grad_kernel<VT, true> : rgba_bundle_ray_grad_kernel<VT, false>, b.N, 0,
                         stream, P);
}

int launch_march_rgba_bundle_fwd(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? rgba_bundle_fwd_dispatch<__half>(a, q, b, stream) : rgba_bundle_fwd_dispatch<float>(a, q, b, stream);
}

int launch_march_rgba_bundle_bwd(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? rgba_bundle_bwd_dispatch<__half>(a, q, b, stream) : rgba_bundle_bwd_dispatch<float>(a, q, b, stream);
}

int launch_rgba_bundle_ray_grad(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? rgba_bundle_ray_grad_dispatch<__half>(a, q, b, stream)
                                 : rgba_bundle_ray_grad_dispatch<float>(a, q, b, stream);
}

}  // namespace dr
