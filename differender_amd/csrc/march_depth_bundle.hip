// march_depth_bundle.hip -- ray-depth moments of the differentiable march over an arbitrary bundle of rays,
// gfx950. march_depth.hip's three kernels with a ray as an input, as march_bundle.hip's are the 1-D TF march's: origins [N][3]
// and unit directions [N][3] in look_from's world coordinates, the ray buffers of bundle_setup_kernel (march_bundle.hip),
// gradients back to the volume, to the table's alpha column and to both ray arrays. The per-sample work is march_depth.hip's
// (dr_depth.h), statement for statement, with the lane's own origin where those kernels read the view's camera: a bundle made
// of a pinhole camera's rays gives that camera's moments, bit for bit, and channel 3 and `steps` are march_bundle_fwd_kernel's.
// t_s is the march's own parameter mix(t0, exit, s/(n-1)): the distance from the ray's origin along its unit direction. There
// is no shading, so nothing here needs the double normals of march_bundle.hip's backwards: all arithmetic is float32.
//
// Shape: dr_bundle.h's -- one lane per ray over the linear ray index, the coherence of a bundle being the caller's ray order.
#include "dr_bundle.h"
#include "dr_depth.h"

namespace dr {

template <typename VT>
struct DepthBundleParams : RayParams<VT> {   // (cam: the origins [N][3]; rays: the directions [N][3]; W = N, H = 1)
    int N;
    const int32_t *fwd_steps;                // ray gradient: the forward's live samples per ray
    float t_near;
    uint32_t jitter_seed, ray_base;
    float *d_origins, *d_dirs;
};

// march_depth_fwd_kernel
template <typename VT, bool TF_LDS>
__global__ __launch_bounds__(256) void march_depth_bundle_fwd_kernel(DepthBundleParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf, P.R);

    const int p = bundle_ray();
    if (p >= P.N) return;
    Ray<VT> ray;
    open_bundle_ray<false>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const int m = depth_samples(ray.rg.n, P.S);

    CompositeDepth c;
    int cnt = 0;
    for (int s = 0; s < m; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        classify(ray.vol, tf, P.R, P.tf_len, P.inv_sr, sm);
        ++cnt;
        float f;
        c.add(sample_t(ray.rg, s, f), sm.op);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel();
    if (P.steps) P.steps[p] = cnt;
}

// march_depth_bwd_kernel: the tape-free adjoint and its three table tiers (tier 2 keeps [R] doubles for the alpha column; the
// colour columns of the caller's d_tf are never written). d_vol goes through a per-cell run (dr_depth.h's VoxelRun1): the eight
// corner sums of the samples a ray spends in one cell are sent when the ray leaves the cell and after its last sample.
template <typename VT, int TABLES>
__global__ __launch_bounds__(256) void march_depth_bundle_bwd_kernel(DepthBundleParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    double *lds_dalpha = reinterpret_cast<double *>(lds_tf_ + P.R);
    const float4 *tf = stage_table<TABLES >= 1>(lds_tf_, P.tf, P.R, lds_dalpha, TABLES == 2 ? P.R : 0);
    float *dtf_g = P.d_tf;

    const int p = bundle_ray();
    if (p < P.N) {
        const GradView dv = P.dvol;
        const bool want_vol = dv.p != nullptr;
        const bool want_tf = P.d_tf != nullptr;
        Ray<VT> ray;
        open_bundle_ray<true>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd);
        const int m = depth_samples(ray.rg.n, P.S);

        CompositeDepth c;
        VoxelRun1 run;
        for (int s = 0; s < m; ++s) {
            if (!(c.A < 0.99f)) break;
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            classify(ray.vol, tf, P.R, P.tf_len, P.inv_sr, sm);
            float f;
            const float t = sample_t(ray.rg, s, f);
            const float T = c.add(t, sm.op);
            const bool last = (s == m - 1) || !(c.A < 0.99f);
            const float a_bar = depth_alpha_adjoint(sm, t, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr);
            if (want_tf) {
                const float w0 = (1.0f - sm.fr) * a_bar, w1 = sm.fr * a_bar;
                if (TABLES == 2) {
                    atomicAdd(lds_dalpha + sm.lo, (double)w0); atomicAdd(lds_dalpha + sm.hi, (double)w1);
                } else {
                    unsafeAtomicAdd(dtf_g + 4 * sm.lo + 3, w0); unsafeAtomicAdd(dtf_g + 4 * sm.hi + 3, w1);
                }
            }
            if (want_vol) {
                Cell cell;
                tri_cell(ray.vol, sm.px, sm.py, sm.pz, cell);   // (the tap's own cell: classify's tri_sample splits the same position)
                if (!run.same(cell)) { run.flush(dv, ray.vol.VX, ray.vol.VY, ray.vol.VZ); run.start(cell); }
                run.add(cell, depth_intensity_adjoint(sm, tf[sm.lo].w, tf[sm.hi].w, a_bar, P.tf_len));
            }
        }
        run.flush(dv, ray.vol.VX, ray.vol.VY, ray.vol.VZ);
    }
    if (P.d_tf && TABLES == 2) {
        __syncthreads();
        for (int k = threadIdx.x; k < P.R; k += 256) {
            const float v = (float)lds_dalpha[k];
            if (v == 0.0f) continue;
            unsafeAtomicAdd(dtf_g + 4 * k + 3, v);
        }
    }
}

// d origin and d direction of one ray: march_depth_cam_kernel's walk, frozen branches (n, the live samples, the jitter draw, the
// slab faces, the t_near clamp, every tap's cell, 0 < xtf) and four sums. Per sample
//   P_s = I_bar grad I  (the one tap; H_s = D_s = 0: no lighting),   e_s = T_s op_s (g.x + 2 g.y t_s)  (t_s in the integrand),
// and with gv = P_s.d + e_s = dL/dt_s: sP += P_s, sTP += t_s P_s, s0 += (1 - f_s) gv, s1 += f_s gv; then dr_bundle.h's
// once-per-ray tail. d dir is the gradient w.r.t. the direction as a free 3-vector WITH t_s THE MARCH PARAMETER: t_s does not
// depend on the direction except through the slab distances (the tail's rows), so e_s enters s0 and s1 only -- there is no
// radial term 2 t_s e_s d, which the dot product (pos - o).d of a free d would add. No reduction, no atomic, no static LDS: each
// lane stores its six floats.
template <typename VT, bool TF_LDS>
__global__ __launch_bounds__(256) void depth_bundle_ray_grad_kernel(DepthBundleParams<VT> P) {
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
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = min(depth_samples(rg.n, P.S), P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        const float4 go = ray.go, of = ray.of;
        f3 sP = make_f3(0.f, 0.f, 0.f), sTP = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f;
        CompositeDepth c;
        for (int s = 0; s < m; ++s) {
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            f3 gI;
            sm.I = tri_sample_grad(vol, sm.px, sm.py, sm.pz, gI);
            classify_from_I(tf, P.R, P.tf_len, P.inv_sr, sm);
            float f;
            const float t = sample_t(rg, s, f);
            const float T = c.add(t, sm.op);
            const bool last = s == m - 1;
            const float a_bar = depth_alpha_adjoint(sm, t, T, c.suffix(go, of), last, go, P.inv_sr);
            const f3 Ps = f3_scale(depth_intensity_adjoint(sm, tf[sm.lo].w, tf[sm.hi].w, a_bar, P.tf_len), gI);
            const float es = (T * sm.op) * (go.x + 2.0f * go.y * t);
            const float gv = dot3(Ps, vd) + es;
            sP = f3_add(sP, Ps);
            sTP = f3_fma(t, Ps, sTP);
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }
        const float u = P.jitter_seed != 0u ? jitter_u(P.jitter_seed, P.ray_base, (uint32_t)p) : 0.0f;
        bundle_ray_tail(lf, vd, rg.n, u, P.t_near, sP, sTP, s0, s1, d_o, d_d);
    }
    const size_t q = 3 * (size_t)p;
    P.d_origins[q] = d_o.x; P.d_origins[q + 1] = d_o.y; P.d_origins[q + 2] = d_o.z;
    P.d_dirs[q] = d_d.x; P.d_dirs[q + 1] = d_d.y; P.d_dirs[q + 2] = d_d.z;
}

template <typename VT>
static DepthBundleParams<VT> make_depth_bundle_params(const MarchArgs &a, const BundleArgs &b) {
    DepthBundleParams<VT> P{make_ray_params<VT>(a)};
    P.cam = b.origins;
    P.N = b.N; P.fwd_steps = b.steps; P.t_near = b.t_near; P.jitter_seed = b.jitter_seed; P.ray_base = b.ray_base;
    P.d_origins = b.d_origins; P.d_dirs = b.d_dirs;
    return P;
}

template <typename VT>
static int depth_bundle_fwd_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);
    const DepthBundleParams<VT> P = make_depth_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 1 ? march_depth_bundle_fwd_kernel<VT, true> : march_depth_bundle_fwd_kernel<VT, false>, b.N, t.lds,
                         stream, P);
}

int launch_march_depth_bundle_fwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? depth_bundle_fwd_dispatch<__half>(a, b, stream) : depth_bundle_fwd_dispatch<float>(a, b, stream);
}

template <typename VT>
static int depth_bundle_bwd_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, true);
    const DepthBundleParams<VT> P = make_depth_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 2 ? march_depth_bundle_bwd_kernel<VT, 2>
                                       : (t.tables == 1 ? march_depth_bundle_bwd_kernel<VT, 1> : march_depth_bundle_bwd_kernel<VT, 0>),
                         b.N, t.lds, stream, P);
}

int launch_march_depth_bundle_bwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? depth_bundle_bwd_dispatch<__half>(a, b, stream) : depth_bundle_bwd_dispatch<float>(a, b, stream);
}

template <typename VT>
static int depth_bundle_ray_grad_dispatch(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);
    const DepthBundleParams<VT> P = make_depth_bundle_params<VT>(a, b);
    return launch_bundle(t.tables == 1 ? depth_bundle_ray_grad_kernel<VT, true> : depth_bundle_ray_grad_kernel<VT, false>, b.N, t.lds,
                         stream, P);
}

int launch_depth_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? depth_bundle_ray_grad_dispatch<__half>(a, b, stream)
                                 : depth_bundle_ray_grad_dispatch<float>(a, b, stream);
}

}  // namespace dr
