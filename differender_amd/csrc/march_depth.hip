// march_depth.hip -- ray-depth moments of the differentiable march, for gfx950.
// The shape of march_baseline.hip / march_rgba.hip: one lane per ray, a wave per 8x8 pixel tile, 256-thread workgroups, direct
// global gathers, the table in LDS while it fits (dr_tile.h's table_tier), the sequential float32 recurrence and the tape-free
// adjoint (suffix = out - prefix). The samples, their classification and the alpha recurrence are the plain kernels' own
// statements (sample_pos, classify, A = fma(T, op, A)), so channel 3 and `steps` are the bits of march_fwd_baseline_kernel in
// DR_MODE_DIFF. What is composited beside alpha is not colour but the distance t_s of the sample from look_from along the unit
// ray direction, and its square: pixel = (sum T_s op_s t_s, sum T_s op_s t_s^2, 0, A). Depth needs the table's alpha only: a
// sample is ONE trilinear tap -- no normal, no shading.
// The camera gradient is the third kernel: D8's four per-ray sums (camera_grad.hip) without lighting terms and with one new
// direct term, because t_s is in the integrand itself; dr_camera.h's once-per-ray tails and reductions.
#include "dr_camera.h"
#include "dr_depth.h"

namespace dr {

template <typename VT>
struct DepthParams : RayParams<VT> {};

template <typename VT, bool TF_LDS>
__global__ __launch_bounds__(256) void march_depth_fwd_kernel(DepthParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, P.R);

    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    Ray<VT> ray;
    open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
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

// TABLES: march_bwd_baseline_kernel's tiers (table_tier). Only the alpha column of d_tf receives anything, so a sample sends
// two adds, not eight, and the gradient table of tier 2 is [R] doubles (within the [R][4] the tier budgets); the colour
// columns of the caller's d_tf are never written.
template <typename VT, int TABLES>
__global__ __launch_bounds__(256) void march_depth_bwd_kernel(DepthParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    double *lds_dalpha = reinterpret_cast<double *>(lds_tf_ + P.R);
    const float4 *tf = stage_table<TABLES >= 1>(lds_tf_, P.tf + view * P.tf_vs, P.R, lds_dalpha, TABLES == 2 ? P.R : 0);
    float *dtf_g = P.d_tf ? P.d_tf + view * P.dtf_vs * 4 : nullptr;

    int i, j;
    if (tile_pixel(P.W, P.H, i, j)) {
        GradView dv = P.dvol;
        const bool want_vol = dv.p != nullptr;
        const bool want_tf = P.d_tf != nullptr;
        const size_t p = ray_index(P.W, P.H, view, i, j);
        Ray<VT> ray;
        open_ray<true>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd,
                       want_vol ? &dv : nullptr, P.dvol_vs);
        const int m = depth_samples(ray.rg.n, P.S);

        CompositeDepth c;
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
            if (want_vol)
                tri_scatter_global(ray.vol, dv, sm.px, sm.py, sm.pz,
                                   depth_intensity_adjoint(sm, tf[sm.lo].w, tf[sm.hi].w, a_bar, P.tf_len));
        }
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

// What the camera gradient reads beside the march's parameters (camera_grad.hip's CamParams; no row bands: the buffers are the
// whole image)
template <typename VT>
struct DepthCamParams : RayParams<VT> {
    const int32_t *fwd_steps;   // the forward's live samples per ray
    CamFields cf;               // (aspect: W / H)
};

// Gradient of the depth march w.r.t. look_from ([views][3]) or, POSE, the free camera's ten parameters. camera_grad_kernel's
// shape and frozen branches (n, the live samples, the jitter draw, the slab faces, the cells, 0 < xtf). Per sample
//   P_s = I_bar grad I  (the one tap; H_s = D_s = 0: no lighting),   e_s = T_s op_s (g.x + 2 g.y t_s)  (t_s in the integrand),
// and with gv = P_s.vd + e_s = dL/dt_s the four sums are sP += P_s, sTG += t_s P_s, s0 += (1 - f_s) gv, s1 += f_s gv: the tails
// of dr_camera.h take them as they are.
constexpr size_t DEPTH_RED_BYTES = 3 * 256 * sizeof(double);   // the reductions' static LDS, beside the table
template <typename VT, bool TF_LDS, bool POSE>
__global__ __launch_bounds__(256) void march_depth_cam_kernel(DepthCamParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    __shared__ double red[3][256];
    static_assert(sizeof(red) == DEPTH_RED_BYTES, "depth_cam_dispatch budgets the table beside it");
    const int view = blockIdx.y;
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, P.R);

    f3 dcam = make_f3(0.f, 0.f, 0.f);
    PoseGrad dpose = pose_zero();
    int i, j;
    const bool in_img = tile_pixel(P.W, P.H, i, j);
    const size_t p = ray_index(P.W, P.H, view, i, j);
    // H6: a single-sample ray sits at 0/0 in the reference and contributes nothing
    if (in_img && P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = min(depth_samples(rg.n, P.S), P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        const float4 go = ray.go, of = ray.of;
        f3 sP = make_f3(0.f, 0.f, 0.f), sTG = make_f3(0.f, 0.f, 0.f);
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
            sTG = f3_fma(t, Ps, sTG);
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }

        if (POSE) {
            // once per ray: the ten pose gradients from the four sums (dr_camera.h), then D5
            const PoseRay q = pose_ray(P.cf.pose, P.cf.fov_v, view, P.cf.near_d, P.cf.aspect, P.cf.near_w, P.cf.near_h, i, P.W, j,
                                       P.H, rg.n, P.cf.jitter_seed, P.cf.view_base + (uint32_t)view);
            dpose = pose_finite(pose_ray_grad(lf, q, vd, P.cf.near_, sP, sTG, s0 * q.A, fmaf(s0, 1.0f - q.A, s1)));
        } else {
            // once per ray: J_vd, the rows of the slab faces the forward picked and the jitter draw behind grad t0
            M3 J;
            f3 g_tmin, g_tmax, g_t0;
            float u;
            camera_ray_tail(lf, vd, i, P.W, j, P.H, P.cf.near_, P.cf.near_w, P.cf.near_h, rg.n, P.cf.jitter_seed,
                            P.cf.view_base + (uint32_t)view, J, g_tmin, g_tmax, g_t0, u);
            dcam = f3_add(sP, mul_t(J, sTG));
            dcam = f3_fma(s0, g_t0, dcam);
            dcam = f3_fma(s1, g_tmax, dcam);
            // D5: a NaN ray (NaN upstream gradient or pixel) contributes nothing, infinities are clamped
            dcam = make_f3(finite_or_zero(dcam.x), finite_or_zero(dcam.y), finite_or_zero(dcam.z));
        }
    }
    if (POSE) pose_reduce(dpose, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
    else camera_reduce(dcam, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
}

template <typename VT>
static int depth_fwd_dispatch(const MarchArgs &a, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);
    const DepthParams<VT> P{make_ray_params<VT>(a)};
    return launch_tiles(t.tables == 1 ? march_depth_fwd_kernel<VT, true> : march_depth_fwd_kernel<VT, false>, a, t.lds, stream, P);
}

int launch_march_depth_fwd(const MarchArgs &a, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? depth_fwd_dispatch<__half>(a, stream) : depth_fwd_dispatch<float>(a, stream);
}

template <typename VT>
static int depth_bwd_dispatch(const MarchArgs &a, hipStream_t stream) {
    const TableTier t = table_tier(a.R, true);
    const DepthParams<VT> P{make_ray_params<VT>(a)};
    return launch_tiles(t.tables == 2 ? march_depth_bwd_kernel<VT, 2>
                                      : (t.tables == 1 ? march_depth_bwd_kernel<VT, 1> : march_depth_bwd_kernel<VT, 0>),
                        a, t.lds, stream, P);
}

int launch_march_depth_bwd(const MarchArgs &a, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? depth_bwd_dispatch<__half>(a, stream) : depth_bwd_dispatch<float>(a, stream);
}

template <typename VT, bool POSE>
static int depth_cam_dispatch(const MarchArgs &a, const CamArgs &c, hipStream_t stream) {
    DepthCamParams<VT> P{make_ray_params<VT>(a)};
    P.fwd_steps = c.steps;
    P.cf = fill_cam_fields(a, c.jitter_seed, c.view_base, c.d_cam, c.d_cam_ray);
    const TableTier t = table_tier(a.R, false, 0, DEPTH_RED_BYTES);   // the table beside the reductions' static LDS
    if (t.tables == 1) return launch_tiles(march_depth_cam_kernel<VT, true, POSE>, a, t.lds - DEPTH_RED_BYTES, stream, P);
    return launch_tiles(march_depth_cam_kernel<VT, false, POSE>, a, 0, stream, P);   // a large TF is read where it lies
}

// MarchArgs::pose null: d look_from into c.d_cam [n_views][3]; else the ten pose gradients into [n_views][10]
int launch_march_depth_bwd_cam(const MarchArgs &a, const CamArgs &c, hipStream_t stream) {
    if (a.pose)
        return a.vol_dtype == DR_F16 ? depth_cam_dispatch<__half, true>(a, c, stream) : depth_cam_dispatch<float, true>(a, c, stream);
    return a.vol_dtype == DR_F16 ? depth_cam_dispatch<__half, false>(a, c, stream) : depth_cam_dispatch<float, false>(a, c, stream);
}

}  // namespace dr
