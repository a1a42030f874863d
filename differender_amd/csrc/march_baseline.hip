// march_baseline.hip -- DR_VARIANT_BASELINE march kernels for gfx950: one lane per ray, a wave per
// 8x8 pixel tile, direct global gathers, TF table in LDS, global float atomics for d_vol.
// Kept as the simplest correct device implementation; the optimised kernels are tested against it
// and against the CPU oracle.
//
// Forward   : VR.py:261-306 (raycast) + 363-372 (get_final_image); nondiff: VR.py:308-361.
// Backward  : tape-free equivalent of raycast.grad/get_final_image.grad (VR.py:460-461,470-471).
//   With T_s = 1 - A_{s-1} and q_s = gC.(L_s rgb_s) + gA the adjoint of the sample opacity is
//   d/d op_s = T_s q_s - [gC.(C_final - C_s) + gA.(A_final - A_s)] / (1 - op_s)   (C_s, A_s = composite up to s),
//   which needs only a forward-order walk and the saved forward output (no per-sample tape).
#include "dr_tile.h"

namespace dr {

template <typename VT>
struct MarchParams : RayParams<VT> {
    const uint8_t *only_flagged;
    const unsigned int *ws_mark; unsigned int ws_mark_expect;  // see RayFilter
    const unsigned int *ws_aux; unsigned int ws_aux_expect;
};

// TF_LDS: the transfer function is staged in LDS (R <= 10176 entries = 159 KiB: what a workgroup is really granted, less headroom); a larger one is read where it lies, through the
// caches -- the reference has no limit on the TF resolution, and neither have the plain kernels.
template <typename VT, int MODE, bool TF_LDS>
__global__ __launch_bounds__(256) void march_fwd_baseline_kernel(MarchParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    const float4 *lds_tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, P.R);

    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    Ray<VT> ray;
    open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const f3 light = make_f3(ray.cam.x + 0.0f, ray.cam.y + 1.0f, ray.cam.z + 0.0f);
    const int nmarch = (MODE == DR_MODE_DIFF && ray.rg.n > P.S) ? P.S : ray.rg.n;

    Composite c;
    int cnt = 0;
    for (int s = 0; s < nmarch; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        classify(ray.vol, lds_tf, P.R, P.tf_len, P.inv_sr, sm);
        ++cnt;
        if (MODE == DR_MODE_NONDIFF && !(sm.a > 1e-3f)) continue;
        shade(ray.vol, light, ray.vd, MODE == DR_MODE_DIFF, sm);
        c.add(sm);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(MODE == DR_MODE_NONDIFF);
    if (P.steps) P.steps[p] = cnt;
}

// TABLES: what the workgroup keeps in LDS --
//   2: [R] TF + [R][4] d_tf accumulators in double (48 R bytes: R <= 3392);
//   1: the TF only; d_tf contributions go straight to the caller's tensor with float atomics (16 R bytes: R <= 10176; at such
//      resolutions a texel collects few samples of a workgroup, so the summation noise the double table exists for -- dtf_add -- is
//      not a concern);
//   0: nothing: the TF is read where it lies (any R; the reference has no limit on the TF resolution).
template <typename VT, int TABLES>
__global__ __launch_bounds__(256) void march_bwd_baseline_kernel(MarchParams<VT> P) {
    // TABLES == 2: [R] TF, then [R][4] d_tf accumulators in double (dr_tile.h's dtf_add says why: fuzz seed 603239)
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    double *lds_dtf = reinterpret_cast<double *>(lds_tf_ + P.R);
    const float4 *lds_tf = stage_table<TABLES >= 1>(lds_tf_, P.tf + view * P.tf_vs, P.R, lds_dtf, TABLES == 2 ? 4 * P.R : 0);
    float *dtf_g = P.d_tf ? P.d_tf + view * P.dtf_vs * 4 : nullptr;

    int i, j;
    bool active = tile_pixel(P.W, P.H, i, j);
    // second pass of the brick-centric backward: only the rays the forward flagged -- unless the workspace is not that
    // forward's (uniform): then the flags mean nothing, B1 has done nothing, and every ray is marched here
    const bool stale_ws = (P.ws_mark != nullptr && *P.ws_mark != P.ws_mark_expect) || (P.ws_aux != nullptr && *P.ws_aux != P.ws_aux_expect);
    if (stale_ws && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        atomicAdd(const_cast<unsigned int *>(P.ws_mark) + 6, 1u);   // header word 9 (ST_STALE_BWD): the host layer warns
    // (flag 1: irregular rays; 2 = rays of the exact pass, whose backward is ray_exact_bwd_kernel's)
    if (active && P.only_flagged && !stale_ws) active = P.only_flagged[ray_index(P.W, P.H, view, i, j)] == 1;
    if (active) {
        GradView dv = P.dvol;
        const bool want_vol = dv.p != nullptr;
        const bool want_tf = P.d_tf != nullptr;
        const size_t p = ray_index(P.W, P.H, view, i, j);
        Ray<VT> ray;
        open_ray<true>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd,
                       want_vol ? &dv : nullptr, P.dvol_vs);
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
            SampleAdj ad;
            sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
            float I_bar = want_vol ? intensity_adjoint(sm, lds_tf[sm.lo], lds_tf[sm.hi], ad, P.tf_len) : 0.0f;
            if (P.only_flagged) {
                // second pass of the brick-centric backward (irregular rays): that path promises finite gradients, so a NaN
                // adjoint is dropped and infinities are clamped here too (dr_march_bwd_variant). On its own, the baseline
                // propagates NaN like the reference.
                ad.r_bar = finite_or_zero(ad.r_bar); ad.g_bar = finite_or_zero(ad.g_bar); ad.b_bar = finite_or_zero(ad.b_bar);
                ad.a_bar = finite_or_zero(ad.a_bar); ad.gx = finite_or_zero(ad.gx); ad.gy = finite_or_zero(ad.gy);
                ad.gz = finite_or_zero(ad.gz); I_bar = finite_or_zero(I_bar);
            }
            if (want_tf && TABLES < 2) dtf_add(dtf_g, sm, ad, P.only_flagged != nullptr);
            else if (want_tf) dtf_add(lds_dtf, sm, ad);
            if (want_vol) scatter_taps(ray.vol, dv, sm, I_bar, ad.gx, ad.gy, ad.gz);
        }
    }
    if (P.d_tf && TABLES == 2) {
        __syncthreads();
        float *dtf = dtf_g;
        for (int k = threadIdx.x; k < 4 * P.R; k += 256) {
            const float v = (float)lds_dtf[k];
            if (v == 0.0f) continue;
            if (P.only_flagged) atomic_add_sat(dtf + k, v);  // second pass of the sanitising backward: the sum stays finite
            else unsafeAtomicAdd(dtf + k, v);
        }
    }
}

template <typename VT>
static MarchParams<VT> make_params(const MarchArgs &a, const RayFilter &f = RayFilter{}) {
    MarchParams<VT> P{make_ray_params<VT>(a)};
    P.only_flagged = f.only_flagged;
    P.ws_mark = f.ws_mark; P.ws_mark_expect = f.ws_mark_expect;
    P.ws_aux = f.ws_aux; P.ws_aux_expect = f.ws_aux_expect;
    return P;
}

template <typename VT>
static int fwd_dispatch(const MarchArgs &a, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);   // (R <= 10176; a larger TF is read from global memory)
    const bool tf_lds = t.tables == 1;
    const MarchParams<VT> P = make_params<VT>(a);
    if (a.mode == DR_MODE_DIFF)
        return launch_tiles(tf_lds ? march_fwd_baseline_kernel<VT, DR_MODE_DIFF, true> : march_fwd_baseline_kernel<VT, DR_MODE_DIFF, false>,
                            a, t.lds, stream, P);
    return launch_tiles(tf_lds ? march_fwd_baseline_kernel<VT, DR_MODE_NONDIFF, true> : march_fwd_baseline_kernel<VT, DR_MODE_NONDIFF, false>,
                        a, t.lds, stream, P);
}

int launch_march_fwd_baseline(const MarchArgs &a, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? fwd_dispatch<__half>(a, stream) : fwd_dispatch<float>(a, stream);
}

template <typename VT>
static int bwd_dispatch(const MarchArgs &a, const RayFilter &f, hipStream_t stream) {
    // TF + its double-precision gradient table in LDS while they fit (R <= 3392), then the TF alone (R <= 10176), then nothing
    const TableTier t = table_tier(a.R, true);
    const MarchParams<VT> P = make_params<VT>(a, f);
    return launch_tiles(t.tables == 2 ? march_bwd_baseline_kernel<VT, 2> : (t.tables == 1 ? march_bwd_baseline_kernel<VT, 1> : march_bwd_baseline_kernel<VT, 0>),
                        a, t.lds, stream, P);
}

int launch_march_bwd_baseline(const MarchArgs &a, const RayFilter &f, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? bwd_dispatch<__half>(a, f, stream) : bwd_dispatch<float>(a, f, stream);
}

}  // namespace dr
