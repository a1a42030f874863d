// march_lit.hip -- the 1-D TF march with a free light and Phong material, gfx950: dr_march_lit_fwd / _bwd.
// The reference shades with a white light at look_from + (0,1,0), ambient 0.4, diffuse 0.8, specular 0.3, shininess 32
// (VR.py:91-95, 281-299); here these are ten per-view parameters light[view][10] (dr_light.h), and the backward also returns
// their gradients. Everything else is march_baseline.hip's: one lane per ray, a wave per 8x8 pixel tile, direct global gathers,
// the TF in LDS, global float atomics for d_vol; positions, jitter, n, the max_samples clip, the TF lookup, the six normal taps,
// D1's flat normals and the termination at A >= 0.99 are the same statements, and what surrounds the sample loops is the same
// code (dr_tile.h: open_ray's parts, dtf_add, scatter_taps). At the reference's values the forward image is
// DR_VARIANT_BASELINE's bit for bit.
//
// Forward   : VR.py:261-306 + 363-372; nondiff: VR.py:308-361.
// Backward  : march_bwd_baseline_kernel's tape-free walk (same frozen branches) with sample_adjoint_lit; the ten lighting sums
//   are f32 per ray, D5 once per ray, f64 per workgroup, one f64 atomic per component and workgroup (light_reduce).
#include "dr_light.h"
#include "dr_tile.h"

namespace dr {

template <typename VT>
struct LitParams : RayParams<VT> {
    const float *light;                     // [views][10]
    double *d_light; float *d_light_ray;    // backward: [views][10] accumulated; [views][W][H][10] overwritten; nullable
};

template <typename VT, int MODE, bool TF_LDS>
__global__ __launch_bounds__(256) void march_lit_fwd_kernel(LitParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    const float4 *lds_tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, P.R);

    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    Ray<VT> ray;
    open_view(ray, view, P.vol, P.vol_vs, P.cam);
    const Light lt = load_light(P.light + 10 * view);   // uniform per blockIdx.y: scalar loads, once
    const bool sh32 = lt.sh == 32.0f;
    open_geom<false>(ray, p, P.entry, P.exit_, P.rays, P.nsamp);
    const int nmarch = (MODE == DR_MODE_DIFF && ray.rg.n > P.S) ? P.S : ray.rg.n;

    CompositeLit c;
    int cnt = 0;
    for (int s = 0; s < nmarch; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        classify(ray.vol, lds_tf, P.R, P.tf_len, P.inv_sr, sm);
        ++cnt;
        if (MODE == DR_MODE_NONDIFF && !(sm.a > 1e-3f)) continue;
        shade_lit(ray.vol, lt, sh32, ray.vd, MODE == DR_MODE_DIFF, sm);
        c.add_lit(sm, lt.lc);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(MODE == DR_MODE_NONDIFF);
    if (P.steps) P.steps[p] = cnt;
}

// TABLES: march_bwd_baseline_kernel's tiers -- 2: TF + the double d_tf table in LDS; 1: the TF only (d_tf by float atomics);
// 0: nothing. LIGHT: d_light or d_light_ray is wanted (else no lighting sums are formed and nothing is reduced).
template <typename VT, int TABLES, bool LIGHT>
__global__ __launch_bounds__(256) void march_lit_bwd_kernel(LitParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    double *lds_dtf = reinterpret_cast<double *>(lds_tf_ + P.R);
    const float4 *lds_tf = stage_table<TABLES >= 1>(lds_tf_, P.tf + view * P.tf_vs, P.R, lds_dtf, TABLES == 2 ? 4 * P.R : 0);
    float *dtf_g = P.d_tf ? P.d_tf + view * P.dtf_vs * 4 : nullptr;

    int i, j;
    const bool active = tile_pixel(P.W, P.H, i, j);
    const size_t p = ray_index(P.W, P.H, view, i, j);
    LightGrad lg = light_zero();
    if (active) {
        GradView dv = P.dvol;
        const bool want_vol = dv.p != nullptr;
        const bool want_tf = P.d_tf != nullptr;
        Ray<VT> ray;
        open_view(ray, view, P.vol, P.vol_vs, P.cam, want_vol ? &dv : nullptr, P.dvol_vs);
        const Light lt = load_light(P.light + 10 * view);
        const bool sh32 = lt.sh == 32.0f;
        open_geom<true>(ray, p, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd);
        const int nmarch = ray.rg.n > P.S ? P.S : ray.rg.n;
        const float4 go = ray.go;

        CompositeLit c;
        for (int s = 0; s < nmarch; ++s) {
            if (!(c.A < 0.99f)) break;
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            classify(ray.vol, lds_tf, P.R, P.tf_len, P.inv_sr, sm);
            const float Pw = shade_lit(ray.vol, lt, sh32, ray.vd, true, sm);
            const float T = c.add_lit(sm, lt.lc);
            const bool last = (s == nmarch - 1) || !(c.A < 0.99f);
            SampleAdj ad;
            sample_adjoint_lit<LIGHT>(sm, Pw, lt, sh32, ray.vd, T, c.suffix(go, ray.of), last, go, P.inv_sr, ad, lg);
            if (want_tf && TABLES < 2) dtf_add(dtf_g, sm, ad, false);
            else if (want_tf) dtf_add(lds_dtf, sm, ad);
            if (want_vol)
                scatter_taps(ray.vol, dv, sm, intensity_adjoint(sm, lds_tf[sm.lo], lds_tf[sm.hi], ad, P.tf_len), ad.gx, ad.gy, ad.gz);
        }
        // D5, once per ray. A NaN channel of the upstream gradient drops the whole ray, not only the sums it reaches: d lc_k
        // reads go_k alone and no lighting sum reads go.a, and a ray that gave some of its ten columns would be no gradient
        if (LIGHT) lg = (go.x == go.x && go.y == go.y && go.z == go.z && go.w == go.w) ? light_finite(lg) : light_zero();
    }
    if (P.d_tf && TABLES == 2) {
        __syncthreads();
        for (int k = threadIdx.x; k < 4 * P.R; k += 256) {
            const float v = (float)lds_dtf[k];
            if (v == 0.0f) continue;
            unsafeAtomicAdd(dtf_g + k, v);
        }
    }
    // (after the d_tf flush: the reduction's 320 B overlay the head of the dynamic region, which a short table shares with lds_dtf)
    if (LIGHT) light_reduce(lg, active, p, view, P.d_light_ray, P.d_light, reinterpret_cast<double *>(lds_tf_));
}

template <typename VT>
static LitParams<VT> make_lit_params(const MarchArgs &a, const LitArgs &q) {
    LitParams<VT> P{make_ray_params<VT>(a)};
    P.light = q.light; P.d_light = q.d_light; P.d_light_ray = q.d_light_ray;
    return P;
}

template <typename VT>
static int lit_fwd_dispatch(const MarchArgs &a, const LitArgs &q, hipStream_t stream) {
    const TableTier t = table_tier(a.R, false);   // (R <= 10176; a larger TF is read from global memory)
    const bool tf_lds = t.tables == 1;
    const LitParams<VT> P = make_lit_params<VT>(a, q);
    if (a.mode == DR_MODE_DIFF)
        return launch_tiles(tf_lds ? march_lit_fwd_kernel<VT, DR_MODE_DIFF, true> : march_lit_fwd_kernel<VT, DR_MODE_DIFF, false>,
                            a, t.lds, stream, P);
    return launch_tiles(tf_lds ? march_lit_fwd_kernel<VT, DR_MODE_NONDIFF, true> : march_lit_fwd_kernel<VT, DR_MODE_NONDIFF, false>,
                        a, t.lds, stream, P);
}

int launch_march_lit_fwd(const MarchArgs &a, const LitArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? lit_fwd_dispatch<__half>(a, q, stream) : lit_fwd_dispatch<float>(a, q, stream);
}

template <typename VT, bool LIGHT>
static int lit_bwd_dispatch(const MarchArgs &a, const LitArgs &q, hipStream_t stream) {
    // the baseline's tiers, and never less than the reduction's own bytes
    static_assert(table_tier(2, true, LIGHT_RED_BYTES).tables == 2 && table_tier(2, true, LIGHT_RED_BYTES).lds == LIGHT_RED_BYTES,
                  "a short table: the reduction's bytes");
    const TableTier t = table_tier(a.R, true, LIGHT ? LIGHT_RED_BYTES : 0);
    const LitParams<VT> P = make_lit_params<VT>(a, q);
    return launch_tiles(t.tables == 2 ? march_lit_bwd_kernel<VT, 2, LIGHT>
                                      : (t.tables == 1 ? march_lit_bwd_kernel<VT, 1, LIGHT> : march_lit_bwd_kernel<VT, 0, LIGHT>),
                        a, t.lds, stream, P);
}

int launch_march_lit_bwd(const MarchArgs &a, const LitArgs &q, hipStream_t stream) {
    if (q.d_light || q.d_light_ray)
        return a.vol_dtype == DR_F16 ? lit_bwd_dispatch<__half, true>(a, q, stream) : lit_bwd_dispatch<float, true>(a, q, stream);
    return a.vol_dtype == DR_F16 ? lit_bwd_dispatch<__half, false>(a, q, stream) : lit_bwd_dispatch<float, false>(a, q, stream);
}

}  // namespace dr
