// march_tf2d.hip -- the march with a 2-D (value, gradient-magnitude) transfer function, for gfx950.
// The shape of march_baseline.hip: one lane per ray, a wave per 8x8 pixel tile, 256-thread workgroups, direct global
// gathers, the sequential float32 recurrence and the tape-free adjoint (suffix = out - prefix). Only the classification
// differs from the 1-D march: the six normal taps come first, and their length u = |grad| * g_scale is the second TF axis.
//   xv = I (RV - 1), xg = u (RG - 1); low_high_frac and the H4/H5 clamp on each axis;
//   rgba = mix(mix(T[v0][g0], T[v1][g0], fv), mix(T[v0][g1], T[v1][g1], fv), fg)   (value axis first, dr_device.h's mixf)
// With RG == 1, fg = 0 and mix(x, x, 0) = x: a (RV, 1) table is bit for bit the 1-D TF of RV entries.
#include "dr_tile.h"

namespace dr {

// RayParams is all the 2-D TF reads: the table is [RV][RG] with RV = R, and lv = RV - 1 is tf_len (a type of its own all
// the same: the kernels' signatures, which profiles name, stay as they were)
template <typename VT>
struct Tf2dParams : RayParams<VT> {};

// The classification of one sample: indices and fractions on both axes, the four texels and the two value-axis lerps.
struct Tf2dSample {
    float xv, xg, fv, fg;
    int v0, v1, g0, g1;   // table rows (value) and columns (gradient)
    float4 a, b, c, d;    // T[v0][g0], T[v1][g0], T[v0][g1], T[v1][g1]
    float4 lo, hi;        // mix(a, b, fv), mix(c, d, fv)
};

__device__ __forceinline__ void axis_index(float x, int R, int &i0, int &i1, float &fr) {
    low_high_frac(x, i0, fr);
    i0 = min(i0, R - 1);
    i1 = min(i0 + 1, R - 1);
}

// sm.I and sm.gnorm must be set; writes sm.r, g, b, a and sm.op
template <typename VT>
__device__ __forceinline__ void classify2d(const Tf2dParams<VT> &P, const float4 *tf, Sample &sm, Tf2dSample &t) {
    const float u = sm.gnorm * P.g_scale;
    t.xv = sm.I * P.tf_len;
    t.xg = u * P.lg;
    axis_index(t.xv, P.R, t.v0, t.v1, t.fv);
    axis_index(t.xg, P.RG, t.g0, t.g1, t.fg);
    t.a = tf[t.v0 * P.RG + t.g0]; t.b = tf[t.v1 * P.RG + t.g0];
    t.c = tf[t.v0 * P.RG + t.g1]; t.d = tf[t.v1 * P.RG + t.g1];
    t.lo = mix4(t.a, t.b, t.fv);
    t.hi = mix4(t.c, t.d, t.fv);
    sm.r = mixf(t.lo.x, t.hi.x, t.fg); sm.g = mixf(t.lo.y, t.hi.y, t.fg);
    sm.b = mixf(t.lo.z, t.hi.z, t.fg); sm.a = mixf(t.lo.w, t.hi.w, t.fg);
    sm.op = opacity_of_alpha(sm.a, P.inv_sr);
}

// The non-differentiable march skips samples with alpha <= 1e-3 (VR.py:334). Every alpha a sample of value rows v0, v1 can
// take is a convex combination of their texels, rounded four times: at most max(rowmax[v0], rowmax[v1]) (1 + 2^-21). Below
// this bound the sample is certain to be skipped, so its six taps are never gathered; the image and steps are those of the
// plain test (a NaN alpha is skipped either way).
constexpr float TF2D_SKIP_BELOW = 9.9999e-4f;

// TF_LDS: the table (and, for the non-differentiable mode, its per-row largest alpha) is staged in LDS; otherwise it is read
// where it lies and every sample is classified.
template <typename VT, int MODE, bool TF_LDS>
__global__ __launch_bounds__(256) void march_tf2d_fwd_kernel(Tf2dParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    const int NT = P.R * P.RG;
    float *rowmax = reinterpret_cast<float *>(lds_tf_ + NT);
    constexpr bool SKIP = TF_LDS && MODE == DR_MODE_NONDIFF;
    const float4 *tf = stage_table<TF_LDS>(lds_tf_, P.tf + view * P.tf_vs, NT);
    if (SKIP) {
        // one wave per row, its lanes across the row's texels, then a butterfly max (the row loop is wave-uniform, so the
        // shuffles run converged): the work is spread alike for tall and for wide tables
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int v = wave; v < P.R; v += 4) {
            float m = -__builtin_inff();
            for (int g = lane; g < P.RG; g += 64) m = fmaxf(m, lds_tf_[v * P.RG + g].w);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            if (lane == 0) rowmax[v] = m;
        }
        __syncthreads();
    }

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
        sm.I = tri_sample(ray.vol, sm.px, sm.py, sm.pz);
        ++cnt;
        if (SKIP) {
            int v0, v1; float fv;
            axis_index(sm.I * P.tf_len, P.R, v0, v1, fv);
            if (fmaxf(rowmax[v0], rowmax[v1]) <= TF2D_SKIP_BELOW) continue;
        }
        shade(ray.vol, light, ray.vd, MODE == DR_MODE_DIFF, sm);   // the taps: sm.gnorm
        Tf2dSample t;
        classify2d(P, tf, sm, t);
        if (MODE == DR_MODE_NONDIFF && !(sm.a > 1e-3f)) continue;
        c.add(sm);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(MODE == DR_MODE_NONDIFF);
    if (P.steps) P.steps[p] = cnt;
}

__device__ __forceinline__ float dot4(float4 x, const SampleAdj &ad) {
    return x.x * ad.r_bar + x.y * ad.g_bar + x.z * ad.b_bar + x.w * ad.a_bar;
}

// d_tf2d contributions of a run of samples in one table cell (the four corner texels i..), summed in f32
struct CellRun {
    int i00 = -1, i10, i01, i11;
    float s00[4], s10[4], s01[4], s11[4];
    __device__ __forceinline__ void start(int a, int b, int c, int d) {
        i00 = a; i10 = b; i01 = c; i11 = d;
#pragma unroll
        for (int q = 0; q < 4; ++q) s00[q] = s10[q] = s01[q] = s11[q] = 0.0f;
    }
    __device__ __forceinline__ void flush(float *dtf) const {
        if (i00 < 0) return;
        float *d00 = dtf + 4 * (size_t)i00, *d10 = dtf + 4 * (size_t)i10, *d01 = dtf + 4 * (size_t)i01, *d11 = dtf + 4 * (size_t)i11;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsafeAtomicAdd(d00 + q, s00[q]); unsafeAtomicAdd(d10 + q, s10[q]);
            unsafeAtomicAdd(d01 + q, s01[q]); unsafeAtomicAdd(d11 + q, s11[q]);
        }
    }
};

// TABLES: what the workgroup keeps in LDS, by texel count P = RV * RG (march_baseline.hip's tiers) --
//   2: the TF + its gradient table in double (48 P bytes: P <= 3392; only when d_tf2d is wanted);
//   1: the TF only; d_tf2d by float atomics on the caller's tensor, one set per run of samples in a cell (16 P bytes: P <= 10176);
//   0: nothing: the TF is read where it lies (d_tf2d as in tier 1).
template <typename VT, int TABLES>
__global__ __launch_bounds__(256) void march_tf2d_bwd_kernel(Tf2dParams<VT> P) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tf_[];
    const int view = blockIdx.y;
    const int NT = P.R * P.RG;
    double *lds_dtf = reinterpret_cast<double *>(lds_tf_ + NT);
    const float4 *tf = stage_table<TABLES >= 1>(lds_tf_, P.tf + view * P.tf_vs, NT, lds_dtf, TABLES == 2 ? 4 * NT : 0);
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
        const f3 light = make_f3(ray.cam.x + 0.0f, ray.cam.y + 1.0f, ray.cam.z + 0.0f);
        const int nmarch = ray.rg.n > P.S ? P.S : ray.rg.n;

        Composite c;
        CellRun run;
        for (int s = 0; s < nmarch; ++s) {
            if (!(c.A < 0.99f)) break;
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            sm.I = tri_sample(ray.vol, sm.px, sm.py, sm.pz);
            shade(ray.vol, light, ray.vd, true, sm);
            Tf2dSample t;
            classify2d(P, tf, sm, t);
            const float T = c.add(sm);
            const bool last = (s == nmarch - 1) || !(c.A < 0.99f);
            SampleAdj ad;
            sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);

            if (want_tf) {
                // d rgba / d T[.][.]: the four bilinear weights
                const float w00 = (1.0f - t.fv) * (1.0f - t.fg), w10 = t.fv * (1.0f - t.fg);
                const float w01 = (1.0f - t.fv) * t.fg, w11 = t.fv * t.fg;
                const int i00 = t.v0 * P.RG + t.g0, i10 = t.v1 * P.RG + t.g0;   // texel indices (< 2^31)
                const int i01 = t.v0 * P.RG + t.g1, i11 = t.v1 * P.RG + t.g1;
                const float adj[4] = {ad.r_bar, ad.g_bar, ad.b_bar, ad.a_bar};
                if (TABLES == 2) {   // (the products are f32, as in the 1-D backward)
                    const int k00 = 4 * i00, k10 = 4 * i10, k01 = 4 * i01, k11 = 4 * i11;   // (P <= 3392)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        atomicAdd(lds_dtf + k00 + q, (double)(w00 * adj[q])); atomicAdd(lds_dtf + k10 + q, (double)(w10 * adj[q]));
                        atomicAdd(lds_dtf + k01 + q, (double)(w01 * adj[q])); atomicAdd(lds_dtf + k11 + q, (double)(w11 * adj[q]));
                    }
                } else {
                    // float atomics on the caller's tensor, one set per RUN of consecutive samples of the ray in one table cell:
                    // neighbouring samples (air, a material's interior) mostly share their cell, and same-address atomics of
                    // thousands of rays are what this tier's time is made of
                    if (i00 != run.i00) { run.flush(dtf_g); run.start(i00, i10, i01, i11); }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        run.s00[q] += w00 * adj[q]; run.s10[q] += w10 * adj[q];
                        run.s01[q] += w01 * adj[q]; run.s11[q] += w11 * adj[q];
                    }
                }
            }
            if (want_vol) {
                // through I: the value-axis slope (1 - fg)(b - a) + fg (d - c), times RV - 1, iff 0 < xv
                const float fv_bar = (1.0f - t.fg) * dot4(sub4(t.b, t.a), ad) + t.fg * dot4(sub4(t.d, t.c), ad);
                const float I_bar = (0.0f < t.xv) ? fv_bar * P.tf_len : 0.0f;
                tri_scatter_global(ray.vol, dv, sm.px, sm.py, sm.pz, I_bar);
                if (!sm.flat) {
                    // through u = |grad| g_scale: the gradient-axis slope hi - lo, times (RG - 1) g_scale, iff 0 < xg, onto the
                    // taps along grad / |grad| -- beside the normal's own adjoint (sample_adjoint)
                    const float fg_bar = dot4(sub4(t.hi, t.lo), ad);
                    const float u_bar = (0.0f < t.xg) ? fg_bar * P.lg : 0.0f;
                    const float k = (u_bar * P.g_scale) * sm.ginv;
                    scatter_normal_taps(ray.vol, dv, sm, fmaf(k, sm.grad.x, ad.gx), fmaf(k, sm.grad.y, ad.gy), fmaf(k, sm.grad.z, ad.gz));
                }
            }
        }
        if (TABLES < 2 && want_tf) run.flush(dtf_g);
    }
    if (P.d_tf && TABLES == 2) {
        __syncthreads();
        for (int k = threadIdx.x; k < 4 * NT; k += 256) {   // (NT <= 3392)
            const float v = (float)lds_dtf[k];
            if (v != 0.0f) unsafeAtomicAdd(dtf_g + k, v);
        }
    }
}

template <typename VT>
static int tf2d_fwd_dispatch(const MarchArgs &a, hipStream_t stream) {
    const size_t NT = (size_t)a.R * a.RG;
    // (beside the table, the non-differentiable mode's largest alpha of each row)
    const TableTier t = table_tier(NT, false, 0, a.mode == DR_MODE_NONDIFF ? (size_t)a.R * sizeof(float) : 0);
    const bool tf_lds = t.tables == 1;
    const Tf2dParams<VT> P{make_ray_params<VT>(a)};
    if (a.mode == DR_MODE_DIFF)
        return launch_tiles(tf_lds ? march_tf2d_fwd_kernel<VT, DR_MODE_DIFF, true> : march_tf2d_fwd_kernel<VT, DR_MODE_DIFF, false>,
                            a, t.lds, stream, P);
    return launch_tiles(tf_lds ? march_tf2d_fwd_kernel<VT, DR_MODE_NONDIFF, true> : march_tf2d_fwd_kernel<VT, DR_MODE_NONDIFF, false>,
                        a, t.lds, stream, P);
}

template <typename VT>
static int tf2d_bwd_dispatch(const MarchArgs &a, hipStream_t stream) {
    const size_t NT = (size_t)a.R * a.RG;
    // (a backward without d_tf2d keeps no gradient table: at 64 x 32 texels the f64 table alone would limit a CU to one
    // workgroup)
    const TableTier t = table_tier(NT, a.d_tf != nullptr);
    const Tf2dParams<VT> P{make_ray_params<VT>(a)};
    return launch_tiles(t.tables == 2 ? march_tf2d_bwd_kernel<VT, 2> : (t.tables == 1 ? march_tf2d_bwd_kernel<VT, 1> : march_tf2d_bwd_kernel<VT, 0>),
                        a, t.lds, stream, P);
}

int launch_march_tf2d_fwd(const MarchArgs &a, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? tf2d_fwd_dispatch<__half>(a, stream) : tf2d_fwd_dispatch<float>(a, stream);
}

int launch_march_tf2d_bwd(const MarchArgs &a, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? tf2d_bwd_dispatch<__half>(a, stream) : tf2d_bwd_dispatch<float>(a, stream);
}

}  // namespace dr
