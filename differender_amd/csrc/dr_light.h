// dr_light.h -- the lit march's device helpers: Phong shading with a free light and material, its adjoint with
// the ten lighting gradients, the coloured composite and the workgroup reduction. They stand beside shade_from_grad,
// sample_adjoint, Composite and pose_reduce (dr_device.h, dr_camera.h), which keep the reference's literals (VR.py:91-95,
// 281-299) and are not touched: at the reference's values every function here performs their operations in their order.
#pragma once
#include "dr_device.h"

namespace dr {

// light[view][10]: position (world), colour, ambient, diffuse and specular weights, shininess
struct Light { f3 p, lc; float ka, kd, ks, sh; };
__device__ __forceinline__ Light load_light(const float *l) {
    Light t;
    t.p = make_f3(l[0], l[1], l[2]); t.lc = make_f3(l[3], l[4], l[5]);
    t.ka = l[6]; t.kd = l[7]; t.ks = l[8]; t.sh = l[9];
    return t;
}

// VR.py:191-203 normal, :287-299 Phong with the light's parameters: shade_from_grad<false> with 0.8 -> kd, 0.3 -> ks, 0.4 -> ka
// and r.v^32 -> r.v^sh. sh32 (uniform): the five squarings of pow32, else D6's specified power (pow_spec(0, .) = 0).
// Returns P = r.v^sh, which the adjoint of ks and sh needs.
__device__ __forceinline__ float shade_lit_from_grad(float dx, float dy, float dz, const Light &lt, bool sh32, f3 vd, bool clampL,
                                                     Sample &sm) {
    sm.grad = make_f3(dx, dy, dz);
    const float gn2 = dot3(sm.grad, sm.grad);
    const f3 lv = make_f3(sm.px - lt.p.x, sm.py - lt.p.y, sm.pz - lt.p.z);
    sm.gnorm = sqrtf(gn2);
    sm.flat = !(sm.gnorm > 0.0f);
    sm.ginv = 1.0f / (sm.gnorm + 0.0f);
    sm.ld = normalized3(lv);
    if (sm.flat) {
        // D1: ndl = rdv = 0
        sm.nrm = make_f3(0.f, 0.f, 0.f);
        sm.m = 0.f; sm.ndl = 0.f; sm.rf = sm.ld; sm.q = 0.f; sm.rdv = 0.f;
    } else {
        sm.nrm = make_f3(sm.ginv * dx, sm.ginv * dy, sm.ginv * dz);
        sm.m = dot3(sm.nrm, sm.ld);
        sm.ndl = fmaxf(sm.m, 0.0f);
        float two_m = 2.0f * sm.m;
        sm.rf = make_f3(fmaf(-two_m, sm.nrm.x, sm.ld.x), fmaf(-two_m, sm.nrm.y, sm.ld.y), fmaf(-two_m, sm.nrm.z, sm.ld.z));
        sm.q = -dot3(sm.rf, vd);
        sm.rdv = fmaxf(sm.q, 0.0f);
    }
    float P;
    if (sh32) P = pow32(sm.rdv);
    else P = pow_spec(sm.rdv, lt.sh);
    sm.spec = lt.ks * P;
    sm.Lraw = fmaf(lt.kd, sm.ndl, sm.spec) + lt.ka;
    sm.L = clampL ? fminf(1.0f, sm.Lraw) : sm.Lraw;
    return P;
}

template <typename VT>
__device__ __forceinline__ float shade_lit(const VolView<VT> &v, const Light &lt, bool sh32, f3 vd, bool clampL, Sample &sm) {
    const float delta = 1e-3f;
    float dx = tri_sample(v, sm.px + delta, sm.py, sm.pz) - tri_sample(v, sm.px - delta, sm.py, sm.pz);
    float dy = tri_sample(v, sm.px, sm.py + delta, sm.pz) - tri_sample(v, sm.px, sm.py - delta, sm.pz);
    float dz = tri_sample(v, sm.px, sm.py, sm.pz + delta) - tri_sample(v, sm.px, sm.py, sm.pz - delta);
    return shade_lit_from_grad(dx, dy, dz, lt, sh32, vd, clampL, sm);
}

// Composite with the light's colour on the three colour channels: C_k = fma(T, (L c_k op) lc_k, C_k)
struct CompositeLit : Composite {
    __device__ __forceinline__ float add_lit(const Sample &sm, f3 lc) {
        const float T = 1.0f - A;
        C0 = fmaf(T, (sm.L * sm.r * sm.op) * lc.x, C0);
        C1 = fmaf(T, (sm.L * sm.g * sm.op) * lc.y, C1);
        C2 = fmaf(T, (sm.L * sm.b * sm.op) * lc.z, C2);
        A = fmaf(T, sm.op, A);
        return T;
    }
};

// a ray's ten f32 sums, in the order of light[view][10]
struct LightGrad { f3 p, lc; float ka, kd, ks, sh; };
__device__ __forceinline__ LightGrad light_zero() {
    LightGrad g; g.p = g.lc = make_f3(0.f, 0.f, 0.f); g.ka = g.kd = g.ks = g.sh = 0.f; return g;
}
// D5 for the ten components: a NaN ray contributes nothing, infinities are clamped
__device__ __forceinline__ LightGrad light_finite(LightGrad g) {
    g.p = make_f3(finite_or_zero(g.p.x), finite_or_zero(g.p.y), finite_or_zero(g.p.z));
    g.lc = make_f3(finite_or_zero(g.lc.x), finite_or_zero(g.lc.y), finite_or_zero(g.lc.z));
    g.ka = finite_or_zero(g.ka); g.kd = finite_or_zero(g.kd); g.ks = finite_or_zero(g.ks); g.sh = finite_or_zero(g.sh);
    return g;
}

// sample_adjoint with the light's parameters. go' = (go.rgb * lc, go.a) stands for go in rgbdot, qs and (r,g,b)_bar; `suffix`
// is the caller's, from the plain go (the composite already holds lc). P = r.v^sh of shade_lit_from_grad.
// LIGHT: this sample's share of the ten lighting gradients is added to lg --
//   ka += Lraw_bar, kd += ndl Lraw_bar, ks += P Lraw_bar, sh += ks P log(r.v) Lraw_bar where r.v > 0,
//   lc_k += go_k (T L c_k op): the un-coloured term, exact also at lc_k = 0,
//   p -= H, H = (ld_bar - (ld.ld_bar) ld) / |pos - p|, ld_bar = m_bar n + rf_bar (camera_grad.hip's H_s; 0 when flat).
template <bool LIGHT>
__device__ __forceinline__ void sample_adjoint_lit(const Sample &sm, float P, const Light &lt, bool sh32, f3 vd, float T,
                                                   float suffix, bool last, float4 go, float inv_sr, SampleAdj &ad, LightGrad &lg) {
    const float gx = go.x * lt.lc.x, gy = go.y * lt.lc.y, gz = go.z * lt.lc.z;
    const float rgbdot = gx * sm.r + gy * sm.g + gz * sm.b;
    const float qs = sm.L * rgbdot + go.w;
    const float sfx = suffix / (1.0f - sm.op);
    const float op_bar = T * qs - (last ? 0.0f : sfx);
    const float Lop = sm.L * sm.op * T;
    ad.Lop = Lop;
    ad.r_bar = Lop * gx; ad.g_bar = Lop * gy; ad.b_bar = Lop * gz;
    const float L_bar = sm.op * T * rgbdot;
    const float Lraw_bar = (1.0f < sm.Lraw) ? 0.0f : L_bar;
    const float base = 1.0f - sm.a;
    ad.a_bar = op_bar * ((inv_sr == 1.0f) ? 1.0f : inv_sr * powf(base, inv_sr - 1.0f));
    if (LIGHT) {
        lg.ka += Lraw_bar;
        lg.kd = fmaf(sm.ndl, Lraw_bar, lg.kd);
        lg.ks = fmaf(P, Lraw_bar, lg.ks);
        if (sm.rdv > 0.0f) lg.sh = fmaf(lt.ks * P * logf(sm.rdv), Lraw_bar, lg.sh);
        lg.lc.x = fmaf(go.x, Lop * sm.r, lg.lc.x);
        lg.lc.y = fmaf(go.y, Lop * sm.g, lg.lc.y);
        lg.lc.z = fmaf(go.z, Lop * sm.b, lg.lc.z);
    }
    // (one assignment of ad.g* below, not an early return for flat samples: the early return left them in scratch)
    float agx = 0.0f, agy = 0.0f, agz = 0.0f;   // D1: a flat sample sends nothing through its normal
    if (!sm.flat) {
        const float ndl_bar = lt.kd * Lraw_bar;
        // d r.v^sh / d r.v = sh r.v^(sh-1): pow31 at sh = 32, else P / r.v (only read where 0 < q, i.e. r.v = q > 0)
        float dP;
        if (sh32) dP = pow31(sm.rdv);
        else dP = P / sm.rdv;
        const float rdv_bar = lt.ks * lt.sh * dP * Lraw_bar;
        const float q_bar = (0.0f < sm.q) ? rdv_bar : 0.0f;
        const f3 rf_bar = make_f3(-vd.x * q_bar, -vd.y * q_bar, -vd.z * q_bar);
        const float m_bar = ((0.0f < sm.m) ? ndl_bar : 0.0f) - 2.0f * dot3(sm.nrm, rf_bar);
        const float m2 = -2.0f * sm.m;
        const f3 n_bar = make_f3(m2 * rf_bar.x + m_bar * sm.ld.x, m2 * rf_bar.y + m_bar * sm.ld.y,
                                 m2 * rf_bar.z + m_bar * sm.ld.z);
        const float nn = dot3(sm.nrm, n_bar);
        const float inv = sm.ginv;
        agx = inv * (n_bar.x - sm.nrm.x * nn);
        agy = inv * (n_bar.y - sm.nrm.y * nn);
        agz = inv * (n_bar.z - sm.nrm.z * nn);
        if (LIGHT) {
            const f3 ld_bar = make_f3(fmaf(m_bar, sm.nrm.x, rf_bar.x), fmaf(m_bar, sm.nrm.y, rf_bar.y), fmaf(m_bar, sm.nrm.z, rf_bar.z));
            const f3 lv = make_f3(sm.px - lt.p.x, sm.py - lt.p.y, sm.pz - lt.p.z);
            const float il = 1.0f / sqrtf(dot3(lv, lv));
            const float along = dot3(sm.ld, ld_bar);
            lg.p.x -= il * fmaf(-along, sm.ld.x, ld_bar.x);
            lg.p.y -= il * fmaf(-along, sm.ld.y, ld_bar.y);
            lg.p.z -= il * fmaf(-along, sm.ld.z, ld_bar.z);
        }
    }
    ad.gx = agx; ad.gy = agy; ad.gz = agz;
}

// The end of the lit backward (256 lanes, every lane arrives): the optional per-ray store, then the workgroup's sum in double
// -- each wave's by butterfly, the four waves' through red[4][10] in LDS -- and ONE f64 atomic per component into
// d_light[view][10]: pose_reduce's result from 320 B of LDS, which the caller carves out of its dynamic region. p: the ray's
// index, read only where in_img.
constexpr size_t LIGHT_RED_BYTES = 4 * 10 * sizeof(double);
__device__ __forceinline__ void light_reduce(const LightGrad &g, bool in_img, size_t p, int view, float *d_light_ray,
                                             double *d_light, double *red) {
    const float c[10] = {g.p.x, g.p.y, g.p.z, g.lc.x, g.lc.y, g.lc.z, g.ka, g.kd, g.ks, g.sh};
    if (in_img && d_light_ray) {
#pragma unroll
        for (int k = 0; k < 10; ++k) d_light_ray[10 * p + k] = c[k];
    }
    if (!d_light) return;   // (uniform)
    __syncthreads();        // red overlays LDS the march has read
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        double v = (double)c[k];
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
        if (lane == 0) red[10 * wave + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const double v = (red[threadIdx.x] + red[10 + threadIdx.x]) + (red[20 + threadIdx.x] + red[30 + threadIdx.x]);
        if (v != 0.0) atomicAdd(d_light + 10 * view + threadIdx.x, v);
    }
}

}  // namespace dr
