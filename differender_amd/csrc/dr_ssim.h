// dr_ssim.h -- the windowed-SSIM tile of the loss kernels: image_loss.hip and msssim.hip (D10) are its two
// callers. The tile geometry, the f32 Gaussian window, the per-tile shift of the moments, every pass of the forward and of the
// backward over one 64 x TY tile, the f64 workgroup sums, the finalize tail, the LDS sizing and the launch. A kernel keeps what
// is its own: which plane and level a workgroup works on, dL/dS, where the gradient goes, which stats slot the atomics hit.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include <algorithm>

#include "dr_kernels.h"
#include "../../include/differender_hip.h"

namespace dr {

hipError_t allow_lds_impl(const void *kernel, size_t bytes);  // capi.hip

namespace ssim {

constexpr int TX = 64;          // tile width: one wave row along W
constexpr int NT = 256;         // threads per workgroup
constexpr int KMAX = 31;        // largest window (validated by the C entries)
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;
constexpr size_t STATIC_LDS = 256;   // the window and the reduction slots beside the dynamic carve

// _gauss_window in f32 into w[0..k), and w[KMAX] = 1: a side shorter than the window is not filtered (the one-tap window {1})
__device__ __forceinline__ void build_window(int k, float sigma_den, float *w) {
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int i = 0; i < k; ++i) {
            const float t = (float)(i - k / 2);
            w[i] = expf(-(t * t) / sigma_den);
            s += w[i];
        }
        for (int i = 0; i < k; ++i) w[i] = w[i] / s;
        w[KMAX] = 1.0f;
    }
    __syncthreads();
}

// Every workgroup filters its tile shifted by one constant, (x - c, y - c): sigma^2 = E[x^2] - E[x]^2 cancels in f32 when the
// mean is large against the spread (a flat region gives 1e-4 of noise in the loss unshifted). c = clamp(0, lo, hi), [lo, hi]
// the range of the finite in-image pixels of both staged tiles (0 when there are none), so |v - c| <= |v| for every pixel:
// the shifted moments are never larger than torch's unshifted ones, and a tile away from 0 is taken from its nearest level.
// (One pixel of the tile would not do: on a bright pixel every dark window of the tile cancels, and a tile mean puts the
// flat black half of a tile off 0.) The means are put back as mu = G(x - c) + c sum(w); the shift leaves the maths unchanged.
// Min and max are exact and order-free, so c, and with it the gradient, is the same run to run.
__device__ __forceinline__ void range_add(float v, float &lo, float &hi) {   // lo = +inf, hi = -inf to start
    if (isfinite(v)) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
}
__device__ __forceinline__ float block_shift(float lo, float hi, float *red) {   // red: 2 NT/64 floats; c in every thread
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[NT / 64 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    return lo <= hi ? fminf(fmaxf(0.0f, lo), hi) : 0.0f;
}
// the staged tile (n floats) shifted in place, between block_shift's barrier and the caller's before the first pass over it.
// The zeros beyond the image become -c: they feed only outputs that do not exist.
__device__ __forceinline__ void shift_tile(float *t, int n, float c) {
    for (int i = threadIdx.x; i < n; i += NT) t[i] -= c;
}
__device__ __forceinline__ float window_mass(const float *wv, int kh, const float *wh, int kw) {   // G applied to a constant 1
    float sv = 0.0f, s = 0.0f;
    for (int j = 0; j < kh; ++j) sv += wv[j];
    for (int j = 0; j < kw; ++j) s += wh[j] * sv;
    return s;
}

// one plane of an image pair: x, y at the plane's first pixel
struct Plane {
    const float *x, *y;
    int64_t s2, s3;
    int H, W, Ho, Wo;           // the plane and its map: Ho = H - kh + 1, Wo = W - kw + 1
};
// the separable window: wv[kh] along H, wh[kw] along W (MS-SSIM: the same k taps twice); C1, C2 of the SSIM formula
struct Window {
    const float *wv, *wh;
    int kh, kw;
    float C1, C2;
};
// D9's window: a side shorter than the window is not filtered
__device__ __forceinline__ Window make_window(const float *w, int kh, int kw, float C1, float C2) {
    return {kh == 1 ? w + KMAX : w, kw == 1 ? w + KMAX : w, kh, kw, C1, C2};
}

// Rows gy0.., columns gx0.. of the plane into lds[2][IH][IW] (X, then Y; zeros beyond the image feed only output positions that
// do not exist), shifted by the tile's shift, which is returned. own(r, c, xv, yv) sees every in-image pixel once.
template <typename F>
__device__ __forceinline__ float stage_tile(const Plane &p, int gy0, int gx0, int IH, int IW, float *lds, float *rng, F own) {
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW, gy = gy0 + r, gx = gx0 + c;
        float xv = 0.0f, yv = 0.0f;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
            const int64_t o = gy * p.s2 + gx * p.s3;
            xv = p.x[o];
            yv = p.y[o];
            own(r, c, xv, yv);
            range_add(xv, lo, hi);
            range_add(yv, lo, hi);
        }
        lds[i] = xv;
        lds[IH * IW + i] = yv;
    }
    const float sh = block_shift(lo, hi, rng);
    shift_tile(lds, 2 * IH * IW, sh);
    __syncthreads();
    return sh;
}

// vertical pass (along H) of the five moments (x, y, xx, yy, xy) on every column of the staged tile: V[5][rows][IW]
__device__ __forceinline__ void moments_v(const float *in, int IH, int IW, int rows, const float *wv, int kh, float *V) {
    const float *in_x = in, *in_y = in + IH * IW;
    const int nV = rows * IW;
    for (int i = threadIdx.x; i < nV; i += NT) {
        const int b = i / IW, c = i - b * IW;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f;
        for (int j = 0; j < kh; ++j) {
            const float w = wv[j], xv = in_x[(b + j) * IW + c], yv = in_y[(b + j) * IW + c];
            a0 = fmaf(w, xv, a0); a1 = fmaf(w, yv, a1); a2 = fmaf(w, xv * xv, a2); a3 = fmaf(w, yv * yv, a3); a4 = fmaf(w, xv * yv, a4);
        }
        V[i] = a0; V[nV + i] = a1; V[2 * nV + i] = a2; V[3 * nV + i] = a3; V[4 * nV + i] = a4;
    }
    __syncthreads();
}
// horizontal pass (along W) at one output position: o = its row * IW + its column in V
__device__ __forceinline__ void moments_h(const float *V, int nV, int o, const float *wh, int kw, float *m) {
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = 0.0f;
    for (int j = 0; j < kw; ++j) {
        const float w = wh[j];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = fmaf(w, V[q * nV + o + j], m[q]);
    }
}
// The two SSIM factors at one position, A = a1 / a2 from the means and B = b1 / b2 (the CS map) from the shifted moments:
// m[0], m[1] = mu1 - shm, mu2 - shm, shm = shift * window_mass. A only where `full` (workgroup-uniform).
struct Factors {
    float mu1, mu2, a2, A, b2, B;
};
__device__ __forceinline__ Factors factors(const float *m, float shm, const Window &w, bool full) {
    Factors f = {0.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f};
    const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
    f.b2 = s1 + s2 + w.C2;
    f.B = (2.0f * s12 + w.C2) / f.b2;
    if (full) {
        f.mu1 = m[0] + shm;
        f.mu2 = m[1] + shm;
        f.a2 = f.mu1 * f.mu1 + f.mu2 * f.mu2 + w.C1;
        f.A = (2.0f * (f.mu1 * f.mu2) + w.C1) / f.a2;
    }
    return f;
}

// Forward of the 64 x TY tile at (y0, x0) of the plane's map: this thread's share of the sum of the SSIM (`full`) or CS map,
// and, where want_se, of the squared error of the pixels the tile owns (its own 64 x TY block, and up to the image edge for the
// last tile of a row / column) added to se. lds: fwd_lds_floats(TY, kh, kw).
__device__ __forceinline__ float tile_map_sum(const Plane &p, int y0, int x0, int TY, const Window &w, bool full, bool want_se,
                                              float *lds, float *rng, float &se) {
    const int IH = TY + w.kh - 1, IW = TX + w.kw - 1, nV = TY * IW;
    float *V = lds + 2 * IH * IW;
    const bool last_x = x0 + TX >= p.Wo, last_y = y0 + TY >= p.Ho;
    const float sh = stage_tile(p, y0, x0, IH, IW, lds, rng, [&](int r, int c, float xv, float yv) {
        if (want_se && (r < TY || last_y) && (c < TX || last_x)) {
            const float d = xv - yv;
            se += d * d;
        }
    });
    moments_v(lds, IH, IW, TY, w.wv, w.kh, V);
    const float shm = sh * window_mass(w.wv, w.kh, w.wh, w.kw);
    float ss = 0.0f;
    for (int i = threadIdx.x; i < TY * TX; i += NT) {
        const int b = i / TX, a = i % TX;
        if (y0 + b >= p.Ho || x0 + a >= p.Wo) continue;
        float m[5];
        moments_h(V, nV, b * IW + a, w.wh, w.kw, m);
        const Factors f = factors(m, shm, w, full);
        ss += full ? f.A * f.B : f.B;
    }
    return ss;
}

// Backward of the 64 x TY tile at (y0, x0) of the plane, up to the transposed horizontal pass. With g = dL/d(map pixel) the four
// adjoint maps (D_mu1, D_mu2, D_m3 = D_m4, D_m5) on the output positions whose windows reach the tile (a halo of k-1, so the
// moments are recomputed over a halo of 2(k-1); zero where no output exists):
//   SSIM (full): dS/dm3 = dS/dm4 = -AB/b2,  dS/dm5 = 2A/b2,  dS/dmu1 = 2B(mu2 - mu1 A)/a2 + 2A(mu1 B - mu2)/b2
//   CS:          dB/dm3 = dB/dm4 = -B/b2,   dB/dm5 = 2/b2,   dB/dmu1 = 2(mu1 B - mu2)/b2            (mu2 by symmetry)
// then G^T along W onto the tile's 64 columns: returns T[4][TY + kh - 1][64] (in lds), and the tile's shift in sh.
// lds: bwd_lds_floats(TY, kh, kw); region 1 holds the input, then the maps; region 2 the vertical moments, then T.
__device__ __forceinline__ const float *tile_adjoint_h(const Plane &p, int y0, int x0, int TY, const Window &w, bool full, float g,
                                                       float *lds, float *rng, float &sh) {
    const int kh = w.kh, kw = w.kw, IH = TY + 2 * (kh - 1), IW = TX + 2 * (kw - 1), QH = TY + kh - 1, QW = TX + kw - 1;
    const int nV = QH * IW, nD = QH * QW, nT = QH * TX;
    float *Dm = lds, *V = lds + max(2 * IH * IW, 4 * nD), *T = V;
    sh = stage_tile(p, y0 - (kh - 1), x0 - (kw - 1), IH, IW, lds, rng, [](int, int, float, float) {});
    moments_v(lds, IH, IW, QH, w.wv, kh, V);
    const float shm = sh * window_mass(w.wv, kh, w.wh, kw);
    for (int i = threadIdx.x; i < nD; i += NT) {
        const int b = i / QW, a = i - b * QW, qy = y0 - (kh - 1) + b, qx = x0 - (kw - 1) + a;
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
        if (qy >= 0 && qy < p.Ho && qx >= 0 && qx < p.Wo) {
            float m[5];
            moments_h(V, nV, b * IW + a, w.wh, kw, m);
            const Factors f = factors(m, shm, w, full);
            const float gb = g / f.b2;
            if (full) {
                const float ga = g / f.a2;
                d0 = 2.0f * f.B * (f.mu2 - f.mu1 * f.A) * ga + 2.0f * f.A * (m[0] * f.B - m[1]) * gb;
                d1 = 2.0f * f.B * (f.mu1 - f.mu2 * f.A) * ga + 2.0f * f.A * (m[1] * f.B - m[0]) * gb;
                d2 = -(f.A * f.B) * gb;
                d3 = 2.0f * f.A * gb;
            } else {
                d0 = 2.0f * (m[0] * f.B - m[1]) * gb;
                d1 = 2.0f * (m[1] * f.B - m[0]) * gb;
                d2 = -f.B * gb;
                d3 = 2.0f * gb;
            }
        }
        Dm[i] = d0; Dm[nD + i] = d1; Dm[2 * nD + i] = d2; Dm[3 * nD + i] = d3;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nT; i += NT) {
        const int b = i / TX, x = i % TX;
        float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < kw; ++j) {
            const float wj = w.wh[j];
            const int o = b * QW + x + kw - 1 - j;
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] += wj * Dm[q * nD + o];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) T[q * nT + i] = t[q];
    }
    __syncthreads();
    return T;
}
// G^T along H at pixel (y, x) of the tile and the chain through x, x^2 and xy (xs, ys: the pixel minus the tile's shift): the
// SSIM part of (dX, dY). T null (a plane without SSIM gradient) is the chain through zero maps: 0 at a finite pixel, and
// 2 xs 0 = NaN at an infinite one.
__device__ __forceinline__ void adjoint_v(const float *T, int TY, int y, int x, const Window &w, float xs, float ys, float &rx,
                                          float &ry) {
    const int nT = (TY + w.kh - 1) * TX;
    float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (T) {
        for (int j = 0; j < w.kh; ++j) {
            const float wj = w.wv[j];
            const int t = (y + w.kh - 1 - j) * TX + x;
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] += wj * T[q * nT + t];
        }
    }
    rx = r[0] + 2.0f * xs * r[2] + ys * r[3];
    ry = r[1] + 2.0f * ys * r[2] + xs * r[3];
}

__device__ __forceinline__ double block_sum(double v, double *red) {  // red: NT/64 doubles; result valid in thread 0
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// The end of a finalize kernel (one workgroup): the deterministic tree over every thread's sum of its planes' values (red: NT
// doubles), then with the sum of squared errors in tail[2]: d = 1 - mean, tail = (nan_to_num(d) + mse, d, mse)
__device__ __forceinline__ void finalize_tail(double acc, double *red, int planes, double inv_numel, double *tail) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double d = 1.0 - red[0] / planes, mse = tail[2] * inv_numel;
        // nan_to_num of the f32 d: NaN -> 0, +-inf -> +-FLT_MAX
        tail[0] = (isnan(d) ? 0.0 : (isinf(d) ? copysign((double)FLT_MAX, d) : d)) + mse;
        tail[1] = d;
        tail[2] = mse;
    }
}

// dynamic LDS of the forward (input with its halo, vertical moments) and of the backward (input with a 2(k-1) halo or the
// adjoint maps, then the vertical moments or the transposed horizontal pass), in floats
inline size_t fwd_lds_floats(int TY, int kh, int kw) {
    const int IH = TY + kh - 1, IW = TX + kw - 1;
    return (size_t)2 * IH * IW + (size_t)5 * TY * IW;
}
inline size_t bwd_lds_floats(int TY, int kh, int kw) {
    const int IH = TY + 2 * (kh - 1), IW = TX + 2 * (kw - 1), QH = TY + kh - 1, QW = TX + kw - 1;
    return std::max((size_t)2 * IH * IW, (size_t)4 * QH * QW) + std::max((size_t)5 * QH * IW, (size_t)4 * QH * TX);
}

// The tallest tile (16 rows at most) whose LDS fits the default 64 KB; a wide window falls back to the opt-in above it
inline int pick_ty(bool bwd, int kh, int kw, size_t *bytes) {
    for (size_t cap : {LDS_DEFAULT, LDS_MAX})
        for (int TY = 16; TY >= 1; TY >>= 1)
            if ((*bytes = (bwd ? bwd_lds_floats : fwd_lds_floats)(TY, kh, kw) * sizeof(float)) + STATIC_LDS <= cap) return TY;
    return 0;
}
// tiles of one plane: the forward tiles the output plane, the backward the input
inline void tile_counts(int H, int W, int Ho, int Wo, int TY, bool bwd, int *tiles_x, int *tiles) {
    *tiles_x = ((bwd ? W : Wo) + TX - 1) / TX;
    *tiles = *tiles_x * (((bwd ? H : Ho) + TY - 1) / TY);
}
// what both kernels' parameter blocks (LossParams, MSParams) take unchanged from the C entry's arguments
template <typename P>
void fill_common(P &p, const ImageArgs &a) {
    p.C = a.C;
    p.planes = a.N * a.C;
    p.k = a.win_size;
    p.sigma_den = (float)(2.0 * a.win_sigma * a.win_sigma);   // as _gauss_window divides by it
    p.C1 = (float)((a.K1 * a.data_range) * (a.K1 * a.data_range));
    p.C2 = (float)((a.K2 * a.data_range) * (a.K2 * a.data_range));
    p.inv_numel = 1.0 / ((double)p.planes * a.H * a.W);
    p.stats = a.stats;
    p.up = a.upstream;
}

// a tile kernel's launch: the opt-in above the default LDS (once per kernel, device and size), then the launch
template <typename K, typename... Args>
int launch_lds(K kernel, unsigned blocks, size_t lds, hipStream_t stream, Args... args) {
    if (lds > LDS_DEFAULT && allow_lds_impl(reinterpret_cast<const void *>(kernel), lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(NT), lds, stream, args...);
    return (int)hipGetLastError();
}

}  // namespace ssim
}  // namespace dr
