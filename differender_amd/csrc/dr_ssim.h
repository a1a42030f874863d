// dr_ssim.h -- pieces shared by the windowed-SSIM loss kernels: image_loss.hip and msssim.hip (D10).
// The tile geometry, the f32 Gaussian window, the per-tile shift of the moments, the f64 workgroup sum and the LDS sizing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

namespace dr {
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

__device__ __forceinline__ double block_sum(double v, double *red) {  // red: NT/64 doubles; result valid in thread 0
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
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
template <typename F>
int pick_ty(F lds_floats, int kh, int kw, size_t *bytes) {
    for (size_t cap : {LDS_DEFAULT, LDS_MAX})
        for (int TY = 16; TY >= 1; TY >>= 1)
            if ((*bytes = lds_floats(TY, kh, kw) * sizeof(float)) + STATIC_LDS <= cap) return TY;
    return 0;
}

}  // namespace ssim
}  // namespace dr
