// image_loss.hip -- the demo's image loss nan_to_num(1 - ssim(res, gt, data_range, nonnegative_ssim)) + mse(res, gt)
// (examples/test_opt_tf.py:70-72, "OPT.py") and its gradient, fused, gfx950. The definition is the torch
// restatement differender_amd.utils.losses.ssim2d / dssim_mse_loss: Gaussian window built in f32 and normalised by its f32
// sum, separable VALID filtering along H then W, a pass skipped when its side is shorter than the window (a skipped pass is
// the one-tap window {1} here, which is exact), the per-plane mean of the SSIM map, relu on it when nonnegative, the mean over
// planes, and the mse over the full images.
//
// Forward (one workgroup per 64 x TY tile of the output plane): stage X and Y with their (k-1) halo in LDS, take the five
// windowed moments (x, y, xx, yy, xy) with a vertical then a horizontal pass, form the SSIM map and the squared error of the
// pixels the tile owns. Sums: f32 per lane, f64 per workgroup, ONE f64 atomic per workgroup into the plane's slot of `stats`
// and one into the mse slot. A one-workgroup finalize turns the sums into S_nc, ssim, dssim, mse and loss.
//
// Backward (one workgroup per 64 x TY tile of the input plane): with A = a1/a2, B = b1/b2 the two SSIM factors,
//   dS/dm3 = dS/dm4 = -AB/b2,  dS/dm5 = 2A/b2,  dS/dmu1 = 2B(mu2 - mu1 A)/a2 + 2A(mu1 B - mu2)/b2  (mu2 by symmetry),
// scaled by dL/dS_nc / (Ho Wo), gives four adjoint maps (D_m3 = D_m4) on the output positions whose windows reach the tile
// (a halo of k-1, so the moments are recomputed over a halo of 2(k-1)); the transposed filter (W then H) brings them back:
//   dX = G^T D_mu1 + 2X G^T D_m3 + Y G^T D_m5 + w_mse 2(X-Y)/numel,  dY the mirror image with the mse term negated.
// dL/dS_nc depends only on relu's mask, the finiteness of dssim and the upstream weights: the gradient has no reduction in it
// and is bitwise the same run to run.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include <algorithm>

#include "dr_kernels.h"
#include "dr_ssim.h"
#include "../../include/differender_hip.h"

namespace dr {

hipError_t allow_lds_impl(const void *kernel, size_t bytes);  // capi.hip

namespace {

using namespace ssim;

struct LossParams {
    const float *x, *y;
    int64_t s0, s1, s2, s3;
    int C, H, W, Ho, Wo, kh, kw, k, TY, tiles_x, tiles, planes;
    float sigma_den;            // 2 sigma^2, as _gauss_window divides by it
    float C1, C2;
    int nonneg;
    double inv_px, inv_numel;   // 1 / (Ho Wo), 1 / (N C H W)
    double *stats;              // forward: sums; backward: read only
    const float *up;            // backward: (d loss, d dssim, d mse) on the device, null = (1, 0, 0)
    float *gx, *gy;
};

__global__ __launch_bounds__(NT) void dssim_mse_fwd_kernel(LossParams P) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ double red[2][NT / 64];
    __shared__ float rng[2 * NT / 64];
    const int tile = blockIdx.x % P.tiles, plane = blockIdx.x / P.tiles;
    const int x0 = (tile % P.tiles_x) * TX, y0 = (tile / P.tiles_x) * P.TY;
    const int TY = P.TY, kh = P.kh, kw = P.kw, IH = TY + kh - 1, IW = TX + kw - 1;
    const int64_t base = (int64_t)(plane / P.C) * P.s0 + (int64_t)(plane % P.C) * P.s1;
    const float *xp = P.x + base, *yp = P.y + base;
    float *in_x = lds, *in_y = lds + IH * IW, *V = lds + 2 * IH * IW;   // V[5][TY][IW]
    build_window(P.k, P.sigma_den, wg);
    const float *wv = P.kh == 1 ? wg + KMAX : wg, *wh = P.kw == 1 ? wg + KMAX : wg;

    // the tile's input with its halo (zeros beyond the image feed only output positions that do not exist); the squared error
    // of the pixels this tile owns: its own 64 x TY block, and up to the image edge for the last tile of a row / column
    const bool last_x = x0 + TX >= P.Wo, last_y = y0 + TY >= P.Ho;
    const float sw = window_mass(wv, kh, wh, kw);
    float se = 0.0f, lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW, gy = y0 + r, gx = x0 + c;
        float xv = 0.0f, yv = 0.0f;
        if (gy < P.H && gx < P.W) {
            const int64_t o = gy * P.s2 + gx * P.s3;
            xv = xp[o];
            yv = yp[o];
            if ((r < TY || last_y) && (c < TX || last_x)) {
                const float d = xv - yv;
                se += d * d;
            }
            range_add(xv, lo, hi);
            range_add(yv, lo, hi);
        }
        in_x[i] = xv;
        in_y[i] = yv;
    }
    const float sh = block_shift(lo, hi, rng);   // the tile's shift
    shift_tile(lds, 2 * IH * IW, sh);
    __syncthreads();
    // vertical pass (along H) of the five moments, on every column of the tile's input
    const int nV = TY * IW;
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
    // horizontal pass (along W) and the SSIM map
    float ss = 0.0f;
    for (int i = threadIdx.x; i < TY * TX; i += NT) {
        const int b = i / TX, a = i % TX;
        if (y0 + b >= P.Ho || x0 + a >= P.Wo) continue;
        float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < kw; ++j) {
            const float w = wh[j];
            const int o = b * IW + a + j;
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fmaf(w, V[q * nV + o], m[q]);
        }
        const float mu1 = m[0] + sh * sw, mu2 = m[1] + sh * sw;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
        const float cs = (2.0f * s12 + P.C2) / (s1 + s2 + P.C2);
        ss += ((2.0f * mu12 + P.C1) / (mu1_sq + mu2_sq + P.C1)) * cs;
    }
    const double ssum = block_sum((double)ss, red[0]);
    const double esum = block_sum((double)se, red[1]);
    if (threadIdx.x == 0) {
        atomicAdd(&P.stats[plane], ssum);
        atomicAdd(&P.stats[P.planes + 2], esum);
    }
}

// sums -> S_nc (relu'd when nonnegative), then loss, dssim, mse; deterministic tree over the planes
__global__ __launch_bounds__(NT) void dssim_mse_finalize_kernel(LossParams P) {
    __shared__ double red[NT];
    double acc = 0.0;
    for (int p = threadIdx.x; p < P.planes; p += NT) {
        double S = P.stats[p] * P.inv_px;
        if (P.nonneg && S <= 0.0) S = 0.0;   // relu (NaN passes through, as torch.relu's)
        P.stats[p] = S;
        acc += S;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double dssim = 1.0 - red[0] / P.planes;
        const double mse = P.stats[P.planes + 2] * P.inv_numel;
        // nan_to_num of the f32 dssim: NaN -> 0, +-inf -> +-FLT_MAX
        const double d = isnan(dssim) ? 0.0 : (isinf(dssim) ? copysign((double)FLT_MAX, dssim) : dssim);
        P.stats[P.planes] = d + mse;
        P.stats[P.planes + 1] = dssim;
        P.stats[P.planes + 2] = mse;
    }
}

__global__ __launch_bounds__(NT) void dssim_mse_bwd_kernel(LossParams P) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ float rng[2 * NT / 64];
    const int tile = blockIdx.x % P.tiles, plane = blockIdx.x / P.tiles;
    const int x0 = (tile % P.tiles_x) * TX, y0 = (tile / P.tiles_x) * P.TY;
    const int TY = P.TY, kh = P.kh, kw = P.kw;
    const int64_t base = (int64_t)(plane / P.C) * P.s0 + (int64_t)(plane % P.C) * P.s1;
    const float *xp = P.x + base, *yp = P.y + base;

    // dL/dS_nc: relu passes where S > 0, nan_to_num where dssim is finite; upstream (d loss, d dssim, d mse)
    double u0 = 1.0, u1 = 0.0, u2 = 0.0;
    if (P.up) { u0 = P.up[0]; u1 = P.up[1]; u2 = P.up[2]; }
    const bool pass = !P.nonneg || P.stats[plane] > 0.0;
    const bool finite = isfinite(P.stats[P.planes + 1]);
    const float g = pass ? (float)(-(u0 * (finite ? 1.0 : 0.0) + u1) / P.planes * P.inv_px) : 0.0f;
    const float wm = (float)(2.0 * (u0 + u2) * P.inv_numel);

    const float *wv = P.kh == 1 ? wg + KMAX : wg, *wh = P.kw == 1 ? wg + KMAX : wg;
    const float *Tt = nullptr;
    float sh = 0.0f;
    // (workgroup-uniform) no SSIM gradient for this plane: the mse term alone, and no 0 * NaN from the moments
    if (g != 0.0f) {
        const int IH = TY + 2 * (kh - 1), IW = TX + 2 * (kw - 1), QH = TY + kh - 1, QW = TX + kw - 1;
        const int r1 = max(2 * IH * IW, 4 * QH * QW);
        float *in_x = lds, *in_y = lds + IH * IW, *Dm = lds;   // region 1: the input, then the adjoint maps Dm[4][QH][QW]
        float *V = lds + r1;                                     // region 2: the vertical moments V[5][QH][IW], then Tt[4][QH][TX]
        build_window(P.k, P.sigma_den, wg);
        const float sw = window_mass(wv, kh, wh, kw);
        float lo = INFINITY, hi = -INFINITY;
        for (int i = threadIdx.x; i < IH * IW; i += NT) {
            const int r = i / IW, c = i - r * IW, gy = y0 - (kh - 1) + r, gx = x0 - (kw - 1) + c;
            float xv = 0.0f, yv = 0.0f;
            if (gy >= 0 && gy < P.H && gx >= 0 && gx < P.W) {
                const int64_t o = gy * P.s2 + gx * P.s3;
                xv = xp[o];
                yv = yp[o];
                range_add(xv, lo, hi);
                range_add(yv, lo, hi);
            }
            in_x[i] = xv;
            in_y[i] = yv;
        }
        sh = block_shift(lo, hi, rng);
        shift_tile(lds, 2 * IH * IW, sh);
        __syncthreads();
        const int nV = QH * IW;
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
        // moments at the output positions that reach the tile, and the adjoint maps there (zero where no output exists)
        const int nD = QH * QW;
        for (int i = threadIdx.x; i < nD; i += NT) {
            const int b = i / QW, a = i - b * QW, qy = y0 - (kh - 1) + b, qx = x0 - (kw - 1) + a;
            float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
            if (qy >= 0 && qy < P.Ho && qx >= 0 && qx < P.Wo) {
                float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                for (int j = 0; j < kw; ++j) {
                    const float w = wh[j];
                    const int o = b * IW + a + j;
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(w, V[q * nV + o], m[q]);
                }
                // A from the means, B from the shifted moments (m[0], m[1] = mu1 - sh sum(w), mu2 - sh sum(w))
                const float mu1 = m[0] + sh * sw, mu2 = m[1] + sh * sw;
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
                const float a2 = mu1_sq + mu2_sq + P.C1, b2 = s1 + s2 + P.C2;
                const float A = (2.0f * mu12 + P.C1) / a2, B = (2.0f * s12 + P.C2) / b2;
                const float ga = g / a2, gb = g / b2;
                d0 = 2.0f * B * (mu2 - mu1 * A) * ga + 2.0f * A * (m[0] * B - m[1]) * gb;
                d1 = 2.0f * B * (mu1 - mu2 * A) * ga + 2.0f * A * (m[1] * B - m[0]) * gb;
                d2 = -(A * B) * gb;
                d3 = 2.0f * A * gb;
            }
            Dm[i] = d0; Dm[nD + i] = d1; Dm[2 * nD + i] = d2; Dm[3 * nD + i] = d3;
        }
        __syncthreads();
        // transposed horizontal pass onto the tile's 64 columns
        float *T = V;
        const int nT = QH * TX;
        for (int i = threadIdx.x; i < nT; i += NT) {
            const int b = i / TX, x = i % TX;
            float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = 0; j < kw; ++j) {
                const float w = wh[j];
                const int o = b * QW + x + kw - 1 - j;
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] += w * Dm[q * nD + o];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) T[q * nT + i] = t[q];
        }
        __syncthreads();
        Tt = T;
    }
    // transposed vertical pass, the chain through x, x^2 and xy, the mse term
    const int nT = (TY + kh - 1) * TX;
    for (int i = threadIdx.x; i < TY * TX; i += NT) {
        const int y = i / TX, x = i % TX, gy = y0 + y, gx = x0 + x;
        if (gy >= P.H || gx >= P.W) continue;
        const int64_t o = gy * P.s2 + gx * P.s3;
        const float xv = xp[o], yv = yp[o], e = wm * (xv - yv);
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (Tt) {
            for (int j = 0; j < kh; ++j) {
                const float w = wv[j];
                const int t = (y + kh - 1 - j) * TX + x;
#pragma unroll
                for (int q = 0; q < 4; ++q) r[q] += w * Tt[q * nT + t];
            }
        }
        const float xs = xv - sh, ys = yv - sh;   // the chain through the shifted x^2 and xy
        P.gx[base + o] = r[0] + 2.0f * xs * r[2] + ys * r[3] + e;
        if (P.gy) P.gy[base + o] = r[1] + 2.0f * ys * r[2] + xs * r[3] - e;
    }
}

int fill_params(LossParams &P, const LossArgs &a, bool bwd, size_t *lds) {
    P.x = a.x; P.y = a.y;
    P.s0 = a.strides[0]; P.s1 = a.strides[1]; P.s2 = a.strides[2]; P.s3 = a.strides[3];
    P.C = a.C; P.H = a.H; P.W = a.W;
    P.k = a.win_size;
    P.kh = a.H >= a.win_size ? a.win_size : 1;
    P.kw = a.W >= a.win_size ? a.win_size : 1;
    P.Ho = a.H - P.kh + 1; P.Wo = a.W - P.kw + 1;
    P.TY = bwd ? pick_ty(bwd_lds_floats, P.kh, P.kw, lds) : pick_ty(fwd_lds_floats, P.kh, P.kw, lds);
    if (P.TY == 0) return DR_EUNSUPPORTED;
    const int ext_x = bwd ? a.W : P.Wo, ext_y = bwd ? a.H : P.Ho;   // the forward tiles the output plane, the backward the input
    P.tiles_x = (ext_x + TX - 1) / TX;
    P.tiles = P.tiles_x * ((ext_y + P.TY - 1) / P.TY);
    P.planes = a.N * a.C;
    if ((int64_t)P.tiles * P.planes > INT32_MAX) return DR_EUNSUPPORTED;
    P.sigma_den = (float)(2.0 * a.win_sigma * a.win_sigma);
    P.C1 = (float)((a.K1 * a.data_range) * (a.K1 * a.data_range));
    P.C2 = (float)((a.K2 * a.data_range) * (a.K2 * a.data_range));
    P.nonneg = (a.flags & DR_SSIM_NONNEGATIVE) != 0;
    P.inv_px = 1.0 / ((double)P.Ho * P.Wo);
    P.inv_numel = 1.0 / ((double)P.planes * a.H * a.W);
    P.stats = a.stats; P.up = a.upstream; P.gx = a.grad_x; P.gy = a.grad_y;
    return 0;
}

template <typename K>
int launch_tiles(K kernel, const LossParams &P, size_t lds, hipStream_t stream) {
    if (lds > LDS_DEFAULT && allow_lds_impl(reinterpret_cast<const void *>(kernel), lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(P.tiles * P.planes)), dim3(NT), lds, stream, P);
    return (int)hipGetLastError();
}

}  // namespace

// three launches: zero the sums, the tiles, the finalize
int launch_dssim_mse_fwd(const LossArgs &a, hipStream_t stream) {
    LossParams P;
    size_t lds = 0;
    int rc = fill_params(P, a, false, &lds);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(a.stats, 0, sizeof(double) * (P.planes + 3), stream);
    if (e != hipSuccess) return (int)e;
    if ((rc = launch_tiles(dssim_mse_fwd_kernel, P, lds, stream))) return rc;
    hipLaunchKernelGGL(dssim_mse_finalize_kernel, dim3(1), dim3(NT), 0, stream, P);
    return (int)hipGetLastError();
}

// one launch
int launch_dssim_mse_bwd(const LossArgs &a, hipStream_t stream) {
    LossParams P;
    size_t lds = 0;
    int rc = fill_params(P, a, true, &lds);
    if (rc) return rc;
    return launch_tiles(dssim_mse_bwd_kernel, P, lds, stream);
}

}  // namespace dr
