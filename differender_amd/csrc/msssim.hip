// msssim.hip -- nan_to_num(1 - ms_ssim(x, y, data_range, weights)) + mse(x, y) and its gradient, fused,
// gfx950. The definition is the torch restatement differender_amd.utils.losses.ms_ssim2d / ms_dssim_mse_loss: at level l the
// SSIM and CS maps of ssim2d (f32 Gaussian window, separable VALID filtering along H then W, never skipped: the C entry asks
// for min(H, W) > 16 (k - 1)), their per-plane means; v_l = relu(CS_l) for l < L-1 and relu(SSIM_{L-1}) at the last level;
// between levels the 2x2 average pool with padding (H % 2, W % 2), padded zeros counted (every pooled pixel is its sum / 4);
// ms_nc = prod_l v_l^w_l, dms = 1 - mean(ms_nc), mse over the level-0 images.
//
// Pyramid: one launch per level 1..L-1 pools level l-1 into dense f32 planes of the workspace (level 0 is the caller's, read
// through its strides). Forward: ONE launch over the tiles of every level (flattened tile index), the tile scheme of D9 (the
// five shifted moments in LDS, a vertical then a horizontal pass); the level's CS or SSIM map summed f32 per lane, f64 per
// workgroup, one f64 atomic per workgroup into stats[l][plane]; level-0 tiles also sum the squared error. A one-workgroup
// finalize turns the sums into v, ms, loss, dms, mse.
//
// Backward: one launch per level, coarsest first, no atomics. With dL/dv_l = w_l ms / v_l dL/dms / (N C) (zero for the whole
// plane unless every v_l > 0), level l forms the adjoint maps of its term over the output positions reaching the tile:
//   CS   (l < L-1): B = b1/b2;  dB/dm3 = dB/dm4 = -B/b2,  dB/dm5 = 2/b2,  dB/dmu1 = 2(mu1 B - mu2)/b2  (mu2 by symmetry)
//   SSIM (l = L-1): the four maps of D9
// applies the transposed filter, adds 1/4 of the parent coarse pixel's dX_{l+1} (the pool's transpose: row y's parent is
// (y + H % 2) / 2) and stores dX_l (and dY_l) -- to the workspace, or at level 0 to grad_x / grad_y with the caller's strides
// plus the mse term. Each pixel's gradient is a fixed sequence of operations: bitwise the same run to run.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "dr_kernels.h"
#include "dr_ssim.h"
#include "../../include/differender_hip.h"

namespace dr {

hipError_t allow_lds_impl(const void *kernel, size_t bytes);  // capi.hip

namespace {

using namespace ssim;

struct MSLevel {
    const float *x, *y;         // level 0: the caller's images; level l > 0: dense [plane][H][W] planes of the workspace
    float *dx, *dy;             // backward: dX_l, dY_l (level 0: grad_x / grad_y, caller's strides; dy null when not wanted)
    int64_t s0, s1, s2, s3;     // element strides of x, y, dx, dy
    int H, W, Ho, Wo;
    int tiles_x, tiles;         // tiles per plane: forward over Ho x Wo, backward over H x W
    int block0;                 // forward: first flattened workgroup of this level
    double inv_px;              // 1 / (Ho Wo)
};

struct MSParams {
    MSLevel lv[MS_MAX_LEVELS];
    double w[MS_MAX_LEVELS];
    int L, C, planes, k, TY;
    float sigma_den, C1, C2;
    double inv_numel;           // 1 / (N C H W)
    double *stats;              // v[L][planes], ms[planes], loss, dms, mse
    const float *up;            // backward: (d loss, d dms, d mse) on the device, null = (1, 0, 0)
};

__device__ __forceinline__ int64_t plane_base(const MSLevel &V, int plane, int C) {
    return (int64_t)(plane / C) * V.s0 + (int64_t)(plane % C) * V.s1;
}

// level l (dense, in the workspace) from level l-1: out(r, c) = (sum of the in-range pixels of rows 2r - ph + {0, 1} and
// columns 2c - pw + {0, 1}) / 4, ph = H_{l-1} % 2, pw = W_{l-1} % 2 (avg_pool2d(2, padding=(ph, pw)), count_include_pad)
__global__ __launch_bounds__(NT) void msssim_pool_kernel(MSLevel S, int H, int W, float *ox, float *oy, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;   // = the dense output element [plane][r][c]
    if (i >= total) return;
    const int64_t pl = (int64_t)H * W;
    const int plane = (int)(i / pl), rem = (int)(i - plane * pl), r = rem / W, c = rem - r * W;
    const int y0 = 2 * r - (S.H & 1), x0 = 2 * c - (S.W & 1);
    const int64_t base = plane_base(S, plane, C);
    float sx[4], sy[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int yy = y0 + (q >> 1), xx = x0 + (q & 1);
        const bool in = yy >= 0 && yy < S.H && xx >= 0 && xx < S.W;
        const int64_t o = base + yy * S.s2 + xx * S.s3;
        sx[q] = in ? S.x[o] : 0.0f;
        sy[q] = in ? S.y[o] : 0.0f;
    }
    ox[i] = ((sx[0] + sx[1]) + (sx[2] + sx[3])) * 0.25f;
    oy[i] = ((sy[0] + sy[1]) + (sy[2] + sy[3])) * 0.25f;
}

__global__ __launch_bounds__(NT) void msssim_fwd_kernel(MSParams P) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ double red[2][NT / 64];
    __shared__ float rng[2 * NT / 64];
    int l = 0;
    for (int i = 1; i < P.L; ++i)
        if ((int)blockIdx.x >= P.lv[i].block0) l = i;
    const MSLevel &V = P.lv[l];
    const int blk = blockIdx.x - V.block0, tile = blk % V.tiles, plane = blk / V.tiles;
    const int x0 = (tile % V.tiles_x) * TX, y0 = (tile / V.tiles_x) * P.TY;
    const int TY = P.TY, k = P.k, IH = TY + k - 1, IW = TX + k - 1;
    const int64_t base = plane_base(V, plane, P.C);
    const float *xp = V.x + base, *yp = V.y + base;
    float *in_x = lds, *in_y = lds + IH * IW, *Vm = lds + 2 * IH * IW;   // Vm[5][TY][IW]
    build_window(k, P.sigma_den, wg);
    const bool last = l == P.L - 1;

    // the tile's input with its halo (zeros beyond the image feed only output positions that do not exist); at level 0 the
    // squared error of the pixels this tile owns: its own 64 x TY block, and up to the image edge for the last tile of a row /
    // column
    const bool last_x = x0 + TX >= V.Wo, last_y = y0 + TY >= V.Ho;
    const float sw = window_mass(wg, k, wg, k);
    float se = 0.0f, lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW, gy = y0 + r, gx = x0 + c;
        float xv = 0.0f, yv = 0.0f;
        if (gy < V.H && gx < V.W) {
            const int64_t o = gy * V.s2 + gx * V.s3;
            xv = xp[o];
            yv = yp[o];
            if (l == 0 && (r < TY || last_y) && (c < TX || last_x)) {
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
    const int nV = TY * IW;
    for (int i = threadIdx.x; i < nV; i += NT) {
        const int b = i / IW, c = i - b * IW;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f;
        for (int j = 0; j < k; ++j) {
            const float w = wg[j], xv = in_x[(b + j) * IW + c], yv = in_y[(b + j) * IW + c];
            a0 = fmaf(w, xv, a0); a1 = fmaf(w, yv, a1); a2 = fmaf(w, xv * xv, a2); a3 = fmaf(w, yv * yv, a3); a4 = fmaf(w, xv * yv, a4);
        }
        Vm[i] = a0; Vm[nV + i] = a1; Vm[2 * nV + i] = a2; Vm[3 * nV + i] = a3; Vm[4 * nV + i] = a4;
    }
    __syncthreads();
    // horizontal pass and the level's map: CS below the last level, SSIM at it
    float ss = 0.0f;
    for (int i = threadIdx.x; i < TY * TX; i += NT) {
        const int b = i / TX, a = i % TX;
        if (y0 + b >= V.Ho || x0 + a >= V.Wo) continue;
        float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < k; ++j) {
            const float w = wg[j];
            const int o = b * IW + a + j;
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fmaf(w, Vm[q * nV + o], m[q]);
        }
        const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
        const float cs = (2.0f * s12 + P.C2) / (s1 + s2 + P.C2);
        if (last) {
            const float mu1 = m[0] + sh * sw, mu2 = m[1] + sh * sw;
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            ss += ((2.0f * mu12 + P.C1) / (mu1_sq + mu2_sq + P.C1)) * cs;
        } else {
            ss += cs;
        }
    }
    const double ssum = block_sum((double)ss, red[0]);
    const double esum = l == 0 ? block_sum((double)se, red[1]) : 0.0;   // (l is workgroup-uniform)
    if (threadIdx.x == 0) {
        atomicAdd(&P.stats[l * P.planes + plane], ssum);
        if (l == 0) atomicAdd(&P.stats[(P.L + 1) * P.planes + 2], esum);
    }
}

// sums -> v (relu'd means), ms = prod v^w, then loss, dms, mse; deterministic tree over the planes
__global__ __launch_bounds__(NT) void msssim_finalize_kernel(MSParams P) {
    __shared__ double red[NT];
    double acc = 0.0;
    for (int p = threadIdx.x; p < P.planes; p += NT) {
        double ms = 1.0;
        for (int l = 0; l < P.L; ++l) {
            double v = P.stats[l * P.planes + p] * P.lv[l].inv_px;
            if (v <= 0.0) v = 0.0;   // relu (NaN passes through, as torch.relu's)
            P.stats[l * P.planes + p] = v;
            ms *= pow(v, P.w[l]);
        }
        P.stats[P.L * P.planes + p] = ms;
        acc += ms;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *tail = P.stats + (P.L + 1) * P.planes;
        const double dms = 1.0 - red[0] / P.planes;
        const double mse = tail[2] * P.inv_numel;
        // nan_to_num of the f32 dms: NaN -> 0, +-inf -> +-FLT_MAX
        const double d = isnan(dms) ? 0.0 : (isinf(dms) ? copysign((double)FLT_MAX, dms) : dms);
        tail[0] = d + mse;
        tail[1] = dms;
        tail[2] = mse;
    }
}

__global__ __launch_bounds__(NT) void msssim_bwd_kernel(MSParams P, int l) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ float rng[2 * NT / 64];
    const MSLevel &V = P.lv[l];
    const int tile = blockIdx.x % V.tiles, plane = blockIdx.x / V.tiles;
    const int x0 = (tile % V.tiles_x) * TX, y0 = (tile / V.tiles_x) * P.TY;
    const int TY = P.TY, k = P.k;
    const int64_t base = plane_base(V, plane, P.C);
    const float *xp = V.x + base, *yp = V.y + base;
    const bool last = l == P.L - 1;

    // dL/dv_l, then per map pixel: the product rule where every v of the plane is > 0 (else torch's relu and prod give the
    // plane no gradient), nan_to_num where dms is finite; upstream (d loss, d dms, d mse)
    double u0 = 1.0, u1 = 0.0, u2 = 0.0;
    if (P.up) { u0 = P.up[0]; u1 = P.up[1]; u2 = P.up[2]; }
    bool pass = true;
    for (int i = 0; i < P.L; ++i) pass = pass && P.stats[i * P.planes + plane] > 0.0;
    const double *tail = P.stats + (P.L + 1) * P.planes;
    const bool finite = isfinite(tail[1]);
    const float g = pass ? (float)(-(u0 * (finite ? 1.0 : 0.0) + u1) / P.planes * P.w[l] * P.stats[P.L * P.planes + plane] /
                                   P.stats[l * P.planes + plane] * V.inv_px)
                         : 0.0f;
    const float wm = l == 0 ? (float)(2.0 * (u0 + u2) * P.inv_numel) : 0.0f;

    const float *Tt = nullptr;
    float sh = 0.0f;
    // (workgroup-uniform) no MS gradient for this plane: skip the moments, and with them any 0 * NaN
    if (g != 0.0f) {
        const int IH = TY + 2 * (k - 1), IW = TX + 2 * (k - 1), QH = TY + k - 1, QW = TX + k - 1;
        const int r1 = max(2 * IH * IW, 4 * QH * QW);
        float *in_x = lds, *in_y = lds + IH * IW, *Dm = lds;   // region 1: the input, then the adjoint maps Dm[4][QH][QW]
        float *Vm = lds + r1;                                    // region 2: the vertical moments Vm[5][QH][IW], then Tt[4][QH][TX]
        build_window(k, P.sigma_den, wg);
        const float sw = window_mass(wg, k, wg, k);
        float lo = INFINITY, hi = -INFINITY;
        for (int i = threadIdx.x; i < IH * IW; i += NT) {
            const int r = i / IW, c = i - r * IW, gy = y0 - (k - 1) + r, gx = x0 - (k - 1) + c;
            float xv = 0.0f, yv = 0.0f;
            if (gy >= 0 && gy < V.H && gx >= 0 && gx < V.W) {
                const int64_t o = gy * V.s2 + gx * V.s3;
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
            for (int j = 0; j < k; ++j) {
                const float w = wg[j], xv = in_x[(b + j) * IW + c], yv = in_y[(b + j) * IW + c];
                a0 = fmaf(w, xv, a0); a1 = fmaf(w, yv, a1); a2 = fmaf(w, xv * xv, a2); a3 = fmaf(w, yv * yv, a3); a4 = fmaf(w, xv * yv, a4);
            }
            Vm[i] = a0; Vm[nV + i] = a1; Vm[2 * nV + i] = a2; Vm[3 * nV + i] = a3; Vm[4 * nV + i] = a4;
        }
        __syncthreads();
        // moments at the output positions that reach the tile, and the adjoint maps there (zero where no output exists)
        const int nD = QH * QW;
        for (int i = threadIdx.x; i < nD; i += NT) {
            const int b = i / QW, a = i - b * QW, qy = y0 - (k - 1) + b, qx = x0 - (k - 1) + a;
            float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
            if (qy >= 0 && qy < V.Ho && qx >= 0 && qx < V.Wo) {
                float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                for (int j = 0; j < k; ++j) {
                    const float w = wg[j];
                    const int o = b * IW + a + j;
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(w, Vm[q * nV + o], m[q]);
                }
                // B from the shifted moments (m[0], m[1] = mu1 - sh sum(w), mu2 - sh sum(w)); A from the means
                const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
                const float b2 = s1 + s2 + P.C2, B = (2.0f * s12 + P.C2) / b2;
                const float gb = g / b2;
                if (last) {
                    const float mu1 = m[0] + sh * sw, mu2 = m[1] + sh * sw;
                    const float a2 = mu1 * mu1 + mu2 * mu2 + P.C1, A = (2.0f * (mu1 * mu2) + P.C1) / a2;
                    const float ga = g / a2;
                    d0 = 2.0f * B * (mu2 - mu1 * A) * ga + 2.0f * A * (m[0] * B - m[1]) * gb;
                    d1 = 2.0f * B * (mu1 - mu2 * A) * ga + 2.0f * A * (m[1] * B - m[0]) * gb;
                    d2 = -(A * B) * gb;
                    d3 = 2.0f * A * gb;
                } else {
                    d0 = 2.0f * (m[0] * B - m[1]) * gb;
                    d1 = 2.0f * (m[1] * B - m[0]) * gb;
                    d2 = -B * gb;
                    d3 = 2.0f * gb;
                }
            }
            Dm[i] = d0; Dm[nD + i] = d1; Dm[2 * nD + i] = d2; Dm[3 * nD + i] = d3;
        }
        __syncthreads();
        // transposed horizontal pass onto the tile's 64 columns
        float *T = Vm;
        const int nT = QH * TX;
        for (int i = threadIdx.x; i < nT; i += NT) {
            const int b = i / TX, x = i % TX;
            float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = 0; j < k; ++j) {
                const float w = wg[j];
                const int o = b * QW + x + k - 1 - j;
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] += w * Dm[q * nD + o];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) T[q * nT + i] = t[q];
        }
        __syncthreads();
        Tt = T;
    }
    // transposed vertical pass, the chain through x, x^2 and xy, the parent's quarter, at level 0 the mse term
    const int nT = (TY + k - 1) * TX;
    const MSLevel *Q = last ? nullptr : &P.lv[l + 1];
    const int64_t qbase = last ? 0 : plane_base(*Q, plane, P.C);
    for (int i = threadIdx.x; i < TY * TX; i += NT) {
        const int y = i / TX, x = i % TX, gy = y0 + y, gx = x0 + x;
        if (gy >= V.H || gx >= V.W) continue;
        const int64_t o = gy * V.s2 + gx * V.s3;
        float rx = 0.0f, ry = 0.0f;
        if (Tt) {
            float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = 0; j < k; ++j) {
                const float w = wg[j];
                const int t = (y + k - 1 - j) * TX + x;
#pragma unroll
                for (int q = 0; q < 4; ++q) r[q] += w * Tt[q * nT + t];
            }
            const float xs = xp[o] - sh, ys = yp[o] - sh;   // the chain through the shifted x^2 and xy
            rx = r[0] + 2.0f * xs * r[2] + ys * r[3];
            ry = r[1] + 2.0f * ys * r[2] + xs * r[3];
        }
        if (Q) {
            const int64_t po = qbase + ((gy + (V.H & 1)) >> 1) * Q->s2 + ((gx + (V.W & 1)) >> 1) * Q->s3;
            rx += 0.25f * Q->dx[po];
            if (V.dy) ry += 0.25f * Q->dy[po];
        }
        if (l == 0) {
            const float e = wm * (xp[o] - yp[o]);
            rx += e;
            ry -= e;
        }
        V.dx[base + o] = rx;
        if (V.dy) V.dy[base + o] = ry;
    }
}

int fill_params(MSParams &P, const MSArgs &a, bool bwd, size_t *lds) {
    const MSLayout lay = msssim_layout(a.N, a.C, a.H, a.W, a.levels, a.grad_y != nullptr);
    char *ws = static_cast<char *>(a.workspace);
    P.L = a.levels; P.C = a.C; P.planes = a.N * a.C; P.k = a.win_size;
    P.TY = bwd ? pick_ty(bwd_lds_floats, P.k, P.k, lds) : pick_ty(fwd_lds_floats, P.k, P.k, lds);
    if (P.TY == 0) return DR_EUNSUPPORTED;
    int64_t blocks = 0;
    for (int l = 0; l < P.L; ++l) {
        MSLevel &V = P.lv[l];
        V.H = lay.H[l]; V.W = lay.W[l];
        V.Ho = V.H - P.k + 1; V.Wo = V.W - P.k + 1;
        if (l == 0) {
            V.x = a.x; V.y = a.y; V.dx = a.grad_x; V.dy = a.grad_y;
            V.s0 = a.strides[0]; V.s1 = a.strides[1]; V.s2 = a.strides[2]; V.s3 = a.strides[3];
        } else {
            V.x = reinterpret_cast<const float *>(ws + lay.x[l]);
            V.y = reinterpret_cast<const float *>(ws + lay.y[l]);
            V.dx = bwd ? reinterpret_cast<float *>(ws + lay.dx[l]) : nullptr;
            V.dy = bwd && a.grad_y ? reinterpret_cast<float *>(ws + lay.dy[l]) : nullptr;
            V.s3 = 1; V.s2 = V.W; V.s1 = (int64_t)V.H * V.W; V.s0 = V.s1 * a.C;
        }
        const int ext_x = bwd ? V.W : V.Wo, ext_y = bwd ? V.H : V.Ho;   // the forward tiles the output plane, the backward the input
        V.tiles_x = (ext_x + TX - 1) / TX;
        V.tiles = V.tiles_x * ((ext_y + P.TY - 1) / P.TY);
        V.block0 = (int)std::min<int64_t>(blocks, INT32_MAX);
        blocks += (int64_t)V.tiles * P.planes;
        V.inv_px = 1.0 / ((double)V.Ho * V.Wo);
        P.w[l] = a.weights[l];
    }
    if (blocks > INT32_MAX) return DR_EUNSUPPORTED;
    P.sigma_den = (float)(2.0 * a.win_sigma * a.win_sigma);
    P.C1 = (float)((a.K1 * a.data_range) * (a.K1 * a.data_range));
    P.C2 = (float)((a.K2 * a.data_range) * (a.K2 * a.data_range));
    P.inv_numel = 1.0 / ((double)P.planes * a.H * a.W);
    P.stats = a.stats; P.up = a.upstream;
    return 0;
}

template <typename K, typename... Args>
int launch_lds(K kernel, unsigned blocks, size_t lds, hipStream_t stream, Args... args) {
    if (lds > LDS_DEFAULT && allow_lds_impl(reinterpret_cast<const void *>(kernel), lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(NT), lds, stream, args...);
    return (int)hipGetLastError();
}

// levels 1..L-1 of the pyramid, one launch each
int launch_pyramid(const MSParams &P, hipStream_t stream) {
    for (int l = 1; l < P.L; ++l) {
        const int64_t total = (int64_t)P.planes * P.lv[l].H * P.lv[l].W;
        hipLaunchKernelGGL(msssim_pool_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, P.lv[l - 1],
                           P.lv[l].H, P.lv[l].W, const_cast<float *>(P.lv[l].x), const_cast<float *>(P.lv[l].y), P.C, total);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

// zero the sums, the pyramid (L-1 launches), the tiles of every level (one launch), the finalize
int launch_msssim_mse_fwd(const MSArgs &a, hipStream_t stream) {
    MSParams P;
    size_t lds = 0;
    int rc = fill_params(P, a, false, &lds);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(a.stats, 0, sizeof(double) * ((P.L + 1) * P.planes + 3), stream);
    if (e != hipSuccess) return (int)e;
    if ((rc = launch_pyramid(P, stream))) return rc;
    const MSLevel &last = P.lv[P.L - 1];
    const unsigned blocks = (unsigned)(last.block0 + last.tiles * P.planes);
    if ((rc = launch_lds(msssim_fwd_kernel, blocks, lds, stream, P))) return rc;
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(1), dim3(NT), 0, stream, P);
    return (int)hipGetLastError();
}

// the pyramid again (the workspace keeps nothing between calls), then one launch per level, coarsest first
int launch_msssim_mse_bwd(const MSArgs &a, hipStream_t stream) {
    MSParams P;
    size_t lds = 0;
    int rc = fill_params(P, a, true, &lds);
    if (rc) return rc;
    if ((rc = launch_pyramid(P, stream))) return rc;
    for (int l = P.L - 1; l >= 0; --l)
        if ((rc = launch_lds(msssim_bwd_kernel, (unsigned)(P.lv[l].tiles * P.planes), lds, stream, P, l))) return rc;
    return 0;
}

}  // namespace dr
