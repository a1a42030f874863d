// msssim.hip -- nan_to_num(1 - ms_ssim(x, y, data_range, weights)) + mse(x, y) and its gradient, fused,
// gfx950. The definition is the torch restatement differender_amd.utils.losses.ms_ssim2d / ms_dssim_mse_loss: at level l the
// SSIM and CS maps of ssim2d (f32 Gaussian window, separable VALID filtering along H then W, never skipped: the C entry asks
// for min(H, W) > 16 (k - 1)), their per-plane means; v_l = relu(CS_l) for l < L-1 and relu(SSIM_{L-1}) at the last level;
// between levels the 2x2 average pool with padding (H % 2, W % 2), padded zeros counted (every pooled pixel is its sum / 4);
// ms_nc = prod_l v_l^w_l, dms = 1 - mean(ms_nc), mse over the level-0 images.
//
// Pyramid: one launch per level 1..L-1 pools level l-1 into dense f32 planes of the workspace (level 0 is the caller's, read
// through its strides). Forward: ONE launch over the tiles of every level (flattened tile index), the tile of D9 (csrc/dr_ssim.h,
// one definition for both losses: the five shifted moments in LDS, a vertical then a horizontal pass, the SSIM or CS map and
// their adjoints); the level's CS or SSIM map summed f32 per lane, f64 per
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
#include <math.h>

#include "dr_kernels.h"
#include "dr_ssim.h"
#include "../../include/differender_hip.h"

namespace dr {
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
__device__ __forceinline__ Plane plane_of(const MSLevel &V, int64_t base) {
    return {V.x + base, V.y + base, V.s2, V.s3, V.H, V.W, V.Ho, V.Wo};
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
    build_window(P.k, P.sigma_den, wg);
    // the level's map: CS below the last level, SSIM at it (l is workgroup-uniform); level-0 tiles also sum the squared error
    float se = 0.0f;
    const float ss = tile_map_sum(plane_of(V, plane_base(V, plane, P.C)), y0, x0, P.TY, Window{wg, wg, P.k, P.k, P.C1, P.C2},
                                  l == P.L - 1, l == 0, lds, rng, se);
    const double ssum = block_sum((double)ss, red[0]);
    const double esum = l == 0 ? block_sum((double)se, red[1]) : 0.0;
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
    finalize_tail(acc, red, P.planes, P.inv_numel, P.stats + (P.L + 1) * P.planes);
}

__global__ __launch_bounds__(NT) void msssim_bwd_kernel(MSParams P, int l) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ float rng[2 * NT / 64];
    const MSLevel &V = P.lv[l];
    const int tile = blockIdx.x % V.tiles, plane = blockIdx.x / V.tiles;
    const int x0 = (tile % V.tiles_x) * TX, y0 = (tile / V.tiles_x) * P.TY;
    const int64_t base = plane_base(V, plane, P.C);
    const Plane pl = plane_of(V, base);
    const Window w = {wg, wg, P.k, P.k, P.C1, P.C2};
    const bool last = l == P.L - 1;   // (workgroup-uniform)

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

    const float *T = nullptr;
    float sh = 0.0f;
    // (workgroup-uniform) no MS gradient for this plane: skip the moments, and with them any 0 * NaN
    if (g != 0.0f) {
        build_window(P.k, P.sigma_den, wg);
        T = tile_adjoint_h(pl, y0, x0, P.TY, w, last, g, lds, rng, sh);
    }
    // transposed vertical pass and the chain (skipped where T is null: such a plane's gradient is the parent's quarter and the
    // mse term alone, also at a non-finite pixel), the parent's quarter, at level 0 the mse term
    const MSLevel *Q = last ? nullptr : &P.lv[l + 1];
    const int64_t qbase = last ? 0 : plane_base(*Q, plane, P.C);
    for (int i = threadIdx.x; i < P.TY * TX; i += NT) {
        const int y = i / TX, x = i % TX, gy = y0 + y, gx = x0 + x;
        if (gy >= V.H || gx >= V.W) continue;
        const int64_t o = gy * V.s2 + gx * V.s3;
        float rx = 0.0f, ry = 0.0f;
        if (T) adjoint_v(T, P.TY, y, x, w, pl.x[o] - sh, pl.y[o] - sh, rx, ry);
        if (Q) {
            const int64_t po = qbase + ((gy + (V.H & 1)) >> 1) * Q->s2 + ((gx + (V.W & 1)) >> 1) * Q->s3;
            rx += 0.25f * Q->dx[po];
            if (V.dy) ry += 0.25f * Q->dy[po];
        }
        if (l == 0) {
            const float e = wm * (pl.x[o] - pl.y[o]);
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
    fill_common(P, a);
    P.L = a.levels;
    P.TY = pick_ty(bwd, P.k, P.k, lds);
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
        tile_counts(V.H, V.W, V.Ho, V.Wo, P.TY, bwd, &V.tiles_x, &V.tiles);
        V.block0 = (int)std::min<int64_t>(blocks, INT32_MAX);
        blocks += (int64_t)V.tiles * P.planes;
        V.inv_px = 1.0 / ((double)V.Ho * V.Wo);
        P.w[l] = a.weights[l];
    }
    return blocks > INT32_MAX ? DR_EUNSUPPORTED : 0;
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
