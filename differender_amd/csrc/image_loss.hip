// image_loss.hip -- the demo's image loss nan_to_num(1 - ssim(res, gt, data_range, nonnegative_ssim)) + mse(res, gt)
// (examples/test_opt_tf.py:70-72, "OPT.py") and its gradient, fused, gfx950. The definition is the torch
// restatement differender_amd.utils.losses.ssim2d / dssim_mse_loss: Gaussian window built in f32 and normalised by its f32
// sum, separable VALID filtering along H then W, a pass skipped when its side is shorter than the window (a skipped pass is
// the one-tap window {1} here, which is exact), the per-plane mean of the SSIM map, relu on it when nonnegative, the mean over
// planes, and the mse over the full images.
//
// The tile itself (staging, shift, the passes, the SSIM formula and its adjoint) is csrc/dr_ssim.h's, shared with msssim.hip;
// here are the plane lookup, dL/dS_nc, the mse term, the stores and the atomics.
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
#include <math.h>

#include "dr_kernels.h"
#include "dr_ssim.h"
#include "../../include/differender_hip.h"

namespace dr {
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

__device__ __forceinline__ int64_t plane_base(const LossParams &P, int plane) {
    return (int64_t)(plane / P.C) * P.s0 + (int64_t)(plane % P.C) * P.s1;
}
__device__ __forceinline__ Plane plane_of(const LossParams &P, int64_t base) {
    return {P.x + base, P.y + base, P.s2, P.s3, P.H, P.W, P.Ho, P.Wo};
}

__global__ __launch_bounds__(NT) void dssim_mse_fwd_kernel(LossParams P) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ double red[2][NT / 64];
    __shared__ float rng[2 * NT / 64];
    const int tile = blockIdx.x % P.tiles, plane = blockIdx.x / P.tiles;
    const int x0 = (tile % P.tiles_x) * TX, y0 = (tile / P.tiles_x) * P.TY;
    build_window(P.k, P.sigma_den, wg);
    float se = 0.0f;
    const float ss = tile_map_sum(plane_of(P, plane_base(P, plane)), y0, x0, P.TY, make_window(wg, P.kh, P.kw, P.C1, P.C2), true, true,
                                  lds, rng, se);
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
    finalize_tail(acc, red, P.planes, P.inv_numel, P.stats + P.planes);
}

__global__ __launch_bounds__(NT) void dssim_mse_bwd_kernel(LossParams P) {
    extern __shared__ float lds[];
    __shared__ float wg[KMAX + 1];
    __shared__ float rng[2 * NT / 64];
    const int tile = blockIdx.x % P.tiles, plane = blockIdx.x / P.tiles;
    const int x0 = (tile % P.tiles_x) * TX, y0 = (tile / P.tiles_x) * P.TY;
    const int64_t base = plane_base(P, plane);
    const Plane pl = plane_of(P, base);
    const Window w = make_window(wg, P.kh, P.kw, P.C1, P.C2);

    // dL/dS_nc: relu passes where S > 0, nan_to_num where dssim is finite; upstream (d loss, d dssim, d mse)
    double u0 = 1.0, u1 = 0.0, u2 = 0.0;
    if (P.up) { u0 = P.up[0]; u1 = P.up[1]; u2 = P.up[2]; }
    const bool pass = !P.nonneg || P.stats[plane] > 0.0;
    const bool finite = isfinite(P.stats[P.planes + 1]);
    const float g = pass ? (float)(-(u0 * (finite ? 1.0 : 0.0) + u1) / P.planes * P.inv_px) : 0.0f;
    const float wm = (float)(2.0 * (u0 + u2) * P.inv_numel);

    const float *T = nullptr;
    float sh = 0.0f;
    // (workgroup-uniform) no SSIM gradient for this plane: the mse term alone, and no 0 * NaN from the moments
    if (g != 0.0f) {
        build_window(P.k, P.sigma_den, wg);
        T = tile_adjoint_h(pl, y0, x0, P.TY, w, true, g, lds, rng, sh);
    }
    // transposed vertical pass and the chain (through zero maps where T is null: NaN at an infinite pixel), the mse term
    for (int i = threadIdx.x; i < P.TY * TX; i += NT) {
        const int y = i / TX, x = i % TX, gy = y0 + y, gx = x0 + x;
        if (gy >= P.H || gx >= P.W) continue;
        const int64_t o = gy * P.s2 + gx * P.s3;
        const float xv = pl.x[o], yv = pl.y[o], e = wm * (xv - yv);
        float rx, ry;
        adjoint_v(T, P.TY, y, x, w, xv - sh, yv - sh, rx, ry);
        P.gx[base + o] = rx + e;
        if (P.gy) P.gy[base + o] = ry - e;
    }
}

int fill_params(LossParams &P, const LossArgs &a, bool bwd, size_t *lds) {
    fill_common(P, a);
    P.x = a.x; P.y = a.y;
    P.s0 = a.strides[0]; P.s1 = a.strides[1]; P.s2 = a.strides[2]; P.s3 = a.strides[3];
    P.H = a.H; P.W = a.W;
    P.kh = a.H >= a.win_size ? a.win_size : 1;
    P.kw = a.W >= a.win_size ? a.win_size : 1;
    P.Ho = a.H - P.kh + 1; P.Wo = a.W - P.kw + 1;
    P.TY = pick_ty(bwd, P.kh, P.kw, lds);
    if (P.TY == 0) return DR_EUNSUPPORTED;
    tile_counts(P.H, P.W, P.Ho, P.Wo, P.TY, bwd, &P.tiles_x, &P.tiles);
    if ((int64_t)P.tiles * P.planes > INT32_MAX) return DR_EUNSUPPORTED;
    P.nonneg = (a.flags & DR_SSIM_NONNEGATIVE) != 0;
    P.inv_px = 1.0 / ((double)P.Ho * P.Wo);
    P.gx = a.grad_x; P.gy = a.grad_y;
    return 0;
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
    if ((rc = launch_lds(dssim_mse_fwd_kernel, (unsigned)(P.tiles * P.planes), lds, stream, P))) return rc;
    hipLaunchKernelGGL(dssim_mse_finalize_kernel, dim3(1), dim3(NT), 0, stream, P);
    return (int)hipGetLastError();
}

// one launch
int launch_dssim_mse_bwd(const LossArgs &a, hipStream_t stream) {
    LossParams P;
    size_t lds = 0;
    int rc = fill_params(P, a, true, &lds);
    if (rc) return rc;
    return launch_lds(dssim_mse_bwd_kernel, (unsigned)(P.tiles * P.planes), lds, stream, P);
}

}  // namespace dr
