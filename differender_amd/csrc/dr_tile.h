// dr_tile.h -- what the one-lane-per-ray march kernels (march_baseline.hip, march_tf2d.hip, camera_grad.hip) share around their
// sample loops: the kernel parameters every one of them reads and their one builder, the volume view (the brick kernels' too),
// the launch shape, staging a view's table in LDS, and the LDS budget.
#pragma once
#include <hip/hip_runtime.h>
#include "dr_device.h"
#include "dr_kernels.h"
#include "../../include/differender_hip.h"

namespace dr {

template <typename VT>
static inline VolView<VT> make_vol_view(const MarchArgs &a) {
    VolView<VT> v;
    v.p = static_cast<const VT *>(a.vol);
    v.sx = a.sx; v.sy = a.sy; v.sz = a.sz;
    v.VX = a.VX; v.VY = a.VY; v.VZ = a.VZ;
    v.scx = (float)((double)a.VX - 1.0 - 1e-4);
    v.scy = (float)((double)a.VY - 1.0 - 1e-4);
    v.scz = (float)((double)a.VZ - 1.0 - 1e-4);
    return v;
}

// The fields of MarchArgs every per-ray kernel reads, in device form (tf_vs and dtf_vs in float4 texels). Each kernel family
// derives its own parameters from this (trivially copyable: it is passed by value as the kernel argument). The table's shape
// sits next to it: where the fields lie in the kernel argument moves the kernels' register counts.
template <typename VT>
struct RayParams {
    VolView<VT> vol; int64_t vol_vs;
    const float4 *tf; int64_t tf_vs;
    int R, RG; float tf_len, lg, g_scale;   // [R][RG] texels (RG = 1: the 1-D TF), tf_len = R - 1, lg = RG - 1; g_scale: 2-D TF
    const float *cam, *entry, *exit_, *rays; const int32_t *nsamp;
    int W, H, S; float inv_sr;
    float *out; int32_t *steps;
    const float *grad_out, *out_fwd;
    GradView dvol; int64_t dvol_vs;
    float *d_tf; int64_t dtf_vs;
};

template <typename VT>
static inline RayParams<VT> make_ray_params(const MarchArgs &a) {
    RayParams<VT> P;
    P.vol = make_vol_view<VT>(a); P.vol_vs = a.vol_vs;
    P.tf = reinterpret_cast<const float4 *>(a.tf); P.tf_vs = a.tf_vs / 4;
    P.R = a.R; P.RG = a.RG; P.tf_len = (float)(a.R - 1); P.lg = (float)(a.RG - 1); P.g_scale = a.g_scale;
    P.cam = a.cam; P.entry = a.entry; P.exit_ = a.exit_; P.rays = a.rays; P.nsamp = a.nsamp;
    P.W = a.W; P.H = a.H; P.S = a.S; P.inv_sr = 1.0f / a.sr;
    P.out = a.out; P.steps = a.steps;
    P.grad_out = a.grad_out; P.out_fwd = a.out_fwd;
    P.dvol.p = a.d_vol; P.dvol.sx = a.dsx; P.dvol.sy = a.dsy; P.dvol.sz = a.dsz; P.dvol_vs = a.dvol_vs;
    P.d_tf = a.d_tf; P.dtf_vs = a.dtf_vs / 4;
    return P;
}

// one lane per ray, one wave per 8x8 pixel tile, four waves per 256-thread workgroup
__device__ __forceinline__ bool tile_pixel(int W, int H, int &i, int &j) {
    const int tiles_j = (H + 7) >> 3;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    i = (wave / tiles_j) * 8 + (lane >> 3);
    j = (wave % tiles_j) * 8 + (lane & 7);
    return i < W && j < H;
}

static inline dim3 tile_grid(int W, int H, int n_views) {
    const int tiles = ((W + 7) / 8) * ((H + 7) / 8);
    return dim3((tiles + 3) / 4, n_views);
}

// The first n texels of this view's table tf: copied to LDS when LDS (with nzero doubles of the caller's LDS cleared, then a
// barrier), else read where they lie. Returns what the kernel reads them from.
template <bool LDS>
__device__ __forceinline__ const float4 *stage_table(float4 *lds, const float4 *tf, int n, double *zero = nullptr,
                                                     int nzero = 0) {
    if (!LDS) return tf;
    for (int k = threadIdx.x; k < n; k += 256) lds[k] = tf[k];
    for (int k = threadIdx.x; k < nzero; k += 256) zero[k] = 0.0;
    __syncthreads();
    return lds;
}

hipError_t allow_lds_impl(const void *kernel, size_t bytes);  // capi.hip
template <typename K>
static hipError_t big_lds(K kernel, size_t bytes) {  // dynamic LDS above 64 KB needs an explicit opt-in (once per kernel)
    if (bytes <= 64 * 1024) return hipSuccess;
    return allow_lds_impl(reinterpret_cast<const void *>(kernel), bytes);
}

// One launch of a per-ray kernel on the tile grid of a's image and views, with `lds` bytes of dynamic LDS.
template <typename Params>
static int launch_tiles(void (*kernel)(Params), const MarchArgs &a, size_t lds, hipStream_t stream, const Params &P) {
    if (big_lds(kernel, lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, tile_grid(a.W, a.H, a.n_views), dim3(256), lds, stream, P);
    return (int)hipGetLastError();
}

// What one workgroup may really ask for: the runtime does not grant a CU's full 160 KiB (163 232 B launched, 163 616 B did not:
// tools/lds_limit_probe.py, round 5) -- 1 KiB of headroom, as brick_path_supported keeps. A table that does not fit drops to the
// next tier instead of failing at launch (R = 3409 .. 3413 and 10 227 .. 10 240 picked a tier the launch refused).
constexpr size_t LDS_PER_CU = 159 * 1024;

}  // namespace dr
