// dr_tile.h -- what the one-lane-per-ray kernels (march_baseline.hip, march_tf2d.hip, march_lit.hip, march_rgba.hip,
// camera_grad.hip, projection.hip) share around their sample loops: the kernel parameters every one of them reads and their one
// builder, the volume view (the brick kernels' too), the launch shape, opening a lane's ray, staging a view's table in LDS, the
// d_vol and d_tf contributions of a sample, and the LDS budget with the table tiers it gives.
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

__device__ __forceinline__ float4 mix4(float4 x, float4 y, float a) {
    return make_float4(mixf(x.x, y.x, a), mixf(x.y, y.y, a), mixf(x.z, y.z, a), mixf(x.w, y.w, a));
}
__device__ __forceinline__ float4 sub4(float4 x, float4 y) { return make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w); }
__device__ __forceinline__ float4 scale4(float4 x, float s) { return make_float4(x.x * s, x.y * s, x.z * s, x.w * s); }

// A lane's ray as every per-ray kernel opens it, given its index p in the [views][W][H] buffers: the view's volume, the camera
// position, the ray buffers' entries and the view direction; ADJ: the upstream gradient and the forward's pixel too. (How many
// samples are marched is the kernel's: the clips differ on purpose.)
template <typename VT>
struct Ray {
    VolView<VT> vol; f3 cam; RayGeom rg; f3 vd;
    float4 go, of;
};

__device__ __forceinline__ size_t ray_index(int W, int H, int view, int i, int j) { return ((size_t)view * W + i) * H + j; }

// The arguments are the fields of RayParams (or of march_rgba.hip's RgbaParams, which names them alike), one by one as
// pose_ray's and camera_ray_tail's are: a kernel that hands its whole parameter struct to a function reads all of it at entry,
// which moves the registers of every kernel that did not do so before. dv: the kernel's d_vol view, moved to this view too,
// or null (no d_vol here, or none wanted).
// The two halves are for a kernel with per-view loads of its own, which lie between them (the lit march's light): the order of
// the loads is the order the compiler schedules from.
template <typename VT>
__device__ __forceinline__ void open_view(Ray<VT> &r, int view, VolView<VT> vol, int64_t vol_vs, const float *cam,
                                          GradView *dv = nullptr, int64_t dvol_vs = 0) {
    r.vol = vol;
    r.vol.p += view * vol_vs;
    if (dv) dv->p += view * dvol_vs;
    r.cam = make_f3(cam[3 * view], cam[3 * view + 1], cam[3 * view + 2]);
}
template <typename VT>
__device__ __forceinline__ void open_adjoint(Ray<VT> &r, size_t p, const float *grad_out, const float *out_fwd) {
    r.go = reinterpret_cast<const float4 *>(grad_out)[p];
    r.of = reinterpret_cast<const float4 *>(out_fwd)[p];
}
template <bool ADJ, typename VT>
__device__ __forceinline__ void open_geom(Ray<VT> &r, size_t p, const float *entry, const float *exit_, const float *rays,
                                          const int32_t *nsamp, const float *grad_out = nullptr, const float *out_fwd = nullptr) {
    load_ray(entry, exit_, rays, nsamp, p, r.rg);
    r.vd = make_f3(r.rg.vx, r.rg.vy, r.rg.vz);
    if (ADJ) open_adjoint(r, p, grad_out, out_fwd);
}
template <bool ADJ, typename VT>
__device__ __forceinline__ void open_ray(Ray<VT> &r, int view, size_t p, VolView<VT> vol, int64_t vol_vs, const float *cam,
                                         const float *entry, const float *exit_, const float *rays, const int32_t *nsamp,
                                         const float *grad_out = nullptr, const float *out_fwd = nullptr, GradView *dv = nullptr,
                                         int64_t dvol_vs = 0) {
    open_view(r, view, vol, vol_vs, cam, dv, dvol_vs);
    open_geom<ADJ>(r, p, entry, exit_, rays, nsamp, grad_out, out_fwd);
}

template <typename VT>
__device__ __forceinline__ void sample_pos(const Ray<VT> &r, int s, float &px, float &py, float &pz) {
    sample_pos(r.rg, r.cam.x, r.cam.y, r.cam.z, s, px, py, pz);
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

// d_vol of one sample through its taps (global float atomics): the adjoint (gx, gy, gz) of the three central differences of
// the normal on the six taps at +-delta ...
template <typename VT>
__device__ __forceinline__ void scatter_normal_taps(const VolView<VT> &vol, const GradView &dv, const Sample &sm, float gx, float gy,
                                                    float gz) {
    const float delta = 1e-3f;
    tri_scatter_global(vol, dv, sm.px + delta, sm.py, sm.pz, gx);
    tri_scatter_global(vol, dv, sm.px - delta, sm.py, sm.pz, -gx);
    tri_scatter_global(vol, dv, sm.px, sm.py + delta, sm.pz, gy);
    tri_scatter_global(vol, dv, sm.px, sm.py - delta, sm.pz, -gy);
    tri_scatter_global(vol, dv, sm.px, sm.py, sm.pz + delta, gz);
    tri_scatter_global(vol, dv, sm.px, sm.py, sm.pz - delta, -gz);
}
// ... and all seven: I_bar on the intensity tap, the six unless the normal is flat (D1)
template <typename VT>
__device__ __forceinline__ void scatter_taps(const VolView<VT> &vol, const GradView &dv, const Sample &sm, float I_bar, float gx,
                                             float gy, float gz) {
    tri_scatter_global(vol, dv, sm.px, sm.py, sm.pz, I_bar);
    if (!sm.flat) scatter_normal_taps(vol, dv, sm, gx, gy, gz);
}

// d_tf of one sample of the 1-D table, onto its two texels: float atomics on the view's rows of the caller's tensor (sat: the
// saturating add of the sanitising backward's second pass) ...
__device__ __forceinline__ void dtf_add(float *dtf, const Sample &sm, const SampleAdj &ad, bool sat) {
    const float w0 = 1.0f - sm.fr, w1 = sm.fr;
    float *d0 = dtf + 4 * sm.lo, *d1 = dtf + 4 * sm.hi;
    const float v8[8] = {w0 * ad.r_bar, w0 * ad.g_bar, w0 * ad.b_bar, w0 * ad.a_bar, w1 * ad.r_bar, w1 * ad.g_bar, w1 * ad.b_bar, w1 * ad.a_bar};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (sat) { atomic_add_sat(d0 + q, v8[q]); atomic_add_sat(d1 + q, v8[4 + q]); }
        else { unsafeAtomicAdd(d0 + q, v8[q]); unsafeAtomicAdd(d1 + q, v8[4 + q]); }
    }
}
// ... or the workgroup's table in LDS, in DOUBLE: thousands of samples of a workgroup land on a few texels (all of them on one
// when R = 1), and f32 atomics in thread order put 1e-3 of summation noise on d_tf at sampling rate 16 (fuzz seed 603239,
// round 4); the oracle sums d_tf in double for the same reason (its d_tf accumulators), so this keeps the twin a twin
__device__ __forceinline__ void dtf_add(double *lds_dtf, const Sample &sm, const SampleAdj &ad) {
    const float w0 = 1.0f - sm.fr, w1 = sm.fr;
    double *d0 = lds_dtf + 4 * sm.lo, *d1 = lds_dtf + 4 * sm.hi;   // (the products are f32, as in the oracle)
    atomicAdd(d0 + 0, (double)(w0 * ad.r_bar)); atomicAdd(d0 + 1, (double)(w0 * ad.g_bar));
    atomicAdd(d0 + 2, (double)(w0 * ad.b_bar)); atomicAdd(d0 + 3, (double)(w0 * ad.a_bar));
    atomicAdd(d1 + 0, (double)(w1 * ad.r_bar)); atomicAdd(d1 + 1, (double)(w1 * ad.g_bar));
    atomicAdd(d1 + 2, (double)(w1 * ad.b_bar)); atomicAdd(d1 + 3, (double)(w1 * ad.a_bar));
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

// What a workgroup keeps in LDS of a table of `texels` float4, and the dynamic LDS bytes of its launch --
//   2: the table + its gradient table in double (48 B a texel; only when want_dtf);
//   1: the table only; a forward stages it, a backward sends d_tf to the caller's tensor with float atomics (16 B a texel);
//   0: nothing: the table is read where it lies, through the caches (the reference has no limit on the TF resolution).
// extra: bytes the kernel keeps beside the table in tiers 1 and 2; min_bytes: what the launch needs whatever the tier (a
// reduction that overlays the tables). (The camera gradient keeps its own 48 KiB limit in cam_dispatch, where a test reads it.)
struct TableTier { int tables; size_t lds; };
constexpr TableTier table_tier(size_t texels, bool want_dtf, size_t min_bytes = 0, size_t extra = 0) {
    const size_t lds2 = texels * (sizeof(float4) + 4 * sizeof(double)) + extra, lds1 = texels * sizeof(float4) + extra;
    const int tables = (want_dtf && lds2 <= LDS_PER_CU) ? 2 : (lds1 <= LDS_PER_CU ? 1 : 0);
    const size_t lds = tables == 2 ? lds2 : (tables == 1 ? lds1 : 0);
    return {tables, lds < min_bytes ? min_bytes : lds};
}
static_assert(table_tier(3392, true).tables == 2 && table_tier(3393, true).tables == 1, "1-D backward: the double table to R = 3392");
static_assert(table_tier(10176, true).tables == 1 && table_tier(10177, true).tables == 0, "1-D backward: the TF to R = 10176");
static_assert(table_tier(3392, false).tables == 1, "2-D TF backward without d_tf: no gradient table");
static_assert(table_tier(2, true, 320).tables == 2 && table_tier(2, true, 320).lds == 320, "lit backward: never below LIGHT_RED_BYTES");
static_assert(table_tier(10176, false).tables == 1 && table_tier(10177, false).tables == 0, "forward: the TF to R = 10176");
static_assert(table_tier(10177, false).lds == 0 && table_tier(3392, true).lds == 3392 * 48, "the bytes of the tier taken");

}  // namespace dr
