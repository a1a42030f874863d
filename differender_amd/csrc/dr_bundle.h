// dr_bundle.h -- what the ray-bundle kernels (march_bundle.hip, projection_bundle.hip, march_rgba_bundle.hip,
// march_depth_bundle.hip) share: the lane's ray index, opening a lane's ray from its own origin, the once-per-ray tail of a ray
// gradient, and the launch shape. One lane per ray, 256-lane workgroups over the linear ray index
// p in [0, N) -- no pixel tile: 64 consecutive rays share a wave, so the memory coherence of a bundle is the caller's ray order.
#pragma once
#include "dr_camera.h"
#include "dr_tile.h"

namespace dr {

__device__ __forceinline__ int bundle_ray() { return (int)(blockIdx.x * 256u + threadIdx.x); }
__device__ __forceinline__ f3 load_f3(const float *a, size_t p) { return make_f3(a[3 * p], a[3 * p + 1], a[3 * p + 2]); }

// open_ray for a lane's own origin: the (single) volume, the ray buffers' entries, the direction; ADJ: the upstream gradient and
// the forward's pixel too
template <bool ADJ, typename VT>
__device__ __forceinline__ void open_bundle_ray(Ray<VT> &r, size_t p, VolView<VT> vol, const float *origins, const float *entry,
                                                const float *exit_, const float *dirs, const int32_t *nsamp,
                                                const float *grad_out = nullptr, const float *out_fwd = nullptr) {
    r.vol = vol;
    r.cam = load_f3(origins, p);
    open_geom<ADJ>(r, p, entry, exit_, dirs, nsamp, grad_out, out_fwd);
}

// The once-per-ray tail of a bundle's ray gradient, from the four sums of the walk over the forward's live samples
// -- sP = sum P_s, sTG = sum t_s G_s (+ D_s), s0 = sum (1 - f_s) gv_s, s1 = sum f_s gv_s -- the faces the forward picked, the
// t_near clamp it took and the jitter draw u behind A. With tmin = (f_a - o_a) / d_a on the face axis a, tmax likewise on b,
// t0 = A tmin + (1 - A) tmax and A = (1 - u/n)(1 - 0.5/n) (D8):
//   d origin = sP  - (k_min / d_a) e_a      - (k_max / d_b) e_b,
//   d dir    = sTG - (k_min tmin / d_a) e_a - (k_max tmax / d_b) e_b,
// k_min = s0 A (0 where the clamp was taken: tmin is then a constant), k_max = s0 (1 - A) + s1. d dir is the gradient w.r.t. the
// direction as a free 3-vector. D5 per component: a NaN ray contributes nothing, infinities are clamped.
// (march_bundle.hip, march_rgba_bundle.hip and projection_bundle.hip still carry their own copies of these statements.)
__device__ __forceinline__ void bundle_ray_tail(f3 lf, f3 vd, int n, float u, float t_near, f3 sP, f3 sTG, float s0, float s1,
                                                f3 &d_o, f3 &d_d) {
    const SlabFaces sf = slab_faces(lf, vd);
    const bool clamped = t_near > -INFINITY && sf.tmin < t_near;
    const float nf = (float)n;
    const float Acoef = (1.0f - u / nf) * (1.0f - 0.5f / nf);
    const float k_min = clamped ? 0.0f : s0 * Acoef, k_max = fmaf(s0, 1.0f - Acoef, s1);
    const f3 emin = make_f3(sf.amin == 0 ? 1.0f : 0.0f, sf.amin == 1 ? 1.0f : 0.0f, sf.amin == 2 ? 1.0f : 0.0f);
    const f3 emax = make_f3(sf.amax == 0 ? 1.0f : 0.0f, sf.amax == 1 ? 1.0f : 0.0f, sf.amax == 2 ? 1.0f : 0.0f);
    const float cmin = -k_min * sf.ivmin, cmax = -k_max * sf.ivmax;
    d_o = f3_fma(cmax, emax, f3_fma(cmin, emin, sP));
    d_d = f3_fma(cmax * sf.tmax, emax, f3_fma(cmin * sf.tmin, emin, sTG));
    d_o = make_f3(finite_or_zero(d_o.x), finite_or_zero(d_o.y), finite_or_zero(d_o.z));
    d_d = make_f3(finite_or_zero(d_d.x), finite_or_zero(d_d.y), finite_or_zero(d_d.z));
}

static dim3 bundle_grid(int N) { return dim3((unsigned)(((int64_t)N + 255) / 256)); }

// One launch of a bundle kernel: ceil(N / 256) workgroups of 256 lanes, `lds` bytes of dynamic LDS.
template <typename Params>
static int launch_bundle(void (*kernel)(Params), int N, size_t lds, hipStream_t stream, const Params &P) {
    if (big_lds(kernel, lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, bundle_grid(N), dim3(256), lds, stream, P);
    return (int)hipGetLastError();
}

}  // namespace dr
