// dr_bundle.h -- what the ray-bundle kernels (march_bundle.hip, projection_bundle.hip) share: the lane's ray index, opening a
// lane's ray from its own origin, and the launch shape. One lane per ray, 256-lane workgroups over the linear ray index
// p in [0, N) -- no pixel tile: 64 consecutive rays share a wave, so the memory coherence of a bundle is the caller's ray order.
#pragma once
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

static dim3 bundle_grid(int N) { return dim3((unsigned)(((int64_t)N + 255) / 256)); }

// One launch of a bundle kernel: ceil(N / 256) workgroups of 256 lanes, `lds` bytes of dynamic LDS.
template <typename Params>
static int launch_bundle(void (*kernel)(Params), int N, size_t lds, hipStream_t stream, const Params &P) {
    if (big_lds(kernel, lds) != hipSuccess) return DR_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, bundle_grid(N), dim3(256), lds, stream, P);
    return (int)hipGetLastError();
}

}  // namespace dr
