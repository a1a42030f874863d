// dr_tile.h -- launch shape and LDS budget shared by the one-lane-per-ray march kernels (march_baseline.hip, march_tf2d.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace dr {

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

hipError_t allow_lds_impl(const void *kernel, size_t bytes);  // capi.hip
template <typename K>
static hipError_t big_lds(K kernel, size_t bytes) {  // dynamic LDS above 64 KB needs an explicit opt-in (once per kernel)
    if (bytes <= 64 * 1024) return hipSuccess;
    return allow_lds_impl(reinterpret_cast<const void *>(kernel), bytes);
}

// What one workgroup may really ask for: the runtime does not grant a CU's full 160 KiB (163 232 B launched, 163 616 B did not:
// tools/lds_limit_probe.py, round 5) -- 1 KiB of headroom, as brick_path_supported keeps. A table that does not fit drops to the
// next tier instead of failing at launch (R = 3409 .. 3413 and 10 227 .. 10 240 picked a tier the launch refused).
constexpr size_t LDS_PER_CU = 159 * 1024;

}  // namespace dr
