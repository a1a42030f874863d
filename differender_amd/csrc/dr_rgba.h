// dr_rgba.h -- what the kernels over a pre-classified RGBA volume (march_rgba.hip, march_rgba_bundle.hip) share: the fetch of a
// voxel's four channels, the four-channel trilinear sample with and without its slopes, the per-cell d_vol accumulation, the
// sample count of a ray and the host's choice of the one-load-per-voxel path.
#pragma once
#include "dr_tile.h"

namespace dr {

struct __attribute__((aligned(8))) Half4 { unsigned short r, g, b, a; };

// the four channels of one voxel
template <bool VEC>
__device__ __forceinline__ float4 ld_voxel4(const float *p, int64_t sc) {
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[sc], p[2 * sc], p[3 * sc]);
}
template <bool VEC>
__device__ __forceinline__ float4 ld_voxel4(const __half *p, int64_t sc) {
    if (VEC) {
        const Half4 q = *reinterpret_cast<const Half4 *>(p);
        return make_float4(__half2float(__ushort_as_half(q.r)), __half2float(__ushort_as_half(q.g)),
                           __half2float(__ushort_as_half(q.b)), __half2float(__ushort_as_half(q.a)));
    }
    return make_float4(__half2float(p[0]), __half2float(p[sc]), __half2float(p[2 * sc]), __half2float(p[3 * sc]));
}

// tri_sample (dr_device.h) on four channels: one cell, eight corner fetches, the lerps x -> y -> z per channel
template <typename VT, bool VEC>
__device__ __forceinline__ float4 tri_sample4(const VolView<VT> &v, int64_t sc, const Cell &c) {
    const VT *b00 = v.p + c.x0 * v.sx + c.y0 * v.sy, *b10 = v.p + c.x1 * v.sx + c.y0 * v.sy;
    const VT *b01 = v.p + c.x0 * v.sx + c.y1 * v.sy, *b11 = v.p + c.x1 * v.sx + c.y1 * v.sy;
    const int64_t o0 = c.z0 * v.sz, o1 = c.z1 * v.sz;
    float4 a = mix4(ld_voxel4<VEC>(b00 + o0, sc), ld_voxel4<VEC>(b10 + o0, sc), c.fx);
    float4 b = mix4(ld_voxel4<VEC>(b01 + o0, sc), ld_voxel4<VEC>(b11 + o0, sc), c.fx);
    const float4 zl = mix4(a, b, c.fy);
    a = mix4(ld_voxel4<VEC>(b00 + o1, sc), ld_voxel4<VEC>(b10 + o1, sc), c.fx);
    b = mix4(ld_voxel4<VEC>(b01 + o1, sc), ld_voxel4<VEC>(b11 + o1, sc), c.fx);
    const float4 zh = mix4(a, b, c.fy);
    return mix4(zl, zh, c.fz);
}

// samples of a ray (n <= 1: none, H6); the non-differentiable march has no max_samples clip
__device__ __forceinline__ int rgba_samples(int n, int S, bool nondiff) { return n > 1 ? (nondiff || n < S ? n : S) : 0; }

// d_vol contributions of a run of consecutive live samples of one ray in one cell: 8 corners x 4 channels, summed in f32 and
// sent as 32 atomics when the ray leaves the cell (march_tf2d.hip's CellRun, on the volume). Measured against 32 atomics per
// sample (tools/patches/rgba_per_sample.patch, profiles/rgba_time.jsonl): 2.1-2.7x less time at sampling rate 1, 4.5-9.4x
// at rate 4, for 21-33 VGPRs more.
struct VoxelRun {
    int x0 = -1, y0, z0;
    float s[8][4];   // corners in tri_scatter_global's order: (x0,y0,z0) (x1,y0,z0) (x0,y1,z0) (x1,y1,z0), then z1
    __device__ __forceinline__ bool same(const Cell &c) const { return c.x0 == x0 && c.y0 == y0 && c.z0 == z0; }
    __device__ __forceinline__ void start(const Cell &c) {
        x0 = c.x0; y0 = c.y0; z0 = c.z0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[k][q] = 0.0f;
    }
    __device__ __forceinline__ void add(const Cell &c, const float adj[4]) {
        const float gx = 1.0f - c.fx, gy = 1.0f - c.fy, gz = 1.0f - c.fz;
        const float w[8] = {gx * gy * gz, c.fx * gy * gz, gx * c.fy * gz, c.fx * c.fy * gz,
                            gx * gy * c.fz, c.fx * gy * c.fz, gx * c.fy * c.fz, c.fx * c.fy * c.fz};
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[k][q] += w[k] * adj[q];
    }
    // (the high indices as tri_cell clamps them)
    __device__ __forceinline__ void flush(const GradView &g, int64_t dsc, int VX, int VY, int VZ) const {
        if (x0 < 0) return;
        const int x1 = min(x0 + 1, VX - 1), y1 = min(y0 + 1, VY - 1), z1 = min(z0 + 1, VZ - 1);
        float *b00 = g.p + x0 * g.sx + y0 * g.sy, *b10 = g.p + x1 * g.sx + y0 * g.sy;
        float *b01 = g.p + x0 * g.sx + y1 * g.sy, *b11 = g.p + x1 * g.sx + y1 * g.sy;
        const int64_t o0 = z0 * g.sz, o1 = z1 * g.sz;
        float *const corner[8] = {b00 + o0, b10 + o0, b01 + o0, b11 + o0, b00 + o1, b10 + o1, b01 + o1, b11 + o1};
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) unsafeAtomicAdd(corner[k] + q * dsc, s[k][q]);
    }
};

// tri_sample4's value (same corners, same mix4 order x -> y -> z, same bits) and, per channel, its slopes along the position's
// three axes: dr_device.h's tri_sample_grad on four channels, with its formulas and its gates -- the cell is frozen, an axis
// passes a gradient iff 0 < 0.5 p + 0.5 <= 1, and a high index clamped onto the low one gives equal corners and a zero slope.
template <typename VT, bool VEC>
__device__ __forceinline__ float4 tri_sample4_grad(const VolView<VT> &v, int64_t sc, const Cell &c, float px, float py, float pz,
                                                   float4 &gx, float4 &gy, float4 &gz) {
    const VT *b00 = v.p + c.x0 * v.sx + c.y0 * v.sy, *b10 = v.p + c.x1 * v.sx + c.y0 * v.sy;
    const VT *b01 = v.p + c.x0 * v.sx + c.y1 * v.sy, *b11 = v.p + c.x1 * v.sx + c.y1 * v.sy;
    const int64_t o0 = c.z0 * v.sz, o1 = c.z1 * v.sz;
    const float4 v000 = ld_voxel4<VEC>(b00 + o0, sc), v100 = ld_voxel4<VEC>(b10 + o0, sc);
    const float4 v010 = ld_voxel4<VEC>(b01 + o0, sc), v110 = ld_voxel4<VEC>(b11 + o0, sc);
    const float4 v001 = ld_voxel4<VEC>(b00 + o1, sc), v101 = ld_voxel4<VEC>(b10 + o1, sc);
    const float4 v011 = ld_voxel4<VEC>(b01 + o1, sc), v111 = ld_voxel4<VEC>(b11 + o1, sc);
    const float4 a0 = mix4(v000, v100, c.fx), b0 = mix4(v010, v110, c.fx);
    const float4 a1 = mix4(v001, v101, c.fx), b1 = mix4(v011, v111, c.fx);
    const float4 zl = mix4(a0, b0, c.fy), zh = mix4(a1, b1, c.fy);
    const float4 dfx = mix4(mix4(sub4(v100, v000), sub4(v110, v010), c.fy), mix4(sub4(v101, v001), sub4(v111, v011), c.fy), c.fz);
    const float4 dfy = mix4(sub4(b0, a0), sub4(b1, a1), c.fz);
    const float4 dfz = sub4(zh, zl);
    const float yx = fmaf(0.5f, px, 0.5f), yy = fmaf(0.5f, py, 0.5f), yz = fmaf(0.5f, pz, 0.5f);
    gx = (0.0f < yx && !(1.0f < yx)) ? scale4(dfx, 0.5f * v.scx) : make_float4(0.f, 0.f, 0.f, 0.f);
    gy = (0.0f < yy && !(1.0f < yy)) ? scale4(dfy, 0.5f * v.scy) : make_float4(0.f, 0.f, 0.f, 0.f);
    gz = (0.0f < yz && !(1.0f < yz)) ? scale4(dfz, 0.5f * v.scz) : make_float4(0.f, 0.f, 0.f, 0.f);
    return mix4(zl, zh, c.fz);
}

// VEC: a voxel's channels are one aligned 16-B (f32) / 8-B (f16) load wherever the voxel lies
static bool rgba_vec_ok(const MarchArgs &a, const RgbaArgs &q) {
    const size_t bytes = 4 * (a.vol_dtype == DR_F16 ? sizeof(__half) : sizeof(float));
    return q.sc == 1 && a.sx % 4 == 0 && a.sy % 4 == 0 && a.sz % 4 == 0 && a.vol_vs % 4 == 0 &&
           reinterpret_cast<uintptr_t>(a.vol) % bytes == 0;
}

}  // namespace dr
