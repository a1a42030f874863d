// dr_depth.h -- what the depth kernels (march_depth.hip, march_depth_bundle.hip) share: the distance of a sample along its ray,
// the composite of the moments, the sample count of a ray, the two adjoint expressions of a composited sample and the per-cell
// d_vol accumulation of the bundle backward.
#pragma once
#include "dr_tile.h"

namespace dr {

// t_s = mix(t0, exit, s/(n-1)): sample_pos's own statements (the same bits as the t it multiplies the direction with)
__device__ __forceinline__ float sample_t(const RayGeom &rg, int s, float &f) {
    f = (float)s / (float)(rg.n - 1);
    return mixf(rg.t0, rg.exit_, f);
}

// Composite (dr_device.h) for the moments: the same fma shape, A the same statement
struct CompositeDepth {
    float M1 = 0.f, M2 = 0.f, A = 0.f;
    // composites one sample at distance t; returns T = 1 - A in front of it
    __device__ __forceinline__ float add(float t, float op) {
        const float T = 1.0f - A;
        M1 = fmaf(T, t * op, M1);
        M2 = fmaf(T, (t * t) * op, M2);
        A = fmaf(T, op, A);
        return T;
    }
    __device__ __forceinline__ float4 pixel() const { return make_float4(M1, M2, 0.0f, A); }
    // what the samples after this prefix contribute to the loss, over the three live channels (go.z is never read)
    __device__ __forceinline__ float suffix(float4 go, float4 of) const {
        return (go.x * (of.x - M1) + go.y * (of.y - M2)) + go.w * (of.w - A);
    }
};

// samples of a ray (n <= 1: none, H6)
__device__ __forceinline__ int depth_samples(int n, int S) { return n > 1 ? (n < S ? n : S) : 0; }

// The adjoint of one composited sample: op_bar = T q - suffix / (1 - op) (0 suffix for the last live sample), q = g.x t + g.y t^2
// + g.w, and a_bar = op_bar d op / d a in sample_adjoint's expression. The colour adjoints are 0.
__device__ __forceinline__ float depth_alpha_adjoint(const Sample &sm, float t, float T, float suffix, bool last, float4 go,
                                                     float inv_sr) {
    const float qs = (go.x * t + go.y * (t * t)) + go.w;
    const float op_bar = T * qs - (last ? 0.0f : suffix / (1.0f - sm.op));
    return op_bar * ((inv_sr == 1.0f) ? 1.0f : inv_sr * powf(1.0f - sm.a, inv_sr - 1.0f));
}
// ... and of its intensity tap, from the alpha slope of the two texels (intensity_adjoint with r_bar = g_bar = b_bar = 0)
__device__ __forceinline__ float depth_intensity_adjoint(const Sample &sm, float a0, float a1, float a_bar, float tf_len) {
    return (0.0f < sm.xtf) ? ((a1 - a0) * a_bar) * tf_len : 0.0f;
}

// d_vol contributions of a run of consecutive live samples of one ray in one cell: eight corner sums in f32, sent as eight
// atomics when the ray leaves the cell -- dr_rgba.h's VoxelRun for the one tap of a scalar volume. At sampling rate 1 a step
// is 1 / (2 sqrt 3) of a voxel edge on a cubic volume, so a ray spends 2 - 3.5 samples in a cell.
struct VoxelRun1 {
    int x0 = -1, y0 = -1, z0 = -1;
    float s[8];   // corners in tri_scatter_global's order: (x0,y0,z0) (x1,y0,z0) (x0,y1,z0) (x1,y1,z0), then z1
    __device__ __forceinline__ bool same(const Cell &c) const { return c.x0 == x0 && c.y0 == y0 && c.z0 == z0; }
    __device__ __forceinline__ void start(const Cell &c) {
        x0 = c.x0; y0 = c.y0; z0 = c.z0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = 0.0f;
    }
    // (tri_scatter_global's weights and its order of products: a run of one sample sends that function's eight addends)
    __device__ __forceinline__ void add(const Cell &c, float adj) {
        const float gx = 1.0f - c.fx, gy = 1.0f - c.fy, gz = 1.0f - c.fz;
        s[0] += gx * gy * gz * adj;
        s[1] += c.fx * gy * gz * adj;
        s[2] += gx * c.fy * gz * adj;
        s[3] += c.fx * c.fy * gz * adj;
        s[4] += gx * gy * c.fz * adj;
        s[5] += c.fx * gy * c.fz * adj;
        s[6] += gx * c.fy * c.fz * adj;
        s[7] += c.fx * c.fy * c.fz * adj;
    }
    // (the high indices as tri_cell clamps them)
    __device__ __forceinline__ void flush(const GradView &g, int VX, int VY, int VZ) const {
        if (x0 < 0) return;
        const int x1 = min(x0 + 1, VX - 1), y1 = min(y0 + 1, VY - 1), z1 = min(z0 + 1, VZ - 1);
        float *b00 = g.p + x0 * g.sx + y0 * g.sy, *b10 = g.p + x1 * g.sx + y0 * g.sy;
        float *b01 = g.p + x0 * g.sx + y1 * g.sy, *b11 = g.p + x1 * g.sx + y1 * g.sy;
        const int64_t o0 = z0 * g.sz, o1 = z1 * g.sz;
        unsafeAtomicAdd(b00 + o0, s[0]); unsafeAtomicAdd(b10 + o0, s[1]);
        unsafeAtomicAdd(b01 + o0, s[2]); unsafeAtomicAdd(b11 + o0, s[3]);
        unsafeAtomicAdd(b00 + o1, s[4]); unsafeAtomicAdd(b10 + o1, s[5]);
        unsafeAtomicAdd(b01 + o1, s[6]); unsafeAtomicAdd(b11 + o1, s[7]);
    }
};

}  // namespace dr
