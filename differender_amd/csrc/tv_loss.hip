// tv_loss.hip -- 3-D total variation of a volume and its gradient, fused, gfx950. The definition is the torch
// code differender_amd.utils.losses.tv3d: forward differences along the last three axes with the last slice repeated (the
// difference at the far edge is exactly 0), per voxel |dD| + |dH| + |dW| (L1), sqrt(dD^2 + dH^2 + dW^2 + eps^2) (ISO) or
// dD^2 + dH^2 + dW^2 (SQ), summed. The terms are symmetric in the three axes, so the host orders them by stride: x (the
// smallest stride) runs across lanes, y across the rows of a tile, z is marched.
//
// Tile: 64 x 16 voxels of the (x, y) plane, 256 threads, 4 consecutive x voxels per thread (one 16-B / 8-B load when x is
// the stride-1 axis and the rows are aligned). A workgroup marches a chunk of z, keeping the next slice (and a prefetched one)
// in registers; each slice goes to LDS with a one-voxel halo so the in-plane neighbours are LDS reads and every voxel is read
// from HBM about once. Halo roles (threads 0-65): the row above (y0-1) and below (y0+16), the column left (x0-1) and right
// (x0+64), the latter two one voxel longer for the corners the isotropic norm reaches.
//
// Forward: f32 per lane per slice, f64 per lane across slices, f64 per workgroup, one f64 atomic per workgroup into *sum.
// Backward, gather form, no atomics: with the flux f_a(p) = sign(d_a), d_a * (1 / r) or 2 d_a,
//   g(p) = scale * up * ( f_x(p-e_x) + f_y(p-e_y) + f_z(p-e_z) - (f_x(p) + f_y(p) + f_z(p)) ),   f(p - e_a) = 0 off the volume.
// Each slice's fluxes are computed once, for the tile and the low halo (x0-1, y0-1), into LDS; f_z(p - e_z) is the thread's own
// flux of the previous slice (a chunk starts one slice early for it). Each gradient element is written once by one fixed
// sequence of operations: the gradient is bitwise deterministic.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "dr_kernels.h"
#include "../../include/differender_hip.h"

namespace dr {

namespace {

constexpr int NT = 256, VX = 4, TX = 64, TY = 16;   // threads, voxels per thread along x, tile
constexpr int VP = 72;                              // LDS row pitch (floats): col c holds x = x0 + c - 4
constexpr int VROWS = TY + 2;                       // LDS row r holds y = y0 + r - 1
constexpr int TARGET_BLOCKS = 2048, ZMIN = 16;      // z chunking: about 8 workgroups per CU, at least 16 slices each

struct TVParams {
    const void *vol;
    float *grad;
    int64_t sb, sx, sy, sz;      // element strides of the volume, axes reordered (x fastest)
    int64_t gb, gx, gy, gz;      // ... of the gradient, same order
    int NB, NX, NY, NZ;
    int tiles_x, tiles_y, zc, nchunks;
    float eps2, scale;
    const float *up;             // backward: d objective / d sum on the device, null = 1
    int accumulate;
    double *sum;                 // forward
};

struct V4 { float v[VX]; };

__device__ __forceinline__ float ld1(const float *p) { return *p; }
__device__ __forceinline__ float ld1(const __half *p) { return __half2float(*p); }

// x-vector of 4 voxels at element `base` (stride sx): one vector load when VEC and all 4 are in range, else n scalar loads
// (the rest 0). VEC guarantees sx == 1 and a base aligned to 4 elements (host check).
template <bool VEC>
__device__ __forceinline__ V4 load4(const float *p, int64_t base, int64_t sx, int n) {
    V4 r;
    if (VEC && n == VX) {
        const float4 q = *reinterpret_cast<const float4 *>(p + base);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
        return r;
    }
#pragma unroll
    for (int i = 0; i < VX; ++i) r.v[i] = i < n ? ld1(p + base + i * sx) : 0.0f;
    return r;
}
template <bool VEC>
__device__ __forceinline__ V4 load4(const __half *p, int64_t base, int64_t sx, int n) {
    V4 r;
    if (VEC && n == VX) {
        const uint2 q = *reinterpret_cast<const uint2 *>(p + base);   // half is not auto-vectorised: one 8-B load
        r.v[0] = __half2float(__ushort_as_half((unsigned short)(q.x & 0xffffu)));
        r.v[1] = __half2float(__ushort_as_half((unsigned short)(q.x >> 16)));
        r.v[2] = __half2float(__ushort_as_half((unsigned short)(q.y & 0xffffu)));
        r.v[3] = __half2float(__ushort_as_half((unsigned short)(q.y >> 16)));
        return r;
    }
#pragma unroll
    for (int i = 0; i < VX; ++i) r.v[i] = i < n ? ld1(p + base + i * sx) : 0.0f;
    return r;
}

template <int NORM>
__device__ __forceinline__ float term(float dx, float dy, float dz, float eps2) {
    if (NORM == DR_TV_L1) return fabsf(dx) + fabsf(dy) + fabsf(dz);
    if (NORM == DR_TV_SQ) return dx * dx + dy * dy + dz * dz;
    return sqrtf(dx * dx + dy * dy + dz * dz + eps2);
}

__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }   // torch: sign(0) = 0

template <int NORM>
__device__ __forceinline__ void flux(float dx, float dy, float dz, float eps2, float &fx, float &fy, float &fz) {
    if (NORM == DR_TV_L1) {
        fx = sgn(dx); fy = sgn(dy); fz = sgn(dz);
    } else if (NORM == DR_TV_SQ) {
        fx = 2.0f * dx; fy = 2.0f * dy; fz = 2.0f * dz;
    } else {
        const float ri = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz + eps2);   // one division instead of three
        fx = dx * ri; fy = dy * ri; fz = dz * ri;
    }
}

// One workgroup's place: tile origin (x0, y0), its chunk [z0, z1) and volume b.
struct Place { int x0, y0, z0, z1, b; };
__device__ __forceinline__ Place place(const TVParams &P) {
    int t = blockIdx.x;
    Place w;
    w.x0 = (t % P.tiles_x) * TX; t /= P.tiles_x;
    w.y0 = (t % P.tiles_y) * TY; t /= P.tiles_y;
    w.z0 = (t % P.nchunks) * P.zc; w.b = t / P.nchunks;
    w.z1 = min(w.z0 + P.zc, P.NZ);
    return w;
}

// The halo role of threads 0..65: a 4-voxel piece of row y0-1 (R0) or y0+16 (R1), or one voxel of column x0-1 at rows
// y0..y0+16 (C0) or of column x0+64 at rows y0-1..y0+15 (C1). R0 and C0 (except C0's corner) are flux owners in the backward;
// the forward needs only R1 and C1's rows y0..y0+15.
struct Role { int64_t base; int n, lds, j, kind; };   // kind 0 R0, 1 R1, 2 C0, 3 C1, 4 none
__device__ __forceinline__ Role role(const TVParams &P, const Place &w, int tid, bool bwd) {
    Role h; h.kind = 4; h.j = 0; h.lds = 0; h.n = 0; h.base = 0;
    int hx = 0, hy = 0, width = 1;
    bool on = false;
    if (tid < 16) { h.kind = 0; h.j = tid; hx = w.x0 + VX * tid; hy = w.y0 - 1; width = VX; h.lds = 4 + VX * tid; on = bwd; }
    else if (tid < 32) { h.kind = 1; h.j = tid - 16; hx = w.x0 + VX * h.j; hy = w.y0 + TY; width = VX; h.lds = (TY + 1) * VP + 4 + VX * h.j; on = true; }
    else if (tid < 49) { h.kind = 2; h.j = tid - 32; hx = w.x0 - 1; hy = w.y0 + h.j; h.lds = (1 + h.j) * VP + 3; on = bwd; }
    else if (tid < 66) { h.kind = 3; h.j = tid - 49; hx = w.x0 + TX; hy = w.y0 - 1 + h.j; h.lds = h.j * VP + 4 + TX; on = bwd || h.j > 0; }
    if (on && hx >= 0 && hx < P.NX && hy >= 0 && hy < P.NY) {
        h.n = min(width, P.NX - hx);
        h.base = (int64_t)w.b * P.sb + (int64_t)hx * P.sx + (int64_t)hy * P.sy;
    }
    return h;
}

__device__ __forceinline__ void put_role(float *B, const Role &h, const V4 &v) {
    if (h.kind == 0 || h.kind == 1) *reinterpret_cast<float4 *>(B + h.lds) = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
    else if (h.kind < 4) B[h.lds] = v.v[0];
}

template <typename T, bool VEC, int NORM>
__global__ __launch_bounds__(NT) void tv3d_fwd_kernel(TVParams P) {
    __shared__ __attribute__((aligned(16))) float lds[2 * VROWS * VP];
    __shared__ double wsum[NT / 64];
    const T *vol = static_cast<const T *>(P.vol);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const Place w = place(P);
    const int x = w.x0 + VX * tx, y = w.y0 + ty;
    const int nown = y < P.NY ? max(0, min(VX, P.NX - x)) : 0;
    const int64_t own = nown ? (int64_t)w.b * P.sb + (int64_t)x * P.sx + (int64_t)y * P.sy : 0;
    const Role h = role(P, w, tid, false);
    const int zl = min(w.z1, P.NZ - 1);   // last slice read (the differences of slice z1-1 need z1)
    const int oc = (ty + 1) * VP + 4 + VX * tx;

    V4 cur = load4<VEC>(vol, own + w.z0 * P.sz, P.sx, nown);
    V4 nxt = w.z0 + 1 <= zl ? load4<VEC>(vol, own + (w.z0 + 1) * P.sz, P.sx, nown) : cur;
    V4 hcur = load4<VEC>(vol, h.base + w.z0 * P.sz, P.sx, h.n);
    double acc = 0.0;
    for (int z = w.z0; z < w.z1; ++z) {
        const bool more = z + 1 < w.z1;
        V4 pre = nxt, hnxt = hcur;
        if (z + 2 <= zl) pre = load4<VEC>(vol, own + (int64_t)(z + 2) * P.sz, P.sx, nown);
        if (more) hnxt = load4<VEC>(vol, h.base + (int64_t)(z + 1) * P.sz, P.sx, h.n);
        float *B = lds + (z & 1) * VROWS * VP;
        *reinterpret_cast<float4 *>(B + oc) = make_float4(cur.v[0], cur.v[1], cur.v[2], cur.v[3]);
        put_role(B, h, hcur);
        __syncthreads();
        const float4 dn = *reinterpret_cast<const float4 *>(B + oc + VP);
        const float down[VX] = {dn.x, dn.y, dn.z, dn.w};
        const float right = B[oc + VX];
        const bool zin = z + 1 < P.NZ, yin = y + 1 < P.NY;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < VX; ++i) {
            const float v = cur.v[i];
            const float vr = x + i + 1 < P.NX ? (i + 1 < VX ? cur.v[i + 1] : right) : v;
            const float vd = yin ? down[i] : v;
            const float vz = zin ? nxt.v[i] : v;
            const float t = term<NORM>(vr - v, vd - v, vz - v, P.eps2);
            s += i < nown ? t : 0.0f;
        }
        acc += (double)s;
        cur = nxt; nxt = pre; hcur = hnxt;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) atomicAdd(P.sum, (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

template <typename T, bool VEC, int NORM>
__global__ __launch_bounds__(NT) void tv3d_bwd_kernel(TVParams P) {
    __shared__ __attribute__((aligned(16))) float lds[VROWS * VP + TY * VP + (TY + 1) * VP];
    float *B = lds;                          // values of slice z, rows y0-1..y0+16, cols x0-1..x0+64
    float *FX = lds + VROWS * VP;            // f_x, rows y0..y0+15, cols x0-1..x0+63
    float *FY = FX + TY * VP;                // f_y, rows y0-1..y0+15, cols x0..x0+63
    const T *vol = static_cast<const T *>(P.vol);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const Place w = place(P);
    const int x = w.x0 + VX * tx, y = w.y0 + ty;
    const int nown = y < P.NY ? max(0, min(VX, P.NX - x)) : 0;
    const int64_t own = nown ? (int64_t)w.b * P.sb + (int64_t)x * P.sx + (int64_t)y * P.sy : 0;
    const int64_t gown = nown ? (int64_t)w.b * P.gb + (int64_t)x * P.gx + (int64_t)y * P.gy : 0;
    const Role h = role(P, w, tid, true);
    const int zs = max(w.z0 - 1, 0), zl = min(w.z1, P.NZ - 1);
    const int oc = (ty + 1) * VP + 4 + VX * tx;    // this thread's voxels in B
    const int fc = ty * VP + 4 + VX * tx;          // ... in FX (row y) and FY (row y: FY row r holds y0 - 1 + r)
    const float coef = (P.up ? P.up[0] : 1.0f) * P.scale;

    V4 cur = load4<VEC>(vol, own + zs * P.sz, P.sx, nown);
    V4 nxt = zs + 1 <= zl ? load4<VEC>(vol, own + (zs + 1) * P.sz, P.sx, nown) : cur;
    V4 hcur = load4<VEC>(vol, h.base + zs * P.sz, P.sx, h.n);
    V4 hnxt = zs + 1 <= zl ? load4<VEC>(vol, h.base + (zs + 1) * P.sz, P.sx, h.n) : hcur;
    float fzp[VX] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int z = zs; z < w.z1; ++z) {
        V4 pre = nxt, hpre = hnxt;
        if (z + 2 <= zl) {
            pre = load4<VEC>(vol, own + (int64_t)(z + 2) * P.sz, P.sx, nown);
            hpre = load4<VEC>(vol, h.base + (int64_t)(z + 2) * P.sz, P.sx, h.n);
        }
        *reinterpret_cast<float4 *>(B + oc) = make_float4(cur.v[0], cur.v[1], cur.v[2], cur.v[3]);
        put_role(B, h, hcur);
        __syncthreads();
        const bool zin = z + 1 < P.NZ;
        // fluxes of this thread's voxels
        float fx[VX], fy[VX], fz[VX];
        {
            const float4 dn = *reinterpret_cast<const float4 *>(B + oc + VP);
            const float down[VX] = {dn.x, dn.y, dn.z, dn.w};
            const float right = B[oc + VX];
            const bool yin = y + 1 < P.NY;
#pragma unroll
            for (int i = 0; i < VX; ++i) {
                const float v = cur.v[i];
                const float vr = x + i + 1 < P.NX ? (i + 1 < VX ? cur.v[i + 1] : right) : v;
                const float vd = yin ? down[i] : v;
                const float vz = zin ? nxt.v[i] : v;
                flux<NORM>(vr - v, vd - v, vz - v, P.eps2, fx[i], fy[i], fz[i]);
                if (i >= nown) fx[i] = fy[i] = fz[i] = 0.0f;
            }
            *reinterpret_cast<float4 *>(FX + fc) = make_float4(fx[0], fx[1], fx[2], fx[3]);
            *reinterpret_cast<float4 *>(FY + fc + VP) = make_float4(fy[0], fy[1], fy[2], fy[3]);
        }
        // fluxes of the low halo: f_y of row y0-1 (R0), f_x of column x0-1 (C0); 0 off the volume
        if (h.kind == 0) {
            float f[VX];
#pragma unroll
            for (int i = 0; i < VX; ++i) {
                const int hx = w.x0 + VX * h.j + i;
                const float v = hcur.v[i];
                const float vr = hx + 1 < P.NX ? (i + 1 < VX ? hcur.v[i + 1] : B[VX * h.j + 4 + VX]) : v;
                const float vd = B[VP + 4 + VX * h.j + i];
                const float vz = zin ? hnxt.v[i] : v;
                float gx, gz;
                flux<NORM>(vr - v, vd - v, vz - v, P.eps2, gx, f[i], gz);
                if (i >= h.n) f[i] = 0.0f;
            }
            *reinterpret_cast<float4 *>(FY + 4 + VX * h.j) = make_float4(f[0], f[1], f[2], f[3]);
        } else if (h.kind == 2 && h.j < TY) {
            const float v = hcur.v[0];
            const float vr = B[(1 + h.j) * VP + 4];
            const float vd = w.y0 + h.j + 1 < P.NY ? B[(2 + h.j) * VP + 3] : v;
            const float vz = zin ? hnxt.v[0] : v;
            float f, gy, gz;
            flux<NORM>(vr - v, vd - v, vz - v, P.eps2, f, gy, gz);
            FX[h.j * VP + 3] = h.n ? f : 0.0f;
        }
        __syncthreads();
        if (z >= w.z0 && nown) {
            const float4 up4 = *reinterpret_cast<const float4 *>(FY + fc);
            const float fyu[VX] = {up4.x, up4.y, up4.z, up4.w};
            const float fxl0 = FX[fc - 1];
            V4 g;
#pragma unroll
            for (int i = 0; i < VX; ++i) {
                const float fxl = i ? fx[i - 1] : fxl0;
                g.v[i] = coef * (((fxl + fyu[i]) + fzp[i]) - ((fx[i] + fy[i]) + fz[i]));
            }
            const int64_t o = gown + (int64_t)z * P.gz;
            if (VEC && nown == VX) {
                float4 *q = reinterpret_cast<float4 *>(P.grad + o);
                if (P.accumulate) {
                    const float4 a = *q;
                    g.v[0] = a.x + g.v[0]; g.v[1] = a.y + g.v[1]; g.v[2] = a.z + g.v[2]; g.v[3] = a.w + g.v[3];
                }
                *q = make_float4(g.v[0], g.v[1], g.v[2], g.v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < VX; ++i) {
                    if (i < nown) {
                        float *q = P.grad + o + i * P.gx;
                        *q = P.accumulate ? *q + g.v[i] : g.v[i];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VX; ++i) fzp[i] = fz[i];
        cur = nxt; nxt = pre; hcur = hnxt; hnxt = hpre;
    }
}

using Kernel = void (*)(TVParams);

template <typename T, bool VEC>
Kernel pick_fwd(int norm) {
    if (norm == DR_TV_L1) return tv3d_fwd_kernel<T, VEC, DR_TV_L1>;
    if (norm == DR_TV_ISO) return tv3d_fwd_kernel<T, VEC, DR_TV_ISO>;
    return tv3d_fwd_kernel<T, VEC, DR_TV_SQ>;
}
template <typename T, bool VEC>
Kernel pick_bwd(int norm) {
    if (norm == DR_TV_L1) return tv3d_bwd_kernel<T, VEC, DR_TV_L1>;
    if (norm == DR_TV_ISO) return tv3d_bwd_kernel<T, VEC, DR_TV_ISO>;
    return tv3d_bwd_kernel<T, VEC, DR_TV_SQ>;
}

// An axis of extent 1 is never stepped along: its stride does not matter (for the order or for alignment).
bool aligned4(const void *p, size_t elem, const int64_t s[4], const int n[4]) {
    if ((uintptr_t)p % (VX * elem)) return false;
    for (int a = 0; a < 4; ++a)
        if (a != 1 && n[a] > 1 && s[a] % VX) return false;
    return n[1] <= 1 || s[1] == 1;
}

// Axes reordered by stride, tile and chunk counts; *vec: the 4-wide loads (and stores) are legal.
int fill_params(TVParams &P, const TVArgs &a, bool bwd, bool *vec) {
    const int ext[3] = {a.D, a.H, a.W};
    int ord[3] = {0, 1, 2};
    auto key = [&](int k) { return ext[k] > 1 ? (a.strides[1 + k] < 0 ? -a.strides[1 + k] : a.strides[1 + k]) : INT64_MAX; };
    for (int i = 1; i < 3; ++i)   // stable insertion sort on |stride|: x = smallest
        for (int j = i; j > 0 && key(ord[j]) < key(ord[j - 1]); --j) { const int t = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = t; }
    P.vol = a.vol; P.grad = a.grad;
    P.NB = a.B; P.NX = ext[ord[0]]; P.NY = ext[ord[1]]; P.NZ = ext[ord[2]];
    P.sb = a.strides[0]; P.sx = a.strides[1 + ord[0]]; P.sy = a.strides[1 + ord[1]]; P.sz = a.strides[1 + ord[2]];
    P.gb = a.grad_strides[0]; P.gx = a.grad_strides[1 + ord[0]]; P.gy = a.grad_strides[1 + ord[1]]; P.gz = a.grad_strides[1 + ord[2]];
    P.eps2 = (float)(a.eps * a.eps);
    P.scale = a.scale; P.up = a.upstream; P.accumulate = a.accumulate; P.sum = a.sum;
    P.tiles_x = (P.NX + TX - 1) / TX;
    P.tiles_y = (P.NY + TY - 1) / TY;
    const int64_t tiles = (int64_t)P.tiles_x * P.tiles_y * P.NB;
    const int64_t want = (TARGET_BLOCKS + tiles - 1) / tiles;          // chunks per column for about TARGET_BLOCKS workgroups
    int64_t zc = (P.NZ + want - 1) / want;
    zc = zc < ZMIN ? ZMIN : zc;
    P.zc = (int)(zc < P.NZ ? zc : P.NZ);
    P.nchunks = (P.NZ + P.zc - 1) / P.zc;
    if (tiles * P.nchunks > INT32_MAX) return DR_EUNSUPPORTED;
    const size_t elem = a.vol_dtype == DR_F16 ? 2 : 4;
    const int n[4] = {P.NB, P.NX, P.NY, P.NZ};
    const int64_t s[4] = {P.sb, P.sx, P.sy, P.sz}, g[4] = {P.gb, P.gx, P.gy, P.gz};
    *vec = aligned4(a.vol, elem, s, n) && (!bwd || aligned4(a.grad, sizeof(float), g, n));
    return 0;
}

int launch(const TVArgs &a, bool bwd, hipStream_t stream) {
    TVParams P;
    bool vec = false;
    int rc = fill_params(P, a, bwd, &vec);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((int64_t)P.tiles_x * P.tiles_y * P.NB * P.nchunks);
    Kernel k;
    if (a.vol_dtype == DR_F16)
        k = bwd ? (vec ? pick_bwd<__half, true>(a.norm) : pick_bwd<__half, false>(a.norm))
                : (vec ? pick_fwd<__half, true>(a.norm) : pick_fwd<__half, false>(a.norm));
    else
        k = bwd ? (vec ? pick_bwd<float, true>(a.norm) : pick_bwd<float, false>(a.norm))
                : (vec ? pick_fwd<float, true>(a.norm) : pick_fwd<float, false>(a.norm));
    if (!bwd) {
        const hipError_t e = hipMemsetAsync(a.sum, 0, sizeof(double), stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NT), 0, stream, P);
    return (int)hipGetLastError();
}

}  // namespace

int launch_tv3d_fwd(const TVArgs &a, hipStream_t stream) { return launch(a, false, stream); }
int launch_tv3d_bwd(const TVArgs &a, hipStream_t stream) { return launch(a, true, stream); }

}  // namespace dr
