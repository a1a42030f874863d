// lds_dtf_bench.hip -- the gate of B1's d_tf adds (profiles/dtfrows_microbench.txt): what does one pass of 64 samples cost a CU
// for d_tf, at B1's shape (8 waves per workgroup, 2 workgroups per CU), when
//   (a) the runs of samples between the same two texels are summed across lanes (seg_scan_sum<4>, as B1 does) and the run-end
//       lanes issue 8 ds_add_f64 into the [texel][4] table,
//   (b) the same into a component-major [4][R] table,
//   (c) six ds_bpermute_b32 bring every sample to lane 16 r + c <- 4 c + r (dr_wave.h: row_transpose) and ALL valid lanes add
//       their own eight products, into either table?
// Texel sequences: mean run length 1 / 1.7 / 4 / 16 / 64, monotone along the ray or turning back in the middle of a segment
// (samples far apart share a texel), two 32-sample segments per pass (one for run length 64), R = 256.
// B1 is bound by VALU issue, not by the LDS: every row is measured twice, alone and among FILL independent v_fma_f32 per pass
// (the rest of B1's sample, ~1000 lane-instructions) -- the second column is what a pass costs the kernel.
//   build: hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -ffp-contract=off -I differender_amd/csrc tools/microbench/lds_dtf_bench.hip -o tools/microbench/lds_dtf_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "dr_wave.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
using namespace dr;

constexpr int R = 256, NT = 512;
constexpr float LIM = 1.0e30f;
constexpr int PAD_BYTES = 56 * 1024;   // with the 8 KB table: two workgroups per CU, as B1's 67 KB

enum { M_NONE = 0, M_SCAN = 1, M_DIRECT = 2 };

template <int CM> __device__ __forceinline__ int tab_idx(int k, int q) { return CM ? q * R + k : 4 * k + q; }
__device__ __forceinline__ void add_f64(double *p, float x) { atomicAdd(p, (double)x); }
__device__ __forceinline__ float sanit(float x) { return (x == x) ? fminf(fmaxf(x, -LIM), LIM) : 0.0f; }

// the texel below sample s (0..63) of the pass
__device__ __forceinline__ int texel_of(int s, int nseg, int turn, float inv_len, float phase, int w) {
    const int seg = nseg == 2 ? s >> 5 : 0, k = nseg == 2 ? s & 31 : s, half = nseg == 2 ? 16 : 32;
    const int u = turn ? (k < half ? k : 2 * half - 1 - k) : k;
    return ((int)(phase + (float)u * inv_len) + 29 * w + 7 * seg) & (R - 1);
}

template <int MODE, int CM, int FILL>
__global__ __launch_bounds__(NT) void k_dtf(float *out, int iters, int nseg, int turn, float inv_len) {
    __shared__ double tab[4 * R];
    extern __shared__ unsigned char pad[];
    for (int i = threadIdx.x; i < 4 * R; i += NT) tab[i] = 0.0;
    if (iters < 0) pad[threadIdx.x] = 0;   // (never: keeps the dynamic allocation referenced)
    __syncthreads();
    const int lane = threadIdx.x & 63, w = (threadIdx.x >> 6) + 8 * (blockIdx.x & 1);
    const int sl = nseg == 2 ? (lane & 32) : 0;
    float f0 = 1.0f + (float)lane, f1 = 0.5f, f2 = 0.25f, f3 = 2.0f;
    for (int it = 0; it < iters; ++it) {
        const float phase = (float)(it & 15) * 0.237f;
        const int lo = texel_of(lane, nseg, turn, inv_len, phase, w), hi = min(lo + 1, R - 1);
        const bool valid = true;
        const float fr = 0.25f + 0.5f * (float)((lane + it) & 1), Lop = 1.0f + (float)(it & 3), a_bar = 0.5f * (float)((lane ^ it) & 7);
        const float gox = 1.0f + (float)(w & 3), goy = 0.5f, goz = 2.0f - (float)(sl >> 5);
        if (FILL > 0) {   // independent full-rate VALU work around the d_tf block
#pragma unroll
            for (int i = 0; i < FILL / 4; ++i) {
                f0 = fmaf(f0, 0.999f, a_bar); f1 = fmaf(f1, 0.998f, fr); f2 = fmaf(f2, 0.997f, Lop); f3 = fmaf(f3, 0.996f, fr);
            }
        }
        if (MODE == M_SCAN) {   // B1's block (march_flat.hip, "if (WANT_TF)")
            const int key = valid ? lo : -1 - lane;
            const int key_prev = wave_up1(key, key);
            const bool run_start = lane == 0 || key != key_prev || lane == sl;
            const unsigned long long starts = __ballot(run_start);
            const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
            const int rs = 63 - __clzll((long long)(starts & upto));
            const float w0 = 1.0f - fr, w1 = fr;
            float tv[4] = {w0 * Lop, w1 * Lop, w0 * a_bar, w1 * a_bar};
            seg_scan_sum<4>(tv, lane, rs);
            const bool run_end = lane == 63 || ((starts >> (lane + 1)) & 1ull);
            const bool emit = valid && run_end;
            const float v8[8] = {tv[0] * gox, tv[0] * goy, tv[0] * goz, tv[2], tv[1] * gox, tv[1] * goy, tv[1] * goz, tv[3]};
            const float vmax = ((fabsf(v8[0]) + fabsf(v8[1])) + (fabsf(v8[2]) + fabsf(v8[3]))) +
                               ((fabsf(v8[4]) + fabsf(v8[5])) + (fabsf(v8[6]) + fabsf(v8[7])));
            if (__any(emit && !(vmax <= LIM))) {
                if (emit) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { add_f64(tab + tab_idx<CM>(lo, q), sanit(v8[q])); add_f64(tab + tab_idx<CM>(hi, q), sanit(v8[4 + q])); }
                }
            } else if (emit) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { add_f64(tab + tab_idx<CM>(lo, q), v8[q]); add_f64(tab + tab_idx<CM>(hi, q), v8[4 + q]); }
            }
        } else if (MODE == M_DIRECT) {   // every lane adds the sample of lane 4 c + r
            int l = lane;
            asm volatile("" : "+v"(l));
            const int a = row_transpose_addr(l);
            const float gx = row_transpose(Lop * gox, a), gy = row_transpose(Lop * goy, a), gz = row_transpose(Lop * goz, a);
            const float ab = row_transpose(a_bar, a), f = row_transpose(fr, a);
            const int wd = row_transpose(valid ? (lo | (hi << 11) | (int)0x80000000u) : 0, a);
            const int lo2 = wd & 0x7ff, hi2 = (wd >> 11) & 0x7ff;
            const bool v2 = wd < 0;
            const float w0 = 1.0f - f;
            const float v8[8] = {w0 * gx, w0 * gy, w0 * gz, w0 * ab, f * gx, f * gy, f * gz, f * ab};
            const float vmax = ((fabsf(v8[0]) + fabsf(v8[1])) + (fabsf(v8[2]) + fabsf(v8[3]))) +
                               ((fabsf(v8[4]) + fabsf(v8[5])) + (fabsf(v8[6]) + fabsf(v8[7])));
            if (__any(v2 && !(vmax <= LIM))) {
                if (v2) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { add_f64(tab + tab_idx<CM>(lo2, q), sanit(v8[q])); add_f64(tab + tab_idx<CM>(hi2, q), sanit(v8[4 + q])); }
                }
            } else if (v2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { add_f64(tab + tab_idx<CM>(lo2, q), v8[q]); add_f64(tab + tab_idx<CM>(hi2, q), v8[4 + q]); }
            }
        } else {   // the sequence and its inputs alone: what every row pays for the harness
            f0 += (float)lo * fr + Lop * gox + a_bar * goz;
        }
    }
    __syncthreads();
    double s = 0; for (int i = threadIdx.x; i < 4 * R; i += NT) s += tab[i];
    out[blockIdx.x * NT + threadIdx.x] = (float)s + ((f0 + f1) + (f2 + f3));
}

struct Ctx { float *out; int blocks, CUs; double clk; hipEvent_t e0, e1; };
template <int MODE, int CM, int FILL>
static double pass_cycles(const Ctx &c, int nseg, int turn, float inv_len) {
    const int iters = FILL ? 256 : 1024;
    auto launch = [&] { hipLaunchKernelGGL((k_dtf<MODE, CM, FILL>), dim3(c.blocks), dim3(NT), PAD_BYTES, 0, c.out, iters, nseg, turn, inv_len); };
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dtf<MODE, CM, FILL>), hipFuncAttributeMaxDynamicSharedMemorySize, PAD_BYTES));
    launch(); CK(hipDeviceSynchronize());
    CK(hipEventRecord(c.e0)); launch(); CK(hipEventRecord(c.e1)); CK(hipEventSynchronize(c.e1));
    float ms; CK(hipEventElapsedTime(&ms, c.e0, c.e1));
    return ms * 1e-3 * c.clk * c.CUs / ((double)c.blocks * (NT / 64) * iters);
}
template <int FILL>
static void table(const Ctx &c) {
    printf("-- %s: cycles per CU and pass of 64 samples (16 waves per CU), the harness row subtracted --\n",
           FILL ? "among 1000 independent v_fma_f32 per pass (a VALU-bound kernel, as B1)" : "the d_tf block alone");
    printf("%-34s %9s | %10s %10s %10s %10s\n", "texel sequence", "harness", "(a) scan", "(b) scan", "(c) direct", "(c) direct");
    printf("%-34s %9s | %10s %10s %10s %10s\n", "", "", "[texel][4]", "[4][R]", "[texel][4]", "[4][R]");
    const struct { const char *name; float len; int nseg; } seqs[] = {{"run length 1", 1.0f, 2}, {"run length 1.7", 1.7f, 2}, {"run length 4", 4.0f, 2},
                                                                    {"run length 16", 16.0f, 2}, {"run length 64 (one run)", 0.0f, 1}};
    for (const auto &s : seqs) for (int turn = 0; turn < 2; ++turn) {
        if (s.len == 0.0f && turn) continue;
        const float inv = s.len > 0.0f ? 1.0f / s.len : 0.0f;
        const double h = pass_cycles<M_NONE, 0, FILL>(c, s.nseg, turn, inv);
        const double a = pass_cycles<M_SCAN, 0, FILL>(c, s.nseg, turn, inv), b = pass_cycles<M_SCAN, 1, FILL>(c, s.nseg, turn, inv);
        const double d0 = pass_cycles<M_DIRECT, 0, FILL>(c, s.nseg, turn, inv), d1 = pass_cycles<M_DIRECT, 1, FILL>(c, s.nseg, turn, inv);
        char name[64];
        snprintf(name, sizeof name, "%s, %s", s.name, turn ? "turning back" : "monotone");
        printf("%-34s %9.1f | %10.1f %10.1f %10.1f %10.1f\n", name, h, a - h, b - h, d0 - h, d1 - h);
    }
}
int main() {
    Ctx c;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    c.CUs = prop.multiProcessorCount; c.clk = prop.clockRate * 1e3; c.blocks = c.CUs * 2;
    CK(hipMalloc(&c.out, (size_t)c.blocks * NT * 4));
    CK(hipEventCreate(&c.e0)); CK(hipEventCreate(&c.e1));
    printf("%s, %d CUs, %.0f MHz; 8 waves per workgroup, 2 workgroups per CU, R = %d\n", prop.name, c.CUs, c.clk * 1e-6, R);
    table<0>(c);
    table<1000>(c);
    return 0;
}
