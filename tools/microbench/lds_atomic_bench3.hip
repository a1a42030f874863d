// lds_atomic_bench3.hip -- ds_add_u64: do duplicate addresses cost the same when the lanes that share one sit in
// DIFFERENT 16-lane rows of the wave (pattern B) as when they are neighbours (pattern A)?
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
__global__ __launch_bounds__(256) void k(float *out, int iters, int pattern, int mult) {
    __shared__ unsigned long long box[4096];
    for (int i = threadIdx.x; i < 4096; i += 256) box[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // mult lanes share an address: A = neighbours (lane / mult), B = lanes a whole row apart (lane % (64 / mult))
    const int grp = pattern == 0 ? lane / mult : lane % (64 / mult);
    int a = ((grp * 19) + w * 1024) & 4095;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 8; ++r) atomicAdd(&box[(a + r * 37) & 4095], (unsigned long long)lane + 1ull);
        a = (a + 5) & 4095;
    }
    __syncthreads();
    unsigned long long s = 0; for (int i = threadIdx.x; i < 4096; i += 256) s += box[i];
    out[blockIdx.x * 256 + threadIdx.x] = (float)s;
}
// ---- rows A and B (profiles/rowscatter_microbench.txt): the d_volume scatter of B1 from a row-transposed lane layout ----
// One "pass" = what one wave of B1 does per 64 samples for d_volume: 20 ds_add_u64 into a 15 x 15 x 15 box with B1's strides
// (8 corners of the centre cell, 3 outside planes of 4), after NPERM ds_bpermute_b32 that bring the scatter's inputs from
// lane 4 (l % 16) + l / 16 (the first of them carries the cell, so the adds wait for it as they would in the kernel).
//   layout 0: one lane per cell (conflict-free reference: row A, the cost of the bpermutes between the adds)
//   layout 1: lanes are consecutive samples of a ray, ~3.5 per cell, two 32-sample segments per pass (B1 today)
//   layout 2: the same samples, lane 16 r + c scatters sample 4 c + r
constexpr int MB_SY = 15, MB_SX = 15 * 15 + 12, MB_N = 15 * MB_SX;
__device__ __forceinline__ int cell_of_sample(int layout, int s, int w, float phase) {
    if (layout == 0) return MB_SX + MB_SY + 1 + (s & 7) * MB_SX + ((s >> 3) & 7) * MB_SY + ((w + (int)(phase * 8.0f)) & 7);
    const int ray = s >> 5, k = s & 31;
    const float x = 1.0f + phase + (float)k * (1.0f / 3.5f), y = 1.3f + (float)ray + (float)(w & 3) * 2.0f + (float)k * 0.11f,
                z = 1.6f + (float)(w >> 2) * 0.5f + (float)k * 0.07f + phase;
    return (int)x * MB_SX + (int)y * MB_SY + (int)z;
}
template <int NPERM>
__global__ __launch_bounds__(256) void k_row(float *out, int iters, int layout) {
    __shared__ unsigned long long box[MB_N];
    for (int i = threadIdx.x; i < MB_N; i += 256) box[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = (threadIdx.x >> 6) + 4 * (blockIdx.x & 1);
    const int src = layout == 2 ? 4 * (lane & 15) + (lane >> 4) : lane;
    float v = 1.0f + (float)lane;
    for (int it = 0; it < iters; ++it) {
        const float phase = (float)(it & 7) * 0.137f;
        int cb;
        unsigned int addend = (unsigned int)lane + 1u;
        if (NPERM > 0) {
            cb = __builtin_amdgcn_ds_bpermute(4 * src, cell_of_sample(layout, lane, w, phase));
#pragma unroll
            for (int p = 1; p < NPERM; ++p) addend += (unsigned int)__builtin_amdgcn_ds_bpermute(4 * src, __float_as_int(v * (float)(p + it)));
        } else {
            cb = cell_of_sample(layout, src, w, phase);
        }
        const bool hi = (cb + it) & 1;   // which outside plane a sample's +-delta taps reach depends on its fractions
        unsigned long long *d = box + cb;
        const unsigned long long a = addend;
#pragma unroll
        for (int q = 0; q < 8; ++q) atomicAdd(d + (q & 1) * MB_SX + ((q >> 1) & 1) * MB_SY + (q >> 2), a + q);
        unsigned long long *px = d + (hi ? 2 * MB_SX : -MB_SX), *py = d + (hi ? -MB_SY : 2 * MB_SY), *pz = d + (hi ? 2 : -1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            atomicAdd(px + (q & 1) * MB_SY + (q >> 1), a + q);
            atomicAdd(py + (q & 1) * MB_SX + (q >> 1), a + q);
            atomicAdd(pz + (q & 1) * MB_SX + (q >> 1) * MB_SY, a + q);
        }
    }
    __syncthreads();
    unsigned long long s = 0; for (int i = threadIdx.x; i < MB_N; i += 256) s += box[i];
    out[blockIdx.x * 256 + threadIdx.x] = (float)s;
}
template <int NPERM>
static double row_pass_cycles(float *out, int blocks, int iters, int layout, int CUs, double clk, hipEvent_t e0, hipEvent_t e1) {
    auto launch = [&] { hipLaunchKernelGGL(k_row<NPERM>, dim3(blocks), dim3(256), 0, 0, out, iters, layout); };
    launch(); CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e-3 * clk * CUs / ((double)blocks * 4 * iters);
}
int main() {
    float *out; CK(hipMalloc(&out, 256 * 8 * 256 * 4));
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int CUs = prop.multiProcessorCount; const double clk = prop.clockRate * 1e3;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 2048, blocks = CUs * 4;
    for (int mult : {1, 2, 4}) for (int pattern : {0, 1}) {
        auto launch = [&] { hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, iters, pattern, mult); };
        launch(); CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%d lanes per address, %s: %7.1f cyc/CU per ds_add_u64\n", mult, pattern ? "a row or more apart (lane %% (64/m))" : "neighbouring lanes (lane / m)",
               ms * 1e-3 * clk * CUs / ((double)blocks * 4 * iters * 8));
    }
    {
        const char *names[3] = {"one lane per cell", "lane order (3.5 neighbouring lanes per cell)", "row-transposed (lane 16r+c <- sample 4c+r)"};
        double c[3][3];
        for (int layout = 0; layout < 3; ++layout) {
            c[layout][0] = row_pass_cycles<0>(out, blocks, 1024, layout, CUs, clk, e0, e1);
            c[layout][1] = row_pass_cycles<8>(out, blocks, 1024, layout, CUs, clk, e0, e1);
            c[layout][2] = row_pass_cycles<14>(out, blocks, 1024, layout, CUs, clk, e0, e1);
        }
        printf("row A: ds_bpermute_b32 between groups of 20 ds_add_u64 (one lane per cell), cyc/CU per wave-instruction: "
               "%.1f in groups of 8, %.1f in groups of 14 (the 20 adds alone: %.1f per pass)\n",
               (c[0][1] - c[0][0]) / 8.0, (c[0][2] - c[0][0]) / 14.0, c[0][0]);
        printf("row B: cyc/CU per pass of 20 ds_add_u64 with 0 / 8 / 14 ds_bpermute_b32 in front\n");
        for (int layout = 0; layout < 3; ++layout) printf("  %-46s %7.1f %7.1f %7.1f\n", names[layout], c[layout][0], c[layout][1], c[layout][2]);
    }
    return 0;
}
