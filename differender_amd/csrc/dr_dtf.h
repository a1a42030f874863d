// dr_dtf.h -- the TF-gradient blocks that the brick kernels (march_flat.hip), the tape kernel (tf_tape.hip) and the exact per-ray
// backward (ray_passes.hip) share: sums over runs of lanes with one key, the carried scan of the composite as (gC . C, A), and the
// guarded add of a finished run's sums into the [texel][4] LDS table of doubles (acc_add_f64, dr_brick_common.h).
// Every helper takes fields, no parameter struct, and is held to the device assembly of the code it replaced (tools/asm_same.sh):
// what a helper owns and what it returns, and the ORDER of its statements, matter to the compiler as much as its signature does
// ("shared TF-gradient blocks", lists what stayed at its call sites for that reason).
#pragma once
#include "dr_brick_common.h"
#include "dr_wave.h"

namespace dr {

// Sums v over every run of consecutive lanes that hold the same key, inside segments that begin at lane `sl` (0: the wave is one
// segment): v leaves as the inclusive sum from the first lane of the lane's run. Returns whether the lane is the last of its run,
// the one that holds the run's total. A lane without a value gives a key of its own (-1 - lane).
template <int NV>
__device__ __forceinline__ bool lane_run_sums(int key, int lane, int sl, float (&v)[NV]) {
    const int prev = wave_up1(key, key);
    const bool start = lane == 0 || key != prev || lane == sl;
    // first lane of this lane's run = highest run-start bit at or below the lane (lane 0 always starts one)
    const unsigned long long starts = __ballot(start);
    const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
    const int rs = 63 - __clzll((long long)(starts & upto));
    seg_scan_sum<NV>(v, lane, rs);
    return lane == 63 || ((starts >> ((lane + 1) & 63)) & 1ull);
}

// Segmented inclusive scan of the lanes' composites (segments begin at lane `sl`) into inc2; returns its exclusive copy. Where
// `cont`, the lanes of segment seg_c (seg: the lane's own) continue what the passes before left in `carry2`; it leaves as lane
// 63's inclusive composite.
__device__ __forceinline__ Over2 scan_over2_carried(const Over2 &el2, int lane, int sl, bool cont, int seg, int seg_c, Over2 &carry2, Over2 &inc2) {
    inc2 = seg_scan_over2(el2, lane, sl);
    Over2 exc2;
    exc2.w = wave_up1(inc2.w, 0.f); exc2.a = wave_up1(inc2.a, 0.f);
    if (lane == sl) { exc2.w = 0.f; exc2.a = 0.f; }
    if (cont && seg == seg_c) { inc2 = over2(carry2, inc2); exc2 = over2(carry2, exc2); }
    carry2.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc2.w), 63));
    carry2.a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc2.a), 63));
    return exc2;
}

// Adds a finished run's sums tq = (w0 L op T, w1 L op T, w0 a_bar, w1 a_bar) to the texels lo / hi of the table, on the lanes
// with `em`: (r, g, b)_bar = (L op T) go.xyz is applied to the run's total (go is constant over a run: one ray). d_tf accumulates
// in double; a NaN or an absurd run total sends the wave through the sanitising path.
__device__ __forceinline__ void dtf_run_add(unsigned long long *dtf, int lo, int hi, bool em, const float (&tq)[4], const float4 &go) {
    const float v8[8] = {tq[0] * go.x, tq[0] * go.y, tq[0] * go.z, tq[2], tq[1] * go.x, tq[1] * go.y, tq[1] * go.z, tq[3]};
    // sum of magnitudes (>= the largest one; full-rate adds, and a NaN propagates into the test)
    const float vmax = ((fabsf(v8[0]) + fabsf(v8[1])) + (fabsf(v8[2]) + fabsf(v8[3]))) +
                       ((fabsf(v8[4]) + fabsf(v8[5])) + (fabsf(v8[6]) + fabsf(v8[7])));
    unsigned long long *d0 = dtf + 4 * lo, *d1 = dtf + 4 * hi;
    if (__any(em && !(vmax <= ACC_LIM))) {
        if (em) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { acc_add_f64(d0 + q, acc_sanitise(v8[q])); acc_add_f64(d1 + q, acc_sanitise(v8[4 + q])); }
        }
    } else if (em) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc_add_f64(d0 + q, v8[q]); acc_add_f64(d1 + q, v8[4 + q]); }
    }
}

// The run sums of a pass whose lanes hold SEVERAL consecutive samples. A lane's samples form an incoming group that may continue
// the run of the lane before (`contl`: same TF cell as that lane's outgoing group, and no segment start between them), and an
// outgoing one (sums V) that is carried on to the next lane; a lane whose samples fall into different TF cells ("split") closes
// the incoming run with its first group and opens a new one with its last: start = !contl || split. Without a split both are the
// same group and V holds all of it. V leaves as the inclusive sum of the lane's outgoing run; returns whether that run ends
// here, where the caller adds V (dtf_run_add).
//   Then, under __any(split), a split lane adds the run it closed: its first group on top of (contl ? Pv : 0), Pv = wave_up1(V),
// the inclusive sum of the previous lane's outgoing run. The callers pin those DPP moves in front of the select with an empty
// asm volatile: the compiler otherwise turns `contl ? dpp : 0` into an exec-masked region around the v_mov_dpp, and a DPP move
// whose SOURCE lane is masked off writes nothing.
__device__ __forceinline__ bool dtf_split_runs(int lane, bool contl, bool start, float (&V)[4]) {
    const unsigned long long starts = __ballot(start);
    const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
    const int rs = 63 - __clzll((long long)(starts & upto));  // first lane of this lane's outgoing run (lane 0 starts one)
    seg_scan_sum<4>(V, lane, rs);
    const unsigned long long contm = __ballot(contl);
    return lane == 63 || !((contm >> ((lane + 1) & 63)) & 1ull);
}

}  // namespace dr
