// lv_pick.h -- the per-row decision bodies of greedy / sample decoding, shared by the stand-alone row kernels of lv_eval.hip
// (lv_argmax_rows_f32, lv_sample_rows_f32) and the device-resident roll-out of lv_rollout.hip.  One definition each, so the two
// routes pick the same word from the same row bit for bit.
#pragma once
#include "lv_device.h"

// online log-sum-exp: (m, s) <- (m, s) merged with (m2, s2), s in units of exp(x - m)
__device__ __forceinline__ void lv_lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) { m = mn; s = 0.f; return; }
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

constexpr int LV_ARGMAX_NONE = 0x7fffffff;

// the order of torch.argmax on the CPU: (v, c) comes before (best, bi) when it is larger, or equal at a lower column
__device__ __forceinline__ bool lv_argmax_before(float v, int c, float best, int bi) { return v > best || (v == best && c < bi); }

// Categorical draw from softmax(x[0 .. C)) by inverse CDF with the uniform u in [0, 1): one wave (lane l of 64), two passes
// (log-sum-exp, then a blocked running sum).  With w[c] = exp(x[c] - m) and s = sum_c w[c]: the first column with w[c] > 0 whose
// inclusive running sum reaches u * s.  A column of weight zero (-inf logit, or underflow) is never returned, as torch.multinomial
// never returns an index of probability zero: when rounding leaves the f32 running sum short of u * s (u close to 1) the result is
// the LAST column with positive weight; C - 1 only if no column has positive weight.  Every lane returns the column and gets
// the row's (m, s).
__device__ __forceinline__ int lv_wave_sample_row(const float* __restrict__ x, int C, float u, int l, float& m, float& s) {
    m = -INFINITY;
    s = 0.f;
    for (int c = l; c < C; c += 64) lv_lse_merge(m, s, x[c], 1.f);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float m2 = __shfl_xor(m, d, 64), s2 = __shfl_xor(s, d, 64);
        lv_lse_merge(m, s, m2, s2);
    }
    const float target = u * s;                        // in units of exp(x - m)
    float run = 0.f;
    int found = -1;
    int last_pos = -1;                                 // highest column with positive weight seen so far: the fallback
    bool done = false;
    for (int c0 = 0; c0 < C && !done; c0 += 64) {      // blocks of 64 consecutive columns, inclusive scan inside the wave
        const int c = c0 + l;
        float p = c < C ? expf(x[c] - m) : 0.f;
        float sc = p;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(sc, d, 64);
            if (l >= d) sc += o;
        }
        const bool hit = p > 0.f && run + sc >= target;      // p > 0 implies c < C
        // lowest lane that hit, highest lane with positive weight
        int first = hit ? l : 64;
        int pos = p > 0.f ? c : -1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(first, d, 64);
            first = o < first ? o : first;
            const int q = __shfl_xor(pos, d, 64);
            pos = q > pos ? q : pos;
        }
        if (first < 64) { found = c0 + first; done = true; }
        last_pos = pos > last_pos ? pos : last_pos;
        run += __shfl(sc, 63, 64);
    }
    return found >= 0 ? found : (last_pos >= 0 ? last_pos : C - 1);
}
