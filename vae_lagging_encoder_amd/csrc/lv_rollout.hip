// lv_rollout.hip -- device-resident greedy and sample decoding for the LSTM decoder (reference
// modules/decoders/dec_lstm.py:270-367).
//
// The reference's loop (and LSTMDecoder._roll_out) decides on the host: per word an argmax or multinomial launch, mask algebra in
// torch and one blocking read of "is anybody still alive".  Here the state of n sentences lives in caller-owned buffers and ONE
// launch per step takes the whole decision for every row:
//
//   tok int64 [n] (next input word)   alive int32 [n]   ids int64 [n][Tmax]   len int32 [n]   score f32 [n] (running log p)
//   margin f32 [n] (greedy: smallest top-1 minus top-2 logit gap so far)   counter int32 [1] (rows still alive)
//   h, c: two [n][H] halves -- the cell reads one and writes the other, the pick moves the new state back
//
// A row that is alive appends its pick, adds (x[pick] - M) - log S to its score and dies when the pick is </s> (counter drops by
// one); a dead row keeps ids / len / score / margin / tok as they are; every row's (h, c) moves src -> dst.  A launch that finds
// counter == 0 changes nothing, so steps queued past the last sentence's end are no-ops and the result does not depend on how
// often the host looks at the counter.  (The counter can also REACH zero while a launch is running.  A workgroup that starts
// after that point owns a row that was dead on entry -- a live one would have kept the counter above zero -- and the only thing it
// skips is moving that row's state, which nothing reads any more.)
//
// The pick is lv_argmax_rows_f32's (lowest column among equal maxima) or lv_sample_rows_f32's (lv_pick.h: the same bodies).
// Nothing here allocates or synchronises.
#include "lv_device.h"
#include "lv_pick.h"

namespace {

constexpr int RO_BATCH = 8;                       // 16-byte loads a thread issues before it consumes any of them

// (h_src, c_src)[r] -> (h_dst, c_dst)[r], NT threads: loads from clamped indices in batches, then the stores
template <int NT> __device__ __forceinline__ void rollout_move_state(const float* __restrict__ h_src, const float* __restrict__ c_src,
                                                                     float* __restrict__ h_dst, float* __restrict__ c_dst, long r,
                                                                     int H, int tid) {
    const float* hs = h_src + r * H;
    const float* cs = c_src + r * H;
    float* hd = h_dst + r * H;
    float* cd = c_dst + r * H;
    for (int i0 = 0; i0 < H; i0 += 4 * NT) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * NT + tid;
            a[j] = hs[i < H ? i : H - 1];
            b[j] = cs[i < H ? i : H - 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * NT + tid;
            if (i < H) { hd[i] = a[j]; cd[i] = b[j]; }
        }
    }
}

// the bookkeeping of one live row (one thread): lp = log p(pick | row)
__device__ __forceinline__ void rollout_commit(int r, int pick, float lp, int64_t* __restrict__ tok, int* __restrict__ alive,
                                               int64_t* __restrict__ ids, int* __restrict__ len, float* __restrict__ score,
                                               int* __restrict__ counter, int t, int Tmax, int end_tok) {
    ids[(long)r * Tmax + t] = pick;
    tok[r] = pick;
    len[r] += 1;
    score[r] += lp;
    if (pick == end_tok) {
        alive[r] = 0;
        atomicAdd(counter, -1);
    }
}

// top-2 of a set as (b1, i1, b2): the argmax under lv_argmax_before and the largest value of the rest (== b1 on a tie)
__device__ __forceinline__ void top2_take(float& b1, int& i1, float& b2, float v, int c) {
    if (lv_argmax_before(v, c, b1, i1)) { b2 = b1; b1 = v; i1 = c; }
    else if (v > b2) b2 = v;
}
__device__ __forceinline__ void top2_merge(float& b1, int& i1, float& b2, float o1, int oi, float o2) {
    if (lv_argmax_before(o1, oi, b1, i1)) { b2 = fmaxf(b1, o2); b1 = o1; i1 = oi; }
    else b2 = fmaxf(b2, o1);
}

// greedy: one workgroup of 256 threads per row, ONE pass over the row.  Rows are 16-byte aligned; a thread issues RO_BATCH float4
// loads from clamped indices before it consumes any of them.  Per thread: (top-1, its column, top-2) and an online
// (m, s = sum exp(x - m)), rescaled once per batch; s is kept in double (see below).
__global__ __launch_bounds__(256) void rollout_pick_greedy_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ h_src,
                                                                  const float* __restrict__ c_src, float* __restrict__ h_dst,
                                                                  float* __restrict__ c_dst, int64_t* __restrict__ tok,
                                                                  int* __restrict__ alive, int64_t* __restrict__ ids, int* __restrict__ len,
                                                                  float* __restrict__ score, float* __restrict__ margin,
                                                                  int* __restrict__ counter, int t, int Tmax, int H, int V, int end_tok) {
    __shared__ float sb1[4], sb2[4];
    __shared__ int si1[4];
    __shared__ double ssum[4];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    if (counter[0] <= 0) return;                                    // uniform for the grid (see the note at the top)
    const int live = alive[r];
    rollout_move_state<256>(h_src, c_src, h_dst, c_dst, r, H, tid);
    if (!live) return;                                              // uniform for the workgroup
    const float4* x4 = reinterpret_cast<const float4*>(logits + (long)r * ld);
    const int n4 = (V + 3) >> 2;
    float b1 = -INFINITY, b2 = -INFINITY;
    int i1 = LV_ARGMAX_NONE;
    float m = -INFINITY;
    // s in double: the greedy pick's log-probability is -log S with S = 1 + (the rest), and a confident row has S - 1 << 1 -- an
    // f32 sum would round the rest at the magnitude of the 1 and leave log S with an absolute, not a relative, error
    double s = 0.0;
    for (int q0 = 0; q0 < n4; q0 += 256 * RO_BATCH) {
        float v[4 * RO_BATCH];
#pragma unroll
        for (int j = 0; j < RO_BATCH; ++j) {
            const int q = q0 + j * 256 + tid;
            const float4 f = x4[q < n4 ? q : n4 - 1];
            v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
        }
        float bm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4 * RO_BATCH; ++j) {
            const int c = 4 * (q0 + (j >> 2) * 256 + tid) + (j & 3);
            if (c >= V) v[j] = -INFINITY;                           // past the row (or a clamped reload): weight zero, never picked
            else top2_take(b1, i1, b2, v[j], c);
            bm = fmaxf(bm, v[j]);
        }
        if (bm > m) { s *= (double)expf(m - bm); m = bm; }
        if (m != -INFINITY) {
#pragma unroll
            for (int j = 0; j < 4 * RO_BATCH; ++j) s += (double)expf(v[j] - m);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o1 = __shfl_xor(b1, d, 64), o2 = __shfl_xor(b2, d, 64);
        const int oi = __shfl_xor(i1, d, 64);
        top2_merge(b1, i1, b2, o1, oi, o2);
    }
    if (l == 0) { sb1[w] = b1; si1[w] = i1; sb2[w] = b2; }
    __syncthreads();
    b1 = sb1[0]; i1 = si1[0]; b2 = sb2[0];
    for (int i = 1; i < 4; ++i) top2_merge(b1, i1, b2, sb1[i], si1[i], sb2[i]);
    const float M = b1;                                             // the row's maximum: every thread's sum moves to its scale
    s = m == -INFINITY ? 0.0 : s * (double)expf(m - M);
    s = lv_wave_sum(s);
    if (l == 0) ssum[w] = s;
    __syncthreads();
    if (tid == 0) {
        const double S = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        const int pick = i1 == LV_ARGMAX_NONE ? 0 : i1;
        const float xp = logits[(long)r * ld + pick];
        // (x - M) - log S, as log_softmax_rows_kernel (lv_eval.hip): x - M is rounded at the magnitude of the difference
        const float lp = (xp - M) - (float)log(S);
        margin[r] = fminf(margin[r], b1 - b2);
        rollout_commit(r, pick, lp, tok, alive, ids, len, score, counter, t, Tmax, end_tok);
    }
}

// sample: one wave per row, the draw of lv_sample_rows_f32 (lv_wave_sample_row) with its own (M, S)
__global__ __launch_bounds__(64) void rollout_pick_sample_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ u,
                                                                 const float* __restrict__ h_src, const float* __restrict__ c_src,
                                                                 float* __restrict__ h_dst, float* __restrict__ c_dst,
                                                                 int64_t* __restrict__ tok, int* __restrict__ alive,
                                                                 int64_t* __restrict__ ids, int* __restrict__ len, float* __restrict__ score,
                                                                 int* __restrict__ counter, int t, int Tmax, int H, int V, int end_tok) {
    const int r = (int)blockIdx.x, l = (int)threadIdx.x;
    if (counter[0] <= 0) return;
    const int live = alive[r];
    rollout_move_state<64>(h_src, c_src, h_dst, c_dst, r, H, l);
    if (!live) return;
    const float* x = logits + (long)r * ld;
    float M, S;
    const int pick = lv_wave_sample_row(x, V, u[r], l, M, S);
    if (l == 0) rollout_commit(r, pick, (x[pick] - M) - logf(S), tok, alive, ids, len, score, counter, t, Tmax, end_tok);
}

// filtered sample: lv_sample_filtered_rows_f32's draw (lv_block_filtered_pick), qscore the running log-probability under the
// distribution drawn from
__global__ __launch_bounds__(256) void rollout_pick_filtered_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ u,
                                                                    float inv_temp, int top_k, float top_p, const float* __restrict__ h_src,
                                                                    const float* __restrict__ c_src, float* __restrict__ h_dst,
                                                                    float* __restrict__ c_dst, int64_t* __restrict__ tok,
                                                                    int* __restrict__ alive, int64_t* __restrict__ ids, int* __restrict__ len,
                                                                    float* __restrict__ score, float* __restrict__ qscore,
                                                                    int* __restrict__ counter, int t, int Tmax, int H, int V, int end_tok) {
    __shared__ LvFilteredShared sh;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (counter[0] <= 0) return;                                    // uniform for the grid (see the note at the top)
    const int live = alive[r];
    rollout_move_state<256>(h_src, c_src, h_dst, c_dst, r, H, tid);
    if (!live) return;                                              // uniform for the workgroup
    const LvFilteredPick p = lv_block_filtered_pick(logits + (long)r * ld, V, u[r], inv_temp, top_k, top_p, tid, sh);
    if (tid == 0) {
        qscore[r] += p.lq;
        rollout_commit(r, p.pick, p.lp, tok, alive, ids, len, score, counter, t, Tmax, end_tok);
    }
}

__global__ __launch_bounds__(256) void rollout_init_kernel(const float* __restrict__ h0, const float* __restrict__ c0, float* __restrict__ h,
                                                           float* __restrict__ c, int64_t* __restrict__ tok, int* __restrict__ alive,
                                                           int* __restrict__ len, float* __restrict__ score, float* __restrict__ margin,
                                                           int* __restrict__ counter, int n, int H, int start_tok) {
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    rollout_move_state<256>(h0, c0, h, c, r, H, tid);
    if (tid == 0) {
        tok[r] = start_tok;
        alive[r] = 1;
        len[r] = 0;
        score[r] = 0.f;
        margin[r] = INFINITY;
        if (r == 0) counter[0] = n;
    }
}

}  // namespace

// Start state of n rows: tok = <s>, alive = 1, len = 0, score = 0, margin = +inf, counter[0] = n, (h0, c0) [n][H] copied into
// (h, c): the half the first step's cell reads.
extern "C" int lv_rollout_init_f32(const float* h0, const float* c0, float* h, float* c, int64_t* tok, int* alive, int* len, float* score,
                                   float* margin, int* counter, int n, int H, int V, int start_tok, void* stream) {
    if (!h0 || !c0 || !h || !c || !tok || !alive || !len || !score || !margin || !counter) return LV_ERR_ARG;
    if (h0 == h || c0 == c) return LV_ERR_ARG;
    if (n <= 0 || H <= 0 || V <= 0 || start_tok < 0 || start_tok >= V) return LV_ERR_SHAPE;
    LV_LAUNCH(rollout_init_kernel, dim3((unsigned)n), dim3(256), 0, stream, h0, c0, h, c, tok, alive, len, score, margin, counter, n, H,
              start_tok);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// Step t (0-based, < Tmax) for all n rows in one launch: the pick from logits [n][ld] -- argmax when u == NULL (greedy; rows must
// be 16-byte aligned: LV_ERR_ALIGN otherwise), else the inverse-CDF draw with u [n] -- and the bookkeeping described at the top
// of this file.  (h_src, c_src) -> (h_dst, c_dst) must be different halves.  margin may be NULL when u is given.
extern "C" int lv_rollout_pick_f32(const float* logits, long ld, const float* u, const float* h_src, const float* c_src, float* h_dst,
                                   float* c_dst, int64_t* tok, int* alive, int64_t* ids, int* len, float* score, float* margin,
                                   int* counter, int t, int Tmax, int n, int H, int V, int end_tok, void* stream) {
    if (!logits || !h_src || !c_src || !h_dst || !c_dst || !tok || !alive || !ids || !len || !score || !counter) return LV_ERR_ARG;
    if (!u && !margin) return LV_ERR_ARG;
    if (h_src == h_dst || c_src == c_dst) return LV_ERR_ARG;
    if (n <= 0 || H <= 0 || V <= 0 || ld < V || Tmax <= 0 || t < 0 || t >= Tmax || end_tok < 0 || end_tok >= V) return LV_ERR_SHAPE;
    if (u) {
        LV_LAUNCH(rollout_pick_sample_kernel, dim3((unsigned)n), dim3(64), 0, stream, logits, ld, u, h_src, c_src, h_dst, c_dst, tok, alive,
                  ids, len, score, counter, t, Tmax, H, V, end_tok);
    } else {
        if ((((uintptr_t)logits) & 15) || (ld & 3)) return LV_ERR_ALIGN;
        LV_LAUNCH(rollout_pick_greedy_kernel, dim3((unsigned)n), dim3(256), 0, stream, logits, ld, h_src, c_src, h_dst, c_dst, tok, alive, ids,
                  len, score, margin, counter, t, Tmax, H, V, end_tok);
    }
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_rollout_pick_f32's step with the draw of lv_sample_filtered_rows_f32 (u [n] mandatory; rows 16-byte aligned): the same
// bookkeeping, counter gate and dead-row rules, and qscore f32 [n] += lq for a live row (a dead row keeps it).  score stays the
// model's log-probability at temperature 1.
extern "C" int lv_rollout_pick_filtered_f32(const float* logits, long ld, const float* u, float inv_temp, int top_k, float top_p,
                                            const float* h_src, const float* c_src, float* h_dst, float* c_dst, int64_t* tok, int* alive,
                                            int64_t* ids, int* len, float* score, float* qscore, int* counter, int t, int Tmax, int n, int H,
                                            int V, int end_tok, void* stream) {
    if (!logits || !u || !h_src || !c_src || !h_dst || !c_dst || !tok || !alive || !ids || !len || !score || !qscore || !counter)
        return LV_ERR_ARG;
    if (h_src == h_dst || c_src == c_dst) return LV_ERR_ARG;
    if (n <= 0 || H <= 0 || V <= 0 || ld < V || Tmax <= 0 || t < 0 || t >= Tmax || end_tok < 0 || end_tok >= V) return LV_ERR_SHAPE;
    if (!(inv_temp > 0.f) || inv_temp == INFINITY || !(top_p > 0.f && top_p <= 1.f) || top_k < 0) return LV_ERR_SHAPE;
    if ((((uintptr_t)logits) & 15) || (ld & 3)) return LV_ERR_ALIGN;
    LV_LAUNCH(rollout_pick_filtered_kernel, dim3((unsigned)n), dim3(256), 0, stream, logits, ld, u, inv_temp, top_k, top_p, h_src, c_src,
              h_dst, c_dst, tok, alive, ids, len, score, qscore, counter, t, Tmax, H, V, end_tok);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
