// lv_beam.hip -- batched, device-resident beam search for the LSTM decoder (reference
// modules/decoders/dec_lstm.py:163-268).
//
// The reference decodes one sentence at a time and takes every decision on the host: per step a full [n][V] log-softmax,
// torch.topk over the n * V candidates, three host reads and a Python loop that sorts the picks into completed and live
// hypotheses.  Here B sentences are decoded together in a fixed layout of K slots per sentence ([B][K], sentence-major; a
// dead slot carries score -inf), and a step's decisions are three launches on caller-owned buffers:
//
//   beam_chunk_kernel   (row, V-chunk) workgroups: the chunk's (max, sum exp) and its K + 1 largest logits with their columns.
//                       A row's log-sum-exp is a constant of the row, so the order of a row's candidates is the order of its raw
//                       logits: no [n][V] log-probabilities are ever written.
//   beam_merge_kernel   one wave per sentence: the rows' log-sum-exp from the chunk partials, every surviving candidate's
//                       score (logit - lse) + score[slot] (the reference's order: log_softmax first, then the running
//                       log-probability), the best K - n_done of them and the runner-up (for the selection margin).
//   beam_advance_kernel one workgroup per sentence: dec_lstm.py:232-246 in rank order -- </s> completes a hypothesis, anything
//                       else takes the next free slot and the (h, c) rows of its parent; the trace keeps (parent, word, slot).
//
// Order is everywhere (score descending, flat index slot * V + word ascending) and every reduction has a fixed shape, so reruns
// are bit-identical.  (Two DIFFERENT logits of one row whose scores round to the same f32 are ordered among the chunk's K + 1
// survivors; equal logits resolve to the lower column, equal scores of different rows to the lower slot.)
//
// Per-sentence integer state `meta` [B][4]: {n_done, active, steps taken, reserved}.  Nothing here allocates or synchronises.
#include "lv_device.h"

#define LV_BEAM_MAX_K 16
#define LV_BEAM_CHUNK 2048                       // columns per stage-1 workgroup: 8 per thread
#define LV_BEAM_SLOT (2 + 2 * (LV_BEAM_MAX_K + 1))   // words of a (row, chunk) partial: max, sum, K + 1 values, K + 1 columns
#define LV_BEAM_MAX_ROWS 8192
#define LV_BEAM_MERGE_CACHE 3072                 // candidates the merge keeps in LDS (24 KB): K = 16 at ten chunks is 2720

namespace {

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) { m = mn; s = 0.f; return; }
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

// (v, i) comes before (w, j): larger value first, equal values by lower index
__device__ __forceinline__ bool beam_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// best (value, index) of the wave under beam_before, in every lane
__device__ __forceinline__ void beam_wave_best(float& v, int& i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        if (beam_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

constexpr int BEAM_NONE = 0x7fffffff;

// stage 1: grid (nchunk, B * K), 256 threads.  part[(row * nchunk + chunk) * LV_BEAM_SLOT ..] = {max, sum exp(x - max),
// val[0 .. K], col[0 .. K]} of columns [chunk * CHUNK, min(V, (chunk + 1) * CHUNK)); col = -1 where the chunk ran out.
__global__ __launch_bounds__(256) void beam_chunk_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ score,
                                                         const int* __restrict__ meta, float* __restrict__ part, int K, int V) {
    __shared__ float sm[4], ss[4];
    __shared__ float bv[2][4];
    __shared__ int bi[2][4];
    const int row = (int)blockIdx.y, chunk = (int)blockIdx.x, nchunk = (int)gridDim.x;
    const int b = row / K;
    if (!meta[4 * b + 1] || score[row] == -INFINITY) return;       // uniform for the workgroup
    const int tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    const int c0 = chunk * LV_BEAM_CHUNK;
    const float* x = logits + (long)row * ld;
    float v[8];
    float m = -INFINITY, s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + tid + 256 * j;
        v[j] = c < V ? x[c] : -INFINITY;
        if (c < V) lse_merge(m, s, v[j], 1.f);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float m2 = __shfl_xor(m, d, 64), s2 = __shfl_xor(s, d, 64);
        lse_merge(m, s, m2, s2);
    }
    if (l == 0) { sm[w] = m; ss[w] = s; }
    __syncthreads();
    float* out = part + ((long)row * nchunk + chunk) * LV_BEAM_SLOT;
    if (tid == 0) {
        float M = sm[0], S = ss[0];
        for (int i = 1; i < 4; ++i) lse_merge(M, S, sm[i], ss[i]);
        out[0] = M;
        out[1] = S;
    }
    // K + 1 rounds: the best element strictly behind the previous pick
    float pv = INFINITY;
    int pi = -1;
    int* outi = reinterpret_cast<int*>(out) + 2 + (LV_BEAM_MAX_K + 1);
    for (int r = 0; r <= K; ++r) {
        float best = -INFINITY;
        int besti = BEAM_NONE;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + tid + 256 * j;
            if (c < V && beam_before(pv, pi, v[j], c) && beam_before(v[j], c, best, besti)) { best = v[j]; besti = c; }
        }
        beam_wave_best(best, besti);
        if (l == 0) { bv[r & 1][w] = best; bi[r & 1][w] = besti; }
        __syncthreads();
        best = bv[r & 1][0];
        besti = bi[r & 1][0];
        for (int i = 1; i < 4; ++i)
            if (beam_before(bv[r & 1][i], bi[r & 1][i], best, besti)) { best = bv[r & 1][i]; besti = bi[r & 1][i]; }
        if (tid == 0) {
            out[2 + r] = best;
            outi[r] = besti == BEAM_NONE ? -1 : besti;
        }
        if (besti == BEAM_NONE) {                                   // ran out (uniform): the remaining entries are empty
            if (tid == 0)
                for (int q = r + 1; q <= K; ++q) { out[2 + q] = -INFINITY; outi[q] = -1; }
            break;
        }
        pv = best;
        pi = besti;
    }
}

// stage 2: one wave per sentence.  pick_score / pick_flat [B][K + 1]: the best n_pick = K - n_done candidates in rank order and,
// at position n_pick, the runner-up; flat = -1 where there was no candidate.  margin[b] = min(margin[b], last accepted - runner-up).
__global__ __launch_bounds__(64) void beam_merge_kernel(const float* __restrict__ part, int nchunk, const float* __restrict__ score,
                                                        const int* __restrict__ meta, float* __restrict__ pick_score,
                                                        int* __restrict__ pick_flat, float* __restrict__ margin, int K, int V) {
    __shared__ float lse[LV_BEAM_MAX_K], prev[LV_BEAM_MAX_K];
    __shared__ float csc[LV_BEAM_MERGE_CACHE];
    __shared__ int cfl[LV_BEAM_MERGE_CACHE];
    const int b = (int)blockIdx.x, l = (int)threadIdx.x;
    if (!meta[4 * b + 1]) return;
    int n_pick = K - meta[4 * b + 0];
    n_pick = n_pick < 0 ? 0 : (n_pick > K ? K : n_pick);
    if (l < K) {
        const int row = b * K + l;
        const float p = score[row];
        float M = -INFINITY, S = 0.f;
        if (p != -INFINITY)
            for (int ch = 0; ch < nchunk; ++ch) {
                const float* q = part + ((long)row * nchunk + ch) * LV_BEAM_SLOT;
                lse_merge(M, S, q[0], q[1]);
            }
        lse[l] = M + logf(S);
        prev[l] = p;
    }
    __syncthreads();
    const int KK = K + 1, per_row = nchunk * KK, ncand = K * per_row;
    // candidate i = (slot, chunk, j): its score and flat index, false where the slot is dead or the chunk ran out
    auto candidate = [&](int i, float& sc, int& flat) -> bool {
        const int k = i / per_row, rem = i - k * per_row, ch = rem / KK, j = rem - ch * KK;
        if (prev[k] == -INFINITY) return false;
        const float* q = part + ((long)(b * K + k) * nchunk + ch) * LV_BEAM_SLOT;
        const int col = reinterpret_cast<const int*>(q)[2 + (LV_BEAM_MAX_K + 1) + j];
        if (col < 0) return false;
        sc = (q[2 + j] - lse[k]) + prev[k];
        flat = k * V + col;
        return true;
    };
    // every round walks all candidates: evaluate them once into LDS when they fit (the same values either way)
    const bool cached = ncand <= LV_BEAM_MERGE_CACHE;
    if (cached) {
        for (int i = l; i < ncand; i += 64) {
            float sc = -INFINITY;
            int flat = BEAM_NONE;
            if (!candidate(i, sc, flat)) flat = BEAM_NONE;
            csc[i] = sc;
            cfl[i] = flat;
        }
        __syncthreads();
    }
    float pv = INFINITY;
    int pi = -1;
    float last = 0.f;
    for (int r = 0; r <= n_pick; ++r) {
        float best = -INFINITY;
        int besti = BEAM_NONE;
        for (int i = l; i < ncand; i += 64) {
            float sc;
            int flat;
            if (cached) {
                sc = csc[i];
                flat = cfl[i];
                if (flat == BEAM_NONE) continue;
            } else if (!candidate(i, sc, flat)) {
                continue;
            }
            if (beam_before(pv, pi, sc, flat) && beam_before(sc, flat, best, besti)) { best = sc; besti = flat; }
        }
        beam_wave_best(best, besti);
        if (l == 0) {
            pick_score[(long)b * KK + r] = best;
            pick_flat[(long)b * KK + r] = besti == BEAM_NONE ? -1 : besti;
        }
        if (besti == BEAM_NONE) {
            if (l == 0)
                for (int q = r + 1; q <= K; ++q) { pick_score[(long)b * KK + q] = -INFINITY; pick_flat[(long)b * KK + q] = -1; }
            return;
        }
        if (r == n_pick && n_pick > 0 && l == 0) margin[b] = fminf(margin[b], last - best);
        last = best;
        pv = best;
        pi = besti;
    }
    if (l == 0)
        for (int q = n_pick + 1; q <= K; ++q) { pick_score[(long)b * KK + q] = -INFINITY; pick_flat[(long)b * KK + q] = -1; }
}

// dec_lstm.py:232-246 for one sentence per workgroup.  (h_src, c_src) is the half the cell just wrote, (h_dst, c_dst) the half the
// next step reads; trace_t = this step's [B][K][3] slab.
__global__ __launch_bounds__(256) void beam_advance_kernel(const float* __restrict__ pick_score, const int* __restrict__ pick_flat,
                                                           const float* __restrict__ h_src, const float* __restrict__ c_src,
                                                           float* __restrict__ h_dst, float* __restrict__ c_dst,
                                                           int64_t* __restrict__ tok, float* __restrict__ score, int* __restrict__ meta,
                                                           float* __restrict__ done_score, int* __restrict__ done_ref,
                                                           int* __restrict__ trace_t, int* __restrict__ counter, int t, int K, int H,
                                                           int V, int end_tok) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int active = meta[4 * b + 1];
    int n_done = meta[4 * b + 0];
    __syncthreads();                                                // everybody has read meta before thread 0 rewrites it
    if (!active) return;
    n_done = n_done < 0 ? 0 : (n_done > K ? K : n_done);
    const int n_pick = K - n_done, KK = K + 1;
    int n_live = 0;
    for (int r = 0; r < K; ++r) {
        int* tr = trace_t + ((long)b * K + r) * 3;
        const int flat = r < n_pick ? pick_flat[(long)b * KK + r] : -1;
        if (flat < 0 || (long)flat >= (long)K * V) {               // no candidate (or not one of this sentence's)
            if (tid == 0) { tr[0] = -1; tr[1] = -1; tr[2] = -1; }
            continue;
        }
        const int parent = flat / V, word = flat - parent * V;
        const float sc = pick_score[(long)b * KK + r];
        if (word == end_tok) {
            if (tid == 0) {
                done_score[(long)b * K + n_done] = sc;
                done_ref[((long)b * K + n_done) * 2 + 0] = t;
                done_ref[((long)b * K + n_done) * 2 + 1] = r;
                tr[0] = parent; tr[1] = word; tr[2] = -1;
            }
            ++n_done;
        } else {
            const long src = ((long)b * K + parent) * H, dst = ((long)b * K + n_live) * H;
            for (int i = tid; i < H; i += 256) {
                h_dst[dst + i] = h_src[src + i];
                c_dst[dst + i] = c_src[src + i];
            }
            if (tid == 0) {
                tok[(long)b * K + n_live] = word;
                score[(long)b * K + n_live] = sc;
                tr[0] = parent; tr[1] = word; tr[2] = n_live;
            }
            ++n_live;
        }
    }
    if (tid == 0) {
        for (int k = n_live; k < K; ++k) score[(long)b * K + k] = -INFINITY;
        meta[4 * b + 0] = n_done;
        meta[4 * b + 2] = t + 1;
        if (n_done >= K || n_live == 0) {
            meta[4 * b + 1] = 0;
            atomicAdd(counter, -1);
        }
    }
}

__global__ __launch_bounds__(256) void beam_init_kernel(const float* __restrict__ h0, const float* __restrict__ c0,
                                                        float* __restrict__ h, float* __restrict__ c, int64_t* __restrict__ tok,
                                                        float* __restrict__ score, int* __restrict__ meta, float* __restrict__ done_score,
                                                        float* __restrict__ margin, int* __restrict__ counter, int B, int K, int H,
                                                        int start_tok) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    for (int i = tid; i < K * H; i += 256) {
        const int k = i / H, j = i - k * H;
        h[(long)b * K * H + i] = k == 0 ? h0[(long)b * H + j] : 0.f;
        c[(long)b * K * H + i] = k == 0 ? c0[(long)b * H + j] : 0.f;
    }
    if (tid < K) {
        tok[(long)b * K + tid] = start_tok;
        score[(long)b * K + tid] = tid == 0 ? 0.f : -INFINITY;
        done_score[(long)b * K + tid] = -INFINITY;
    }
    if (tid == 0) {
        meta[4 * b + 0] = 0; meta[4 * b + 1] = 1; meta[4 * b + 2] = 0; meta[4 * b + 3] = 0;
        margin[b] = INFINITY;
        if (b == 0) counter[0] = B;
    }
}

// one thread per sentence: the winner and its words
__global__ __launch_bounds__(64) void beam_backtrace_kernel(const float* __restrict__ score, const int* __restrict__ meta,
                                                            const float* __restrict__ done_score, const int* __restrict__ done_ref,
                                                            const int* __restrict__ trace, int64_t* __restrict__ ids, int* __restrict__ len,
                                                            float* __restrict__ win_score, int B, int K, int Tmax, int start_tok) {
    const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (b >= B) return;
    int64_t* out = ids + (long)b * (Tmax + 1);
    out[0] = start_tok;
    len[b] = 1;
    win_score[b] = 0.f;
    int n_done = meta[4 * b + 0], steps = meta[4 * b + 2];
    n_done = n_done < 0 ? 0 : (n_done > K ? K : n_done);
    steps = steps < 0 ? 0 : (steps > Tmax ? Tmax : steps);
    // first maximum over completed (completion order), then live slots (slot order)
    float best = 0.f;
    int kind = -1, which = 0;
    for (int i = 0; i < n_done; ++i) {
        const float s = done_score[(long)b * K + i];
        if (kind < 0 || s > best) { best = s; kind = 0; which = i; }
    }
    for (int k = 0; k < K; ++k) {
        const float s = score[(long)b * K + k];
        if (s == -INFINITY) continue;
        if (kind < 0 || s > best) { best = s; kind = 1; which = k; }
    }
    if (kind < 0 || steps == 0) return;
    int t, r = -1;
    if (kind == 0) {
        t = done_ref[((long)b * K + which) * 2 + 0];
        r = done_ref[((long)b * K + which) * 2 + 1];
        if (t < 0 || t >= steps || r < 0 || r >= K) return;
    } else {
        t = steps - 1;
        for (int q = 0; q < K; ++q)
            if (trace[(((long)t * B + b) * K + q) * 3 + 2] == which) { r = q; break; }
        if (r < 0) return;
    }
    const int n = t + 2;
    for (int s = t; s >= 0; --s) {
        const int* tr = trace + (((long)s * B + b) * K + r) * 3;
        const int parent = tr[0];
        out[s + 1] = tr[1];
        if (s == 0) break;
        r = -1;
        if (parent >= 0 && parent < K)
            for (int q = 0; q < K; ++q)
                if (trace[(((long)(s - 1) * B + b) * K + q) * 3 + 2] == parent) { r = q; break; }
        if (r < 0) return;                                          // broken chain: leave [<s>]
    }
    len[b] = n;
    win_score[b] = best;
}

bool beam_shape_ok(int B, int K, int V) {
    return B > 0 && K > 0 && V > 0 && K <= LV_BEAM_MAX_K && (long)K * V < (1L << 31) && (long)B * K <= LV_BEAM_MAX_ROWS;
}

}  // namespace

// 1 when (B sentences, beam width K, vocabulary V) is inside the envelope of the lv_beam_* entry points, else 0
extern "C" int lv_beam_supported(int B, int K, int V) { return beam_shape_ok(B, K, V) ? 1 : 0; }

// floats of `part` scratch lv_beam_select_f32 needs (0 outside the envelope)
extern "C" long lv_beam_ws_floats(int B, int K, int V) {
    if (!beam_shape_ok(B, K, V)) return 0;
    return (long)B * K * lv_cdiv(V, LV_BEAM_CHUNK) * LV_BEAM_SLOT;
}

// Start state of B sentences: slot 0 of every sentence holds <s> with score 0 and (h0, c0)[b] ([B][H]); the other slots are dead
// (score -inf, zero state).  h / c: the [B][K][H] half the first step reads.  counter[0] = B sentences still active.
extern "C" int lv_beam_init_f32(const float* h0, const float* c0, float* h, float* c, int64_t* tok, float* score, int* meta,
                                float* done_score, float* margin, int* counter, int B, int K, int H, int V, int start_tok,
                                void* stream) {
    if (!h0 || !c0 || !h || !c || !tok || !score || !meta || !done_score || !margin || !counter) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || H <= 0 || V <= 0 || start_tok < 0 || start_tok >= V) return LV_ERR_SHAPE;
    if (!beam_shape_ok(B, K, V)) return LV_ERR_UNSUPPORTED;
    LV_LAUNCH(beam_init_kernel, dim3((unsigned)B), dim3(256), 0, stream, h0, c0, h, c, tok, score, meta, done_score, margin, counter,
              B, K, H, start_tok);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// The selection of one step (dec_lstm.py:218-227 for every active sentence): logits [B * K][ld] -> pick_score / pick_flat
// [B][K + 1] (rank order; position K - n_done holds the runner-up) and the running minimum selection margin [B].
// part: lv_beam_ws_floats(B, K, V) floats.
extern "C" int lv_beam_select_f32(const float* logits, long ld, const float* score, const int* meta, float* part, float* pick_score,
                                  int* pick_flat, float* margin, int B, int K, int V, void* stream) {
    if (!logits || !score || !meta || !part || !pick_score || !pick_flat || !margin) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || V <= 0 || ld < V) return LV_ERR_SHAPE;
    if (!beam_shape_ok(B, K, V)) return LV_ERR_UNSUPPORTED;
    const int nchunk = lv_cdiv(V, LV_BEAM_CHUNK);
    LV_LAUNCH(beam_chunk_kernel, dim3((unsigned)nchunk, (unsigned)(B * K)), dim3(256), 0, stream, logits, ld, score, meta, part, K, V);
    LV_LAUNCH(beam_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, (const float*)part, nchunk, score, meta, pick_score, pick_flat,
              margin, K, V);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// The bookkeeping of one step (dec_lstm.py:232-246) from lv_beam_select_f32's picks: completed hypotheses are appended to
// done_score [B][K] / done_ref [B][K][2] = (step, rank); the others take the low slots of tok / score and of (h_dst, c_dst), which
// receive their parents' rows of (h_src, c_src) (all [B][K][H]; src and dst must not overlap); trace [Tmax][B][K][3] gets step
// t's (parent slot, word, destination slot or -1).  A sentence with K completed hypotheses or no live one goes inactive and
// counter[0] drops by one.
extern "C" int lv_beam_advance_f32(const float* pick_score, const int* pick_flat, const float* h_src, const float* c_src, float* h_dst,
                                   float* c_dst, int64_t* tok, float* score, int* meta, float* done_score, int* done_ref, int* trace,
                                   int* counter, int t, int Tmax, int B, int K, int H, int V, int end_tok, void* stream) {
    if (!pick_score || !pick_flat || !h_src || !c_src || !h_dst || !c_dst || !tok || !score || !meta || !done_score || !done_ref ||
        !trace || !counter)
        return LV_ERR_ARG;
    if (h_src == h_dst || c_src == c_dst) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || H <= 0 || V <= 0 || Tmax <= 0 || t < 0 || t >= Tmax || end_tok < 0 || end_tok >= V) return LV_ERR_SHAPE;
    if (!beam_shape_ok(B, K, V)) return LV_ERR_UNSUPPORTED;
    LV_LAUNCH(beam_advance_kernel, dim3((unsigned)B), dim3(256), 0, stream, pick_score, pick_flat, h_src, c_src, h_dst, c_dst, tok, score,
              meta, done_score, done_ref, trace + (long)t * B * K * 3, counter, t, K, H, V, end_tok);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// The winner of every sentence (first maximum over completed hypotheses in completion order, then live slots in slot order) and
// its words: ids [B][Tmax + 1] with <s> in front, len [B], win_score [B].  A sentence with no hypothesis yields [<s>].
extern "C" int lv_beam_backtrace(const float* score, const int* meta, const float* done_score, const int* done_ref, const int* trace,
                                 int64_t* ids, int* len, float* win_score, int B, int K, int Tmax, int start_tok, void* stream) {
    if (!score || !meta || !done_score || !done_ref || !trace || !ids || !len || !win_score) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || Tmax <= 0 || start_tok < 0) return LV_ERR_SHAPE;
    if (K > LV_BEAM_MAX_K) return LV_ERR_UNSUPPORTED;
    LV_LAUNCH(beam_backtrace_kernel, dim3((unsigned)lv_cdiv(B, 64)), dim3(64), 0, stream, score, meta, done_score, done_ref, trace, ids,
              len, win_score, B, K, Tmax, start_tok);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
