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

// ---- temperature / top-k / nucleus (top-p) sampling: one 256-thread workgroup per row ----------------------------------------------
// With y[c] = x[c] * inv_temp (one f32 multiply) and the order of lv_argmax_before on y (larger first, lower column among equals):
// Kk = the first min(top_k, C) columns (all of them when top_k <= 0 or >= C); w[c] = exp(y[c] - max y); K = the shortest prefix of
// Kk whose weight reaches top_p * sum_Kk w (K = Kk when top_p >= 1; never empty).  The draw is lv_wave_sample_row's rule restricted
// to K and taken in COLUMN order: the first column of K with w > 0 whose inclusive running sum over K reaches u * sum_K w; the last
// positive-weight column of K if rounding leaves the sum short; C - 1 only if no column has positive weight.
//
// No sort.  K is described by a threshold: K = {y > tau} plus the first ntie columns with y == tau.  tau is found by a radix descent
// (4 bits a level, 8 levels) over an order-preserving 32-bit key of y: per level every thread counts -- and for top-p weighs -- the
// columns under the current prefix per digit in registers, the workgroup adds the 256 partials through LDS in a fixed order, and
// every thread takes the same decision from the same 16 totals.  Columns equal to tau have equal weights, so how many of them the
// nucleus needs is arithmetic.  A last pass in column order (one 16-byte piece per thread and round, a wave scan and one barrier a
// round) does the draw.  The row is re-read from global memory (L2) on every pass: 16-byte pieces from clamped indices, the columns
// C .. ld never used as values.
//
// Every decision is a function of the row alone: no atomics, fixed summation orders, so repeated launches and both entry points
// (lv_sample_filtered_rows_f32, lv_rollout_pick_filtered_f32) give the same bits.
//
// Rounding: every sum is carried in double -- the weights are f32 (expf of an f32 difference), their per-thread, per-workgroup and
// running sums are not -- so L, the longest chain of dependent F32 additions behind one sum, is
constexpr int LV_FILTERED_L = 2;   // the two f32 subtractions of a score, (x - M) - (float)log(S); tests/test_filtered_sampling.py reads it
constexpr int LV_FP_NT = 256;
constexpr int LV_FP_BATCH = 4;     // 16-byte loads a thread issues before it consumes any of them

struct LvFilteredShared {          // static LDS of one workgroup, 49.7 KB
    double pw[16][LV_FP_NT];       // per-thread weight per digit ...
    int pc[16][LV_FP_NT];          // ... and count
    double qw[16][16];             // 16 threads' worth each
    int qc[16][16];
    double tw[16];                 // the workgroup's totals
    int tc[16];
    double sd[2][4][2];            // small reductions, double-buffered for the scan's one barrier per round
    int si[2][4][2];
    float rf[4];
    unsigned ru[4];
};

struct LvFilteredPick {
    int pick;
    float lp;                      // (x[pick] - max x) - log sum_all exp(x - max x): the model's log-probability at temperature 1
    float lq;                      // (y[pick] - max y) - log sum_K w: the log-probability under the distribution drawn from
    int kept;                      // |K|
    float tau;                     // min y over K
    int ntie;                      // columns of K equal to tau
};

// larger y <=> larger key; -0 and +0 share a key, as they compare equal
__device__ __forceinline__ unsigned lv_order_key(float y) {
    unsigned b;
    memcpy(&b, &y, 4);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lv_order_key_value(unsigned k) {
    const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float y;
    memcpy(&y, &b, 4);
    return y;
}

// LV_FP_BATCH 16-byte pieces of the row for thread tid, from clamped indices: v[4 j + i] is column 4 (q0 + j NT + tid) + i
__device__ __forceinline__ void lv_fp_load(const float4* __restrict__ x4, int n4, int q0, int tid, float (&v)[4 * LV_FP_BATCH]) {
#pragma unroll
    for (int j = 0; j < LV_FP_BATCH; ++j) {
        const int q = q0 + j * LV_FP_NT + tid;
        const float4 f = x4[q < n4 ? q : n4 - 1];
        v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
    }
}
__device__ __forceinline__ int lv_fp_col(int q0, int tid, int j) { return 4 * (q0 + (j >> 2) * LV_FP_NT + tid) + (j & 3); }

// One level of the descent.  Of the columns whose key agrees with `prefix` above bit shift + 4 and is larger than lo (-1: every
// key): sh.tc[d] = how many have digit d at `shift`, sh.tw[d] = their weight (W).  Ends with a barrier: every thread may read both.
template <bool W>
__device__ __forceinline__ void lv_fp_level(const float4* __restrict__ x4, int n4, int V, int tid, float inv_temp, float My, int shift,
                                            unsigned prefix, long long lo, LvFilteredShared& sh) {
    int cnt[16];
    double ws[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) { cnt[d] = 0; ws[d] = 0.0; }
    const unsigned long long hi = (unsigned long long)prefix >> (shift + 4);
    for (int q0 = 0; q0 < n4; q0 += LV_FP_NT * LV_FP_BATCH) {
        float v[4 * LV_FP_BATCH];
        lv_fp_load(x4, n4, q0, tid, v);
#pragma unroll
        for (int j = 0; j < 4 * LV_FP_BATCH; ++j) {
            const float y = v[j] * inv_temp;
            const unsigned k = lv_order_key(y);
            if (lv_fp_col(q0, tid, j) < V && ((unsigned long long)k >> (shift + 4)) == hi && (long long)k > lo) {
                const int dig = (int)((k >> shift) & 15u);
                const double w = W ? (double)expf(y - My) : 0.0;
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    cnt[d] += dig == d ? 1 : 0;
                    if (W) ws[d] += dig == d ? w : 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        sh.pc[d][tid] = cnt[d];
        if (W) sh.pw[d][tid] = ws[d];
    }
    __syncthreads();
    {
        const int d = tid >> 4, part = tid & 15;
        int c = 0;
        double s = 0.0;
        for (int i = 0; i < 16; ++i) {
            c += sh.pc[d][i * 16 + part];
            if (W) s += sh.pw[d][i * 16 + part];
        }
        sh.qc[d][part] = c;
        sh.qw[d][part] = s;
    }
    __syncthreads();
    if (tid < 16) {
        int c = 0;
        double s = 0.0;
        for (int i = 0; i < 16; ++i) { c += sh.qc[tid][i]; s += sh.qw[tid][i]; }
        sh.tc[tid] = c;
        sh.tw[tid] = s;
    }
    __syncthreads();
}

// The whole decision for one row x[0 .. V) (16-byte aligned), by the LV_FP_NT threads of a workgroup; every thread returns it.
__device__ __forceinline__ LvFilteredPick lv_block_filtered_pick(const float* __restrict__ x, int V, float u, float inv_temp, int top_k,
                                                                 float top_p, int tid, LvFilteredShared& sh) {
    const int l = tid & 63, wv = tid >> 6;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int n4 = (V + 3) >> 2;
    // pass 1: max x (max y is its image: rounding is monotone) and the smallest key
    float Mx = -INFINITY;
    unsigned kmin = 0xffffffffu;
    for (int q0 = 0; q0 < n4; q0 += LV_FP_NT * LV_FP_BATCH) {
        float v[4 * LV_FP_BATCH];
        lv_fp_load(x4, n4, q0, tid, v);
#pragma unroll
        for (int j = 0; j < 4 * LV_FP_BATCH; ++j) {
            if (lv_fp_col(q0, tid, j) < V) {
                Mx = fmaxf(Mx, v[j]);
                const unsigned k = lv_order_key(v[j] * inv_temp);
                kmin = k < kmin ? k : kmin;
            }
        }
    }
    Mx = lv_wave_max(Mx);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)kmin, d, 64);
        kmin = o < kmin ? o : kmin;
    }
    if (l == 0) { sh.rf[wv] = Mx; sh.ru[wv] = kmin; }
    __syncthreads();
    for (int i = 0; i < 4; ++i) {
        Mx = fmaxf(Mx, sh.rf[i]);
        kmin = sh.ru[i] < kmin ? sh.ru[i] : kmin;
    }
    const float My = Mx * inv_temp;

    // top-k: the key of the k-th column in order, and how many of its equals are in
    const int k_eff = (top_k > 0 && top_k < V) ? top_k : V;
    unsigned tauk = kmin;
    int ntie_k = 0;
    if (k_eff < V) {
        unsigned prefix = 0u;
        int rem = k_eff;                                             // 1 <= rem <= columns under the prefix, at every level
        for (int shift = 28; shift >= 0; shift -= 4) {
            lv_fp_level<false>(x4, n4, V, tid, inv_temp, My, shift, prefix, -1LL, sh);
            int d = 15;
            for (; d > 0; --d) {
                const int c = sh.tc[d];
                if (c >= rem) break;
                rem -= c;
            }
            prefix |= (unsigned)d << shift;
        }
        tauk = prefix;
        ntie_k = rem;
    }
    // pass 2: sum exp(x - max x) for lp, the weight of Kk above its threshold, the columns equal to it
    double Sx = 0.0, Sab = 0.0;
    int ctie = 0;
    for (int q0 = 0; q0 < n4; q0 += LV_FP_NT * LV_FP_BATCH) {
        float v[4 * LV_FP_BATCH];
        lv_fp_load(x4, n4, q0, tid, v);
#pragma unroll
        for (int j = 0; j < 4 * LV_FP_BATCH; ++j) {
            if (lv_fp_col(q0, tid, j) < V) {
                const float y = v[j] * inv_temp;
                const unsigned k = lv_order_key(y);
                Sx += (double)expf(v[j] - Mx);
                if (k > tauk) Sab += (double)expf(y - My);
                ctie += k == tauk ? 1 : 0;
            }
        }
    }
    Sx = lv_wave_sum(Sx);
    Sab = lv_wave_sum(Sab);
    ctie = lv_wave_sum(ctie);
    if (l == 0) { sh.sd[0][wv][0] = Sx; sh.sd[0][wv][1] = Sab; sh.si[0][wv][0] = ctie; }
    __syncthreads();
    Sx = (sh.sd[0][0][0] + sh.sd[0][1][0]) + (sh.sd[0][2][0] + sh.sd[0][3][0]);
    Sab = (sh.sd[0][0][1] + sh.sd[0][1][1]) + (sh.sd[0][2][1] + sh.sd[0][3][1]);
    ctie = (sh.si[0][0][0] + sh.si[0][1][0]) + (sh.si[0][2][0] + sh.si[0][3][0]);
    __syncthreads();                                                 // sd / si are the scan's buffers below
    if (k_eff == V) ntie_k = ctie;
    const double w_tk = (double)expf(lv_order_key_value(tauk) - My);
    const double S_kk = Sab + (double)ntie_k * w_tk;

    // top-p: the shortest prefix of Kk that reaches top_p * S_kk.  acc < target holds throughout, so the bucket that reaches the
    // target has positive weight, and so has every column in it (weights fall with the key).
    unsigned tau = tauk;
    int ntie = ntie_k, kept = k_eff;
    double SK = S_kk;
    if (top_p < 1.f) {
        const double target = (double)top_p * S_kk;
        double acc = 0.0;
        int cacc = 0, cb = 0;
        unsigned prefix = 0u;
        bool reached = true;
        for (int shift = 28; shift >= 0; shift -= 4) {
            lv_fp_level<true>(x4, n4, V, tid, inv_temp, My, shift, prefix, (long long)tauk, sh);
            // the ntie_k members equal to tauk were left out above (their equals outside Kk look the same): they join their bucket here
            const bool inj = ((unsigned long long)tauk >> (shift + 4)) == ((unsigned long long)prefix >> (shift + 4));
            const int dt = (int)((tauk >> shift) & 15u);
            int d = 15;
            bool hit = false;
            for (; d >= 0; --d) {
                double w = sh.tw[d];
                int c = sh.tc[d];
                if (inj && d == dt) { w += (double)ntie_k * w_tk; c += ntie_k; }
                if (acc + w >= target) { hit = true; cb = c; break; }
                acc += w;
                cacc += c;
            }
            if (!hit) { reached = false; break; }                    // rounding left the sum short (or the row has no weight): K = Kk
            prefix |= (unsigned)d << shift;
        }
        if (reached) {
            // cb columns equal to `prefix`, each of weight w_t > 0: the smallest j in [1, cb] with acc + j w_t >= target
            const double w_t = (double)expf(lv_order_key_value(prefix) - My);
            const double need = (target - acc) / w_t;
            int j = need >= (double)cb ? cb : (int)ceil(need);
            j = j < 1 ? 1 : (j > cb ? cb : j);
            if (j > 1 && acc + (double)(j - 1) * w_t >= target) --j;
            if (j < cb && acc + (double)j * w_t < target) ++j;
            tau = prefix;
            ntie = j;
            kept = cacc + j;
            SK = acc + (double)j * w_t;
        }
    }

    // the draw, in column order: a round is 1024 consecutive columns, four to a thread
    const double w_tau = (double)expf(lv_order_key_value(tau) - My);
    const double target = (double)u * SK;
    double runA = 0.0;                                               // weight of {y > tau} before this round
    int runT = 0;                                                    // columns equal to tau before this round
    int found = LV_ARGMAX_NONE, last_pos = -1;
    int buf = 0;
    for (int q0 = 0; q0 < n4; q0 += LV_FP_NT, buf ^= 1) {
        const int q = q0 + tid;
        const float4 f = x4[q < n4 ? q : n4 - 1];
        const float xv[4] = {f.x, f.y, f.z, f.w};
        double a[4];
        int t[4];
        double A = 0.0;
        int T = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = xv[j] * inv_temp;
            const unsigned k = lv_order_key(y);
            const bool valid = q < n4 && 4 * q + j < V;
            a[j] = valid && k > tau ? (double)expf(y - My) : 0.0;
            t[j] = valid && k == tau ? 1 : 0;
            A += a[j];
            T += t[j];
        }
        double sA = A;
        int sT = T;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double oA = __shfl_up(sA, d, 64);
            const int oT = __shfl_up(sT, d, 64);
            if (l >= d) { sA += oA; sT += oT; }
        }
        if (l == 63) { sh.sd[buf][wv][0] = sA; sh.si[buf][wv][0] = sT; }
        double cA = __shfl_up(sA, 1, 64);                            // the wave's columns in front of this thread's
        int cT = __shfl_up(sT, 1, 64);
        if (l == 0) { cA = 0.0; cT = 0; }
        __syncthreads();
        double pA = runA;
        int pT = runT;
        for (int i = 0; i < 4; ++i) {
            if (i == wv) { cA += pA; cT += pT; }
            pA += sh.sd[buf][i][0];
            pT += sh.si[buf][i][0];
        }
        runA = pA;
        runT = pT;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cA += a[j];
            cT += t[j];
            const bool member = a[j] > 0.0 || (t[j] && cT <= ntie && w_tau > 0.0);      // in K with positive weight
            if (member) {
                last_pos = 4 * q + j;
                const double incl = cA + (double)(cT < ntie ? cT : ntie) * w_tau;
                if (found == LV_ARGMAX_NONE && incl >= target) found = 4 * q + j;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int of = __shfl_xor(found, d, 64), ol = __shfl_xor(last_pos, d, 64);
        found = of < found ? of : found;
        last_pos = ol > last_pos ? ol : last_pos;
    }
    __syncthreads();                                                 // the last round's readers of si are done
    if (l == 0) { sh.si[0][wv][0] = found; sh.si[0][wv][1] = last_pos; }
    __syncthreads();
    for (int i = 0; i < 4; ++i) {
        found = sh.si[0][i][0] < found ? sh.si[0][i][0] : found;
        last_pos = sh.si[0][i][1] > last_pos ? sh.si[0][i][1] : last_pos;
    }
    LvFilteredPick r;
    r.pick = found != LV_ARGMAX_NONE ? found : (last_pos >= 0 ? last_pos : V - 1);
    const float xp = x[r.pick];
    r.lp = (xp - Mx) - (float)log(Sx);
    r.lq = (xp * inv_temp - My) - (float)log(SK);
    r.kept = kept;
    r.tau = lv_order_key_value(tau);
    r.ntie = ntie;
    return r;
}
