// lv_optim.hip -- global grad-norm, clip coefficient, fused clip+SGD (plain and with momentum) / clip+Adam over flat parameter buffers.
//
// Replaces torch.nn.utils.clip_grad_norm_(vae.parameters(), 5.0) (text.py:385, image.py:312; the norm spans
// encoder AND decoder grads -- SURVEY.md G1), optim.SGD(lr=1.0, momentum=0).step (text.py:325,387) and
// optim.Adam(lr=1e-3).step (image.py:267,314).  Parameters and grads live in flat HBM buffers (one segment per
// nn.Parameter, each 16-byte aligned) so the norm is one streaming reduction and the update one streaming pass.
// Scalars that change between graph replays (lr, step count) are read from device memory.
#include "lv_device.h"

namespace {

constexpr int NORM_BLOCKS = 1024;

__global__ __launch_bounds__(256) void sumsq_stage1_kernel(const float* __restrict__ x, long n, float* __restrict__ partial, int nblk) {
    __shared__ float red[4];
    const int tid = (int)threadIdx.x;
    // contiguous chunk per block, 16-byte vector loads on the aligned interior
    const long per = (((n + nblk - 1) / nblk) + 3) & ~3L;
    const long beg = (long)blockIdx.x * per;
    long end = beg + per;
    if (end > n) end = n;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (beg < end) {
        const bool vec = ((((uintptr_t)x) & 15) == 0);
        if (vec) {
            const long nv = (end - beg) / 4;
            const float4* x4 = reinterpret_cast<const float4*>(x + beg);
            for (long i = tid; i < nv; i += 256) {
                const float4 v = x4[i];
                s0 += v.x * v.x; s1 += v.y * v.y; s2 += v.z * v.z; s3 += v.w * v.w;
            }
            for (long i = beg + nv * 4 + tid; i < end; i += 256) s0 += x[i] * x[i];
        } else {
            for (long i = beg + tid; i < end; i += 256) s0 += x[i] * x[i];
        }
    }
    float s = (s0 + s1) + (s2 + s3);
    s = lv_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] (=|+=) sum(partial[0..NORM_BLOCKS))
__global__ __launch_bounds__(256) void sumsq_stage2_kernel(const float* __restrict__ partial, float* __restrict__ out, int accumulate, int nblk) {
    __shared__ double red[4];
    const int tid = (int)threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < nblk; i += 256) s += (double)partial[i];
    s = lv_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        out[0] = (float)(tot + (accumulate ? (double)out[0] : 0.0));
    }
}

// stage 1 over TWO buffers in one launch: blocks [0, nb1) reduce x1, blocks [nb1, nb1 + nb2) reduce x2
__global__ __launch_bounds__(256) void sumsq2_stage1_kernel(const float* __restrict__ x1, long n1, int nb1,
                                                            const float* __restrict__ x2, long n2, int nb2,
                                                            float* __restrict__ partial) {
    __shared__ float red[4];
    const int tid = (int)threadIdx.x;
    const bool first = (int)blockIdx.x < nb1;
    const float* x = first ? x1 : x2;
    const long n = first ? n1 : n2;
    const int nblk = first ? nb1 : nb2;
    const int blk = first ? (int)blockIdx.x : (int)blockIdx.x - nb1;
    const long per = (((n + nblk - 1) / nblk) + 3) & ~3L;
    const long beg = (long)blk * per;
    long end = beg + per;
    if (end > n) end = n;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (beg < end) {
        if ((((uintptr_t)x) & 15) == 0) {
            const long nv = (end - beg) / 4;
            const float4* x4 = reinterpret_cast<const float4*>(x + beg);
            for (long i = tid; i < nv; i += 256) {
                const float4 v = x4[i];
                s0 += v.x * v.x; s1 += v.y * v.y; s2 += v.z * v.z; s3 += v.w * v.w;
            }
            for (long i = beg + nv * 4 + tid; i < end; i += 256) s0 += x[i] * x[i];
        } else {
            for (long i = beg + tid; i < end; i += 256) s0 += x[i] * x[i];
        }
    }
    float s = (s0 + s1) + (s2 + s3);
    s = lv_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The transaction gate of a fused training step (lv_clip_*_txn_f32).  A persistent LSTM recurrence that ran into its bounded
// hand-off spin returns early and leaves a non-zero status word; everything queued behind it then works on a half-finished
// recurrence.  The gate sits in the one single-thread spot every step passes before anything is applied -- the clip coefficient --
// and decides on the DEVICE whether the step counts: status words zero (and, data parallel, the exchanged guard element zero: no
// rank saw a timeout) -> the step's pending report sums are committed and the step counter advances; otherwise the sticky void
// flag goes up, and the update kernels (lv_sgd_step_txn_f32 / lv_scale_txn_f32) leave weights and gradients alone for this and
// every later step until the host has noticed (one read per loss window), moved the engines down the fallback ladder and replayed
// the voided steps.  txn = {void flag, steps committed, pending loss / rec / kl sums}; acc = the three running report sums.
struct TxnGate {
    const int* status1; const int* status2;      // the two engines' persistent-launch status words (either may be null)
    const float* guard;                          // data parallel: element of the exchanged gradient buffer that is non-zero iff a rank was void
    float* txn;                                  // null: no gate (the plain entries)
    float* acc;
};

__device__ __forceinline__ bool txn_gate(const TxnGate& g) {
    if (!g.txn) return true;
    const bool bad = (g.status1 && g.status1[0] != 0) || (g.status2 && g.status2[0] != 0) || (g.guard && g.guard[0] != 0.f) ||
                     g.txn[0] != 0.f;
    if (bad) {
        g.txn[0] = 1.f;
    } else {
        if (g.acc) { g.acc[0] += g.txn[2]; g.acc[1] += g.txn[3]; g.acc[2] += g.txn[4]; }
        g.txn[1] += 1.f;
    }
    g.txn[2] = 0.f; g.txn[3] = 0.f; g.txn[4] = 0.f;
    return !bad;
}

// stage 2 + clip coefficient: sumsq = sum(partial) in double; norm = sqrt; coef = min(1, max_norm / (norm + 1e-6))
// (extra: partial sums of squares the gradients' PRODUCERS emitted -- lv_gemm_b16_sumsq, lv_embed_scatter_full_sumsq_f32 -- for the
// tensors stage 1 was not run over; 256 or 1024 threads)
__global__ __launch_bounds__(1024) void clip_finish_kernel(const float* __restrict__ partial, int nblk, const float* __restrict__ extra,
                                                           int n_extra, float max_norm, float* sumsq, float* coef, float* norm_out,
                                                           TxnGate gate) {
    __shared__ double red[16];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    double s = 0.0;
    for (int i = tid; i < nblk; i += nt) s += (double)partial[i];
    if (n_extra > 0 && (((uintptr_t)extra) & 15) == 0) {
        // ~30k producer partials at the Yahoo shape, written on other XCDs (every load is a trip to memory): 16-byte loads, four in
        // flight per thread -- two round trips instead of thirty
        const float4* e4 = reinterpret_cast<const float4*>(extra);
        const int n4 = n_extra / 4;
        for (int i0 = tid; i0 < n4; i0 += 4 * nt) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = e4[i0 + u * nt < n4 ? i0 + u * nt : i0];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * nt < n4) s += ((double)v[u].x + (double)v[u].y) + ((double)v[u].z + (double)v[u].w);
        }
        for (int i = n4 * 4 + tid; i < n_extra; i += nt) s += (double)extra[i];
    } else {
        for (int i = tid; i < n_extra; i += nt) s += (double)extra[i];
    }
    s = lv_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int w = 0; w < nt / 64; ++w) tot += red[w];
        const float ss = (float)tot;
        const float nrm = sqrtf(ss);
        float c = max_norm / (nrm + 1e-6f);
        if (c > 1.f) c = 1.f;
        if (sumsq) sumsq[0] = ss;
        coef[0] = c;
        if (norm_out) norm_out[0] = nrm;
        txn_gate(gate);
    }
}

// norm = sqrt(sumsq); coef = min(1, max_norm / (norm + 1e-6))   (torch.nn.utils.clip_grad_norm_)
__global__ void clip_coef_kernel(const float* sumsq, float max_norm, float* coef, float* norm_out, TxnGate gate) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float nrm = sqrtf(sumsq[0]);
        float c = max_norm / (nrm + 1e-6f);
        if (c > 1.f) c = 1.f;
        coef[0] = c;
        if (norm_out) norm_out[0] = nrm;
        txn_gate(gate);
    }
}

// data parallel: guard[0] = 1 when one of this rank's persistent launches reported a timeout, else 0 -- written into the tail
// padding of the gradient buffer that is about to be mean-all-reduced, so that afterwards it is non-zero on EVERY rank iff any
// rank was void (all ranks then void the same step and replay it together)
__global__ void txn_guard_kernel(const int* status1, const int* status2, float* guard) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        guard[0] = ((status1 && status1[0] != 0) || (status2 && status2[0] != 0)) ? 1.f : 0.f;
}

// x *= c over [0, n) by workgroup blk of nblk (16-byte accesses where the buffer allows)
__device__ __forceinline__ void scale_range(float* __restrict__ x2, long n2, float c, long blk, long nblk) {
    const long stride2 = nblk * 256;
    const long m4 = (((uintptr_t)x2) & 15) == 0 ? n2 / 4 : 0;
    float4* x4 = reinterpret_cast<float4*>(x2);
    for (long i = blk * 256 + threadIdx.x; i < m4; i += stride2) {
        float4 v = x4[i];
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        x4[i] = v;
    }
    for (long i = m4 * 4 + blk * 256 + threadIdx.x; i < n2; i += stride2) x2[i] *= c;
}

// g <- g*c (written back when wb); p <- p - a * g over [0, n) by workgroup blk of nblk
__device__ __forceinline__ void sgd_range(float* __restrict__ p, float* __restrict__ g, long n, float a, float c, bool wb, long blk, long nblk) {
    const long stride = nblk * 256;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g)) & 15) == 0;
    if (vec) {
        const long n4 = n / 4;
        float4* p4 = reinterpret_cast<float4*>(p);
        float4* g4 = reinterpret_cast<float4*>(g);
        for (long i = blk * 256 + threadIdx.x; i < n4; i += stride) {
            float4 gv = g4[i], pv = p4[i];
            gv.x *= c; gv.y *= c; gv.z *= c; gv.w *= c;
            pv.x -= a * gv.x; pv.y -= a * gv.y; pv.z -= a * gv.z; pv.w -= a * gv.w;
            p4[i] = pv;
            if (wb) g4[i] = gv;
        }
        for (long i = n4 * 4 + blk * 256 + threadIdx.x; i < n; i += stride) {
            const float gv = g[i] * c;
            p[i] -= a * gv;
            if (wb) g[i] = gv;
        }
    } else {
        for (long i = blk * 256 + threadIdx.x; i < n; i += stride) {
            const float gv = g[i] * c;
            p[i] -= a * gv;
            if (wb) g[i] = gv;
        }
    }
}

// g <- g*coef (optional write-back); p <- p - lr * g
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g, long n,
                                                  const float* __restrict__ lr, const float* __restrict__ coef,
                                                  int write_back, const float* __restrict__ void_flag,
                                                  float* __restrict__ x2, long n2) {
    if (void_flag && void_flag[0] != 0.f) return;      // the step was voided by the transaction gate: nothing is applied
    const float c = coef ? coef[0] : 1.f;
    // clip_grad_norm_ scales EVERY gradient, the buffer that is not stepped too: in this launch instead of one of its own
    // (16-byte accesses where the buffer allows: 150 MB of decoder gradient at the Yahoo shape whenever the clip is active)
    if (x2 && c != 1.0f) scale_range(x2, n2, c, (long)blockIdx.x, (long)gridDim.x);
    const float a = lr[0];
    const bool wb = write_back && c != 1.0f;      // g * 1 is g: the clipped-gradient write-back is skipped when the clip is inactive
    sgd_range(p, g, n, a, c, wb, (long)blockIdx.x, (long)gridDim.x);
}

// sgd_kernel where rows [0, V) of an embedding table (ni floats each, at element emb_off of p and g) carry a gradient on the rows of
// the batch's tokens only and EXACT +0 everywhere else -- what lv_embed_scatter_full* leaves behind (lv_sgd_step_scale_rows_txn_f32).
// tok[0 .. N) is that launch's sorted token list.  Workgroups [0, nb_rows): one wave per sorted position, the wave at a run's first
// position updates the row (the others leave after two loads); the remaining workgroups run the dense code over the rest of
// (p, g) and over x2.  An absent row would see g*c = +0 and p - a*(+0) = p: that holds bit for bit while c and a are finite and
// not negative (a negative factor turns the product into -0, which moves a p of -0; inf or NaN make it NaN), so any other
// (c, a) takes -- uniformly, the whole grid -- the dense walk over every row.
__global__ __launch_bounds__(256) void sgd_rows_kernel(float* __restrict__ p, float* __restrict__ g, long n,
                                                       const float* __restrict__ lr, const float* __restrict__ coef,
                                                       int write_back, const float* __restrict__ void_flag,
                                                       float* __restrict__ x2, long n2, long emb_off, int V, int ni,
                                                       const int* __restrict__ tok, int N, int nb_rows) {
    if (void_flag && void_flag[0] != 0.f) return;
    const float c = coef[0];
    const float a = lr[0];
    const bool wb = write_back && c != 1.0f;
    const bool rows_ok = c >= 0.f && c <= 3.402823466e+38f && a >= 0.f && a <= 3.402823466e+38f;      // (false for NaN)
    if (!rows_ok) {
        if (x2 && c != 1.0f) scale_range(x2, n2, c, (long)blockIdx.x, (long)gridDim.x);
        sgd_range(p, g, n, a, c, wb, (long)blockIdx.x, (long)gridDim.x);
        return;
    }
    if ((int)blockIdx.x >= nb_rows) {
        const long blk = (long)blockIdx.x - nb_rows, nblk = (long)gridDim.x - nb_rows;
        if (x2 && c != 1.0f) scale_range(x2, n2, c, blk, nblk);
        const long tail = emb_off + (long)V * ni;
        if (emb_off > 0) sgd_range(p, g, emb_off, a, c, wb, blk, nblk);
        if (tail < n) sgd_range(p + tail, g + tail, n - tail, a, c, wb, blk, nblk);
        return;
    }
    const int i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (i >= N) return;
    const int row = tok[i];
    if (i > 0 && tok[i - 1] == row) return;            // not the first position of its run
    if (row < 0 || row >= V) return;
    float* pr = p + emb_off + (long)row * ni;
    float* gr = g + emb_off + (long)row * ni;
    if (ni % 4 == 0 && ((((uintptr_t)pr) | ((uintptr_t)gr)) & 15) == 0) {
        for (int k = lane * 4; k < ni; k += 256) {
            float4 gv = *reinterpret_cast<float4*>(gr + k), pv = *reinterpret_cast<float4*>(pr + k);
            gv.x *= c; gv.y *= c; gv.z *= c; gv.w *= c;
            pv.x -= a * gv.x; pv.y -= a * gv.y; pv.z -= a * gv.z; pv.w -= a * gv.w;
            *reinterpret_cast<float4*>(pr + k) = pv;
            if (wb) *reinterpret_cast<float4*>(gr + k) = gv;
        }
    } else {
        for (int k = lane; k < ni; k += 64) {
            const float gv = gr[k] * c;
            pr[k] -= a * gv;
            if (wb) gr[k] = gv;
        }
    }
}

// buf * mu + g as torch.optim.SGD forms it -- buf.mul_(momentum).add_(grad): the product is rounded, then the sum (two roundings,
// never one fused multiply-add).  hipcc contracts a * b + c by default, and this ROCm's __fmul_rn / __fadd_rn are plain * and + that
// contract just the same: what keeps the two operations apart is the contraction pragma below (checked in the gfx950 ISA under
// hipcc's default flags: v_mul_f32, v_add_f32) on top of the -ffp-contract=off every build recipe of this library passes; the
// emulator's g++ has no such pragma and rests on that flag alone (tests/emu/build_emu.py).
__device__ __forceinline__ float sgd_velocity(float buf, float mu, float g) {
#pragma clang fp contract(off)
    const float t = buf * mu;
    return t + g;
}

// One element of torch.optim.SGD(momentum=mu, dampening=0, nesterov=False, weight_decay=0) on the clipped gradient c * g:
// buf <- buf * mu + g'; p <- p - lr * buf, the latter as ONE rounding (torch's add_(buf, alpha=-lr) is a fused multiply-add)
__device__ __forceinline__ void sgd_momentum_elem(float& p, float& g, float& buf, float c, float mu, float neg_lr) {
    g = g * c;
    buf = sgd_velocity(buf, mu, g);
    p = fmaf(neg_lr, buf, p);
}

// The momentum twin of sgd_kernel (lv_sgd_momentum_step*_f32): one velocity element per parameter element, laid out like p.
// A zero velocity buffer is torch's "no momentum_buffer yet" (0 * mu + g' = g' bit for bit), so there is no step counter.
// A no-op while the transaction gate's void flag is up: p, g, buf and x2 keep their bit patterns.
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, long n,
                                                           const float* __restrict__ lr, const float* __restrict__ coef, float mu,
                                                           int write_back, const float* __restrict__ void_flag,
                                                           float* __restrict__ x2, long n2) {
    if (void_flag && void_flag[0] != 0.f) return;
    const float c = coef ? coef[0] : 1.f;
    const long stride = (long)gridDim.x * 256;
    const long tid0 = (long)blockIdx.x * 256 + threadIdx.x;
    if (x2 && c != 1.0f) {
        const long m4 = (((uintptr_t)x2) & 15) == 0 ? n2 / 4 : 0;
        float4* x4 = reinterpret_cast<float4*>(x2);
        for (long i = tid0; i < m4; i += stride) {
            float4 v = x4[i];
            v.x *= c; v.y *= c; v.z *= c; v.w *= c;
            x4[i] = v;
        }
        for (long i = m4 * 4 + tid0; i < n2; i += stride) x2[i] *= c;
    }
    const float na = -lr[0];
    const bool wb = write_back && c != 1.0f;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)buf)) & 15) == 0;
    const long n4 = vec ? n / 4 : 0;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* b4 = reinterpret_cast<float4*>(buf);
    for (long i = tid0; i < n4; i += stride) {
        float4 pv = p4[i], gv = g4[i], bv = b4[i];
        sgd_momentum_elem(pv.x, gv.x, bv.x, c, mu, na);
        sgd_momentum_elem(pv.y, gv.y, bv.y, c, mu, na);
        sgd_momentum_elem(pv.z, gv.z, bv.z, c, mu, na);
        sgd_momentum_elem(pv.w, gv.w, bv.w, c, mu, na);
        p4[i] = pv;
        b4[i] = bv;
        if (wb) g4[i] = gv;
    }
    for (long i = n4 * 4 + tid0; i < n; i += stride) {
        float pv = p[i], gv = g[i], bv = buf[i];
        sgd_momentum_elem(pv, gv, bv, c, mu, na);
        p[i] = pv;
        buf[i] = bv;
        if (wb) g[i] = gv;
    }
}

__device__ __forceinline__ float bf16_bits_hi_to_f32(uint32_t bits_in_high_half) {      // bf16 = the high half of an f32
    float f;
    memcpy(&f, &bits_in_high_half, 4);
    return f;
}

// dst[i] = bf16(src[i]) * scale: the way back from a bf16 gradient payload (data-parallel exchange), with the 1/world mean folded in
__global__ __launch_bounds__(256) void cvt_f32_bf16_scaled_kernel(const uint16_t* __restrict__ src, long n, float scale,
                                                                  float* __restrict__ dst) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        const uint2 q = *reinterpret_cast<const uint2*>(src + i);
        float4 o;
        o.x = bf16_bits_hi_to_f32(q.x << 16) * scale; o.y = bf16_bits_hi_to_f32(q.x & 0xFFFF0000u) * scale;
        o.z = bf16_bits_hi_to_f32(q.y << 16) * scale; o.w = bf16_bits_hi_to_f32(q.y & 0xFFFF0000u) * scale;
        *reinterpret_cast<float4*>(dst + i) = o;
    } else {
        for (long j = i; j < n; ++j) dst[j] = bf16_bits_hi_to_f32((uint32_t)src[j] << 16) * scale;
    }
}

__global__ __launch_bounds__(256) void keep_scale_kernel(float* __restrict__ x, const uint8_t* __restrict__ keep, float kscale, int T,
                                                         int Bsz, int C, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long r = i / C;
    const int c = (int)(i % C);
    x[i] *= keep[((r % Bsz) * (long)T + r / Bsz) * C + c] ? kscale : 0.f;
}

// four consecutive columns per thread (C % 4 == 0, 16-byte aligned x, 4-byte aligned keep): one float4, four keep bytes in one
// load, one row division per four elements -- the scalar form above spends its time on a 64-bit division per element
__global__ __launch_bounds__(256) void keep_scale_v4_kernel(float* __restrict__ x, const uint8_t* __restrict__ keep, float kscale, int T,
                                                            int Bsz, int C4, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int r = (int)(i / C4), c4 = (int)(i - (long)r * C4);
    const int t = r / Bsz, b = r - t * Bsz;
    const uint32_t k = *reinterpret_cast<const uint32_t*>(keep + ((long)b * T + t) * (4L * C4) + 4 * c4);
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x *= (k & 0xFFu) ? kscale : 0.f;
    v.y *= (k & 0xFF00u) ? kscale : 0.f;
    v.z *= (k & 0xFF0000u) ? kscale : 0.f;
    v.w *= (k & 0xFF000000u) ? kscale : 0.f;
    reinterpret_cast<float4*>(x)[i] = v;
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long n, const float* __restrict__ coef,
                                                    const float* __restrict__ void_flag) {
    if (void_flag && void_flag[0] != 0.f) return;
    const float c = coef[0];
    if (c == 1.0f) return;            // clip inactive (coef is exactly 1): x * 1 is x bit for bit, skip the pass
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] *= c;
}

// torch.optim.Adam (no amsgrad, no weight decay): state = {m, v}; step count t read from device (float)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, const float* __restrict__ lr,
                                                   const float* __restrict__ coef, const float* __restrict__ step,
                                                   float beta1, float beta2, float eps, int write_back) {
    const float c = coef ? coef[0] : 1.f;
    const float a = lr[0];
    const float t = step[0];
    const float bc1 = 1.f - powf(beta1, t);
    const float bc2 = 1.f - powf(beta2, t);
    const float step_size = a / bc1;
    const float bc2s = sqrtf(bc2);
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gv = g[i] * c;
        const float mi = m[i] + (gv - m[i]) * (1.f - beta1);        // lerp form, as torch's _single_tensor_adam
        const float vi = v[i] * beta2 + (1.f - beta2) * gv * gv;
        const float denom = sqrtf(vi) / bc2s + eps;
        p[i] -= step_size * (mi / denom);
        m[i] = mi; v[i] = vi;
        if (write_back) g[i] = gv;
    }
}

// One element of torch.optim.Adam (amsgrad=False, weight_decay=0) on the clipped gradient c * g[i]: the same operation order as
// torch's _single_tensor_adam -- m.lerp_(g, 1 - beta1), v.mul_(beta2).addcmul_(g, g, 1 - beta2), p.addcdiv_(m, sqrt(v) / bc2s + eps,
// -step_size)
__device__ __forceinline__ void adam_elem(float& p, float& g, float& m, float& v, float c, float w1, float beta2, float w2, float step_size,
                                          float bc2s, float eps, bool wb) {
    const float gv = g * c;
    const float mi = m + w1 * (gv - m);
    const float vi = v * beta2 + w2 * gv * gv;
    const float denom = sqrtf(vi) / bc2s + eps;
    p = p - step_size * (mi / denom);
    m = mi;
    v = vi;
    if (wb) g = gv;
}

// The gated Adam step of the fused text trainer (lv_adam_step_txn_f32 / lv_adam_step_scale_txn_f32): a no-op while the transaction
// gate's void flag is up.  step[0] counts the COMMITTED steps of this optimizer; the bias corrections use step[0] + 1, the step
// number after this one, and adam_tick_kernel, queued behind this launch, advances the counter (no workgroup here writes it).
// x2 / n2: the gradient buffer of the side that is not stepped, scaled by the clip coefficient in the same launch.
__global__ __launch_bounds__(256) void adam_txn_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, const float* __restrict__ lr,
                                                       const float* __restrict__ coef, const float* __restrict__ step,
                                                       double beta1, double beta2, float eps, int write_back,
                                                       const float* __restrict__ void_flag, float* __restrict__ x2, long n2) {
    if (void_flag[0] != 0.f) return;
    const float c = coef ? coef[0] : 1.f;
    const long stride = (long)gridDim.x * 256;
    const long tid0 = (long)blockIdx.x * 256 + threadIdx.x;
    if (x2 && c != 1.0f) {
        const long m4 = (((uintptr_t)x2) & 15) == 0 ? n2 / 4 : 0;
        float4* x4 = reinterpret_cast<float4*>(x2);
        for (long i = tid0; i < m4; i += stride) {
            float4 t = x4[i];
            t.x *= c; t.y *= c; t.z *= c; t.w *= c;
            x4[i] = t;
        }
        for (long i = m4 * 4 + tid0; i < n2; i += stride) x2[i] *= c;
    }
    // the betas, 1 - beta and the bias corrections as torch forms them: Python floats (double), rounded to f32 where they meet the
    // tensors
    const double t = (double)step[0] + 1.0;
    const double bc1 = 1.0 - pow(beta1, t);
    const double bc2 = 1.0 - pow(beta2, t);
    const float step_size = (float)((double)lr[0] / bc1);
    const float bc2s = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2), b2 = (float)beta2;
    const bool wb = write_back && c != 1.0f;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
    const long n4 = vec ? n / 4 : 0;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4v = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (long i = tid0; i < n4; i += stride) {
        float4 pv = p4[i], gv = g4[i], mv = m4v[i], vv = v4[i];
        adam_elem(pv.x, gv.x, mv.x, vv.x, c, w1, b2, w2, step_size, bc2s, eps, wb);
        adam_elem(pv.y, gv.y, mv.y, vv.y, c, w1, b2, w2, step_size, bc2s, eps, wb);
        adam_elem(pv.z, gv.z, mv.z, vv.z, c, w1, b2, w2, step_size, bc2s, eps, wb);
        adam_elem(pv.w, gv.w, mv.w, vv.w, c, w1, b2, w2, step_size, bc2s, eps, wb);
        p4[i] = pv;
        m4v[i] = mv;
        v4[i] = vv;
        if (wb) g4[i] = gv;
    }
    for (long i = n4 * 4 + tid0; i < n; i += stride) {
        float pv = p[i], gv = g[i], mv = m[i], vv = v[i];
        adam_elem(pv, gv, mv, vv, c, w1, b2, w2, step_size, bc2s, eps, wb);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
        if (wb) g[i] = gv;
    }
}

// step[0] += 1 unless the step was voided: one thread, queued behind adam_txn_kernel
__global__ void adam_tick_kernel(float* step, const float* void_flag) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && void_flag[0] == 0.f) step[0] = step[0] + 1.f;
}

// out[0] += sum(x[0..n))  (single workgroup; n is a batch size)
__global__ __launch_bounds__(256) void sum_accum_kernel(const float* __restrict__ x, long n, float* out) {
    __shared__ float red[4];
    const int tid = (int)threadIdx.x;
    float s = 0.f;
    for (long i = tid; i < n; i += 256) s += x[i];
    s = lv_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[0] += (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void add_scalar_kernel(float* x, float v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) x[0] += v;
}

}  // namespace

extern "C" int lv_sumsq_workspace_floats() { return 2 * NORM_BLOCKS; }

// out[0] (=|+=) sum(x[i]^2); ws: lv_sumsq_workspace_floats() floats.  Deterministic two-stage reduction.
extern "C" int lv_sumsq_f32(const float* x, long n, float* ws, float* out, int accumulate, void* stream) {
    if (!x || !ws || !out || n < 0) return LV_ERR_ARG;
    long nb = (n + 8191) / 8192;
    if (nb < 1) nb = 1;
    if (nb > NORM_BLOCKS) nb = NORM_BLOCKS;
    const int nblk = (int)nb;
    LV_LAUNCH(sumsq_stage1_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, x, n, ws, nblk);
    LV_LAUNCH(sumsq_stage2_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, out, accumulate, nblk);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_clip_coef_f32(const float* sumsq, float max_norm, float* coef, float* norm_out, void* stream) {
    if (!sumsq || !coef) return LV_ERR_ARG;
    LV_LAUNCH(clip_coef_kernel, dim3(1), dim3(64), 0, stream, sumsq, max_norm, coef, norm_out, TxnGate{nullptr, nullptr, nullptr, nullptr, nullptr});
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_clip_coef_f32 + the transaction gate (see TxnGate): status1 / status2 / guard may be null; txn = device float[5] {void flag,
// steps committed, pending loss, rec, kl sums}; acc = device float[3] the committed running sums (may be null)
extern "C" int lv_clip_coef_txn_f32(const float* sumsq, float max_norm, float* coef, float* norm_out, const int* status1,
                                    const int* status2, const float* guard, float* txn, float* acc, void* stream) {
    if (!sumsq || !coef || !txn) return LV_ERR_ARG;
    LV_LAUNCH(clip_coef_kernel, dim3(1), dim3(64), 0, stream, sumsq, max_norm, coef, norm_out, TxnGate{status1, status2, guard, txn, acc});
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_txn_guard_f32(const int* status1, const int* status2, float* guard, void* stream) {
    if (!guard) return LV_ERR_ARG;
    LV_LAUNCH(txn_guard_kernel, dim3(1), dim3(64), 0, stream, status1, status2, guard);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

static inline unsigned lv_stream_grid(long n) {
    long b = (n + 1023) / 1024;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (unsigned)b;
}

extern "C" int lv_sgd_step_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev,
                               int write_back_clipped, void* stream) {
    if (!p || !g || !lr_dev || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    LV_LAUNCH(sgd_kernel, dim3(lv_stream_grid(n)), dim3(256), 0, stream, p, g, n, lr_dev, coef_dev, write_back_clipped, (const float*)nullptr, (float*)nullptr, 0L);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_sgd_step_f32 behind the transaction gate: a no-op while void_flag_dev[0] != 0 (txn[0] of lv_clip_*_txn_f32)
extern "C" int lv_sgd_step_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev,
                                   int write_back_clipped, const float* void_flag_dev, void* stream) {
    if (!p || !g || !lr_dev || !void_flag_dev || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    LV_LAUNCH(sgd_kernel, dim3(lv_stream_grid(n)), dim3(256), 0, stream, p, g, n, lr_dev, coef_dev, write_back_clipped, void_flag_dev, (float*)nullptr, 0L);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// x [T*Bsz][C] time-major (row t*Bsz + b) *= keep [Bsz][T][C] ? kscale : 0: the backward of nn.Dropout on the decoder LSTM's
// output (dec_lstm.py:106), applied to dO once with loads along C instead of inside the persistent BPTT
extern "C" int lv_keep_scale_f32(float* x, const uint8_t* keep, float kscale, int T, int Bsz, int C, void* stream) {
    if (!x || !keep) return LV_ERR_ARG;
    if (T < 0 || Bsz <= 0 || C <= 0) return LV_ERR_SHAPE;
    const long n = (long)T * Bsz * C;
    if (n == 0) return LV_OK;
    if (C % 4 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)keep) & 3) == 0 && (long)T * Bsz < (1L << 31))
        LV_LAUNCH(keep_scale_v4_kernel, dim3((unsigned)lv_cdiv(n / 4, 256)), dim3(256), 0, stream, x, keep, kscale, T, Bsz, C / 4, n / 4);
    else
        LV_LAUNCH(keep_scale_kernel, dim3((unsigned)lv_cdiv(n, 256)), dim3(256), 0, stream, x, keep, kscale, T, Bsz, C, n);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// dst f32 [n] = bf16 src [n] * scale (src 8-byte aligned, dst 16-byte aligned): unpacks a bf16 gradient payload
extern "C" int lv_cvt_f32_bf16_scaled(const uint16_t* src, long n, float scale, float* dst, void* stream) {
    if (!src || !dst || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    if ((((uintptr_t)src) & 7) != 0 || (((uintptr_t)dst) & 15) != 0) return LV_ERR_ALIGN;
    LV_LAUNCH(cvt_f32_bf16_scaled_kernel, dim3((unsigned)lv_cdiv(lv_cdiv(n, 4), 256)), dim3(256), 0, stream, src, n, scale, dst);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_scale_f32(float* x, long n, const float* coef_dev, void* stream) {
    if (!x || !coef_dev || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    LV_LAUNCH(scale_kernel, dim3(lv_stream_grid(n)), dim3(256), 0, stream, x, n, coef_dev, (const float*)nullptr);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_sgd_step_txn_f32 on (p, g) + lv_scale_txn_f32 on a second gradient buffer x2 (the one that is not stepped) in one launch
extern "C" int lv_sgd_step_scale_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev,
                                         int write_back_clipped, float* x2, long n2, const float* void_flag_dev, void* stream) {
    if (!p || !g || !lr_dev || !coef_dev || !void_flag_dev || !x2 || n < 0 || n2 < 0) return LV_ERR_ARG;
    if (n == 0 && n2 == 0) return LV_OK;
    LV_LAUNCH(sgd_kernel, dim3(lv_stream_grid(n > n2 ? n : n2)), dim3(256), 0, stream, p, g, n, lr_dev, coef_dev, write_back_clipped,
              void_flag_dev, x2, n2);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_sgd_step_scale_txn_f32 where the embedding table at elements [emb_off, emb_off + V * ni) of (p, g) has a gradient on the rows
// of the batch's tokens alone: tok[0 .. N) is the sorted token list of the lv_embed_scatter_full* launch that wrote that gradient
// this step (every other row of it is +0, and the table is stepped with nothing added to g since).  Same results as the dense
// entry bit for bit, same void-flag and write_back_clipped behaviour, one launch; the rows no token names are neither read nor
// written (89 of 199 MB at the Yahoo shape) unless lr or the clip coefficient is negative or not finite (see sgd_rows_kernel).
extern "C" int lv_sgd_step_scale_rows_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev,
                                              int write_back_clipped, float* x2, long n2, const float* void_flag_dev, long emb_off, int V,
                                              int ni, const int* sorted_tok, int N, void* stream) {
    if (!p || !g || !lr_dev || !coef_dev || !void_flag_dev || !x2 || !sorted_tok || n < 0 || n2 < 0) return LV_ERR_ARG;
    if (V <= 0 || ni <= 0 || N <= 0 || emb_off < 0 || emb_off + (long)V * ni > n) return LV_ERR_SHAPE;
    const long rest = n - (long)V * ni;
    const int nb_rows = (int)lv_cdiv((long)N, 4);
    LV_LAUNCH(sgd_rows_kernel, dim3((unsigned)nb_rows + lv_stream_grid(rest > n2 ? rest : n2)), dim3(256), 0, stream, p, g, n, lr_dev, coef_dev,
              write_back_clipped, void_flag_dev, x2, n2, emb_off, V, ni, sorted_tok, N, nb_rows);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// torch.optim.SGD(momentum > 0) (text.py --momentum: text.py:30,325-326) over a flat buffer: buf <- buf * momentum + coef * g,
// p <- p - lr * buf, bit for bit torch's arithmetic (see sgd_momentum_elem).  x2 / n2: see lv_sgd_step_scale_txn_f32.
static int sgd_momentum_step(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev, float momentum,
                             int write_back_clipped, float* x2, long n2, const float* void_flag_dev, void* stream) {
    if (n == 0 && n2 == 0) return LV_OK;
    LV_LAUNCH(sgd_momentum_kernel, dim3(lv_stream_grid(n > n2 ? n : n2)), dim3(256), 0, stream, p, g, buf, n, lr_dev, coef_dev, momentum,
              write_back_clipped, void_flag_dev, x2, n2);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_sgd_momentum_step_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev,
                                        float momentum, int write_back_clipped, void* stream) {
    if (!p || !g || !buf || !lr_dev || n < 0) return LV_ERR_ARG;
    return sgd_momentum_step(p, g, buf, n, lr_dev, coef_dev, momentum, write_back_clipped, nullptr, 0, nullptr, stream);
}

// lv_sgd_momentum_step_f32 behind the transaction gate: p, g and buf stay untouched while void_flag_dev[0] != 0
extern "C" int lv_sgd_momentum_step_txn_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev,
                                            float momentum, int write_back_clipped, const float* void_flag_dev, void* stream) {
    if (!p || !g || !buf || !lr_dev || !void_flag_dev || n < 0) return LV_ERR_ARG;
    return sgd_momentum_step(p, g, buf, n, lr_dev, coef_dev, momentum, write_back_clipped, nullptr, 0, void_flag_dev, stream);
}

// lv_sgd_momentum_step_txn_f32 on (p, g, buf) + lv_scale_txn_f32 on x2 (the gradient of the side that is not stepped) in one launch
extern "C" int lv_sgd_momentum_step_scale_txn_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev,
                                                  float momentum, int write_back_clipped, float* x2, long n2,
                                                  const float* void_flag_dev, void* stream) {
    if (!p || !g || !buf || !lr_dev || !coef_dev || !void_flag_dev || !x2 || n < 0 || n2 < 0) return LV_ERR_ARG;
    return sgd_momentum_step(p, g, buf, n, lr_dev, coef_dev, momentum, write_back_clipped, x2, n2, void_flag_dev, stream);
}

extern "C" int lv_scale_txn_f32(float* x, long n, const float* coef_dev, const float* void_flag_dev, void* stream) {
    if (!x || !coef_dev || !void_flag_dev || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    LV_LAUNCH(scale_kernel, dim3(lv_stream_grid(n)), dim3(256), 0, stream, x, n, coef_dev, void_flag_dev);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_adam_step_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev,
                                const float* coef_dev, const float* step_dev, float beta1, float beta2, float eps,
                                int write_back_clipped, void* stream) {
    if (!p || !g || !m || !v || !lr_dev || !step_dev || n < 0) return LV_ERR_ARG;
    if (n == 0) return LV_OK;
    LV_LAUNCH(adam_kernel, dim3(lv_stream_grid(n)), dim3(256), 0, stream, p, g, m, v, n, lr_dev, coef_dev, step_dev,
              beta1, beta2, eps, write_back_clipped);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_adam_step_f32 behind the transaction gate: p, g, m, v and the step counter step_dev[0] stay untouched while void_flag_dev[0] != 0;
// otherwise the step is taken with bias corrections for step number step_dev[0] + 1 and the counter advances by one
static int adam_step_txn(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev, float* step_dev,
                         double beta1, double beta2, float eps, int write_back_clipped, float* x2, long n2, const float* void_flag_dev,
                         void* stream) {
    if (!p || !g || !m || !v || !lr_dev || !step_dev || !void_flag_dev || n < 0 || n2 < 0) return LV_ERR_ARG;
    LV_LAUNCH(adam_txn_kernel, dim3(lv_stream_grid(n > n2 ? n : n2)), dim3(256), 0, stream, p, g, m, v, n, lr_dev, coef_dev,
              (const float*)step_dev, beta1, beta2, eps, write_back_clipped, void_flag_dev, x2, n2);
    LV_LAUNCH(adam_tick_kernel, dim3(1), dim3(64), 0, stream, step_dev, void_flag_dev);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_adam_step_txn_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev,
                                    float* step_dev, double beta1, double beta2, float eps, int write_back_clipped,
                                    const float* void_flag_dev, void* stream) {
    return adam_step_txn(p, g, m, v, n, lr_dev, coef_dev, step_dev, beta1, beta2, eps, write_back_clipped, nullptr, 0, void_flag_dev,
                         stream);
}

// lv_adam_step_txn_f32 on (p, g, m, v) + lv_scale_txn_f32 on x2 (the gradient of the side that is not stepped) in one launch
extern "C" int lv_adam_step_scale_txn_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev,
                                          float* step_dev, double beta1, double beta2, float eps, int write_back_clipped, float* x2,
                                          long n2, const float* void_flag_dev, void* stream) {
    if (!coef_dev || !x2) return LV_ERR_ARG;
    return adam_step_txn(p, g, m, v, n, lr_dev, coef_dev, step_dev, beta1, beta2, eps, write_back_clipped, x2, n2, void_flag_dev,
                         stream);
}

extern "C" int lv_sum_accum_f32(const float* x, long n, float* out_dev, void* stream) {
    if (!x || !out_dev || n < 0) return LV_ERR_ARG;
    LV_LAUNCH(sum_accum_kernel, dim3(1), dim3(256), 0, stream, x, n, out_dev);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_add_scalar_f32(float* x_dev, float v, void* stream) {
    if (!x_dev) return LV_ERR_ARG;
    LV_LAUNCH(add_scalar_kernel, dim3(1), dim3(64), 0, stream, x_dev, v);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// clip_grad_norm_ over two flat gradient buffers (encoder, decoder: the norm spans both) in two launches:
// one streaming pass over both buffers, then sum + norm + coefficient.  ws: lv_sumsq_workspace_floats() floats.
extern "C" int lv_clip_norm2_f32(const float* g1, long n1, const float* g2, long n2, float* ws, float max_norm,
                                 float* sumsq_dev, float* coef_dev, float* norm_dev, void* stream) {
    if (!g1 || !g2 || !ws || !coef_dev || n1 < 0 || n2 < 0) return LV_ERR_ARG;
    long nb1 = (n1 + 8191) / 8192, nb2 = (n2 + 8191) / 8192;
    if (nb1 < 1) nb1 = 1;
    if (nb1 > NORM_BLOCKS) nb1 = NORM_BLOCKS;
    if (nb2 < 1) nb2 = 1;
    if (nb2 > NORM_BLOCKS) nb2 = NORM_BLOCKS;
    LV_LAUNCH(sumsq2_stage1_kernel, dim3((unsigned)(nb1 + nb2)), dim3(256), 0, stream, g1, n1, (int)nb1, g2, n2, (int)nb2, ws);
    LV_LAUNCH(clip_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, (int)(nb1 + nb2), (const float*)nullptr, 0, max_norm,
              sumsq_dev, coef_dev, norm_dev, TxnGate{nullptr, nullptr, nullptr, nullptr, nullptr});
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_clip_norm2_f32 + the transaction gate (see TxnGate / lv_clip_coef_txn_f32)
static int clip_norm2_txn(const float* g1, long n1, const float* g2, long n2, float* ws, const float* extra, int n_extra, float max_norm,
                          float* sumsq_dev, float* coef_dev, float* norm_dev, const int* status1, const int* status2,
                          const float* guard, float* txn, float* acc, void* stream) {
    if (!g1 || !g2 || !ws || !coef_dev || !txn || n1 < 0 || n2 < 0 || n_extra < 0 || (n_extra > 0 && !extra)) return LV_ERR_ARG;
    long nb1 = (n1 + 8191) / 8192, nb2 = (n2 + 8191) / 8192;
    if (nb1 < 1) nb1 = 1;
    if (nb1 > NORM_BLOCKS) nb1 = NORM_BLOCKS;
    if (nb2 < 1) nb2 = 1;
    if (nb2 > NORM_BLOCKS) nb2 = NORM_BLOCKS;
    LV_LAUNCH(sumsq2_stage1_kernel, dim3((unsigned)(nb1 + nb2)), dim3(256), 0, stream, g1, n1, (int)nb1, g2, n2, (int)nb2, ws);
    LV_LAUNCH(clip_finish_kernel, dim3(1), dim3(n_extra > 0 ? 1024 : 256), 0, stream, (const float*)ws, (int)(nb1 + nb2), extra, n_extra,
              max_norm, sumsq_dev, coef_dev, norm_dev, TxnGate{status1, status2, guard, txn, acc});
    LV_CHECK_LAUNCH();
    return LV_OK;
}

extern "C" int lv_clip_norm2_txn_f32(const float* g1, long n1, const float* g2, long n2, float* ws, float max_norm,
                                     float* sumsq_dev, float* coef_dev, float* norm_dev, const int* status1, const int* status2,
                                     const float* guard, float* txn, float* acc, void* stream) {
    return clip_norm2_txn(g1, n1, g2, n2, ws, nullptr, 0, max_norm, sumsq_dev, coef_dev, norm_dev, status1, status2, guard, txn, acc, stream);
}

// The same where part of the gradient arrives as partial sums of squares its producers emitted (extra[0 .. n_extra): the
// vocabulary-sized tensors, see lv_gemm_b16_sumsq / lv_embed_scatter_full_sumsq_f32): g1 / g2 are then the REST of the two flat
// gradients, and the 164 MB of the three big tensors are not read a second time for the norm.
extern "C" int lv_clip_norm2_fold_txn_f32(const float* g1, long n1, const float* g2, long n2, float* ws, const float* extra, int n_extra,
                                          float max_norm, float* sumsq_dev, float* coef_dev, float* norm_dev, const int* status1,
                                          const int* status2, const float* guard, float* txn, float* acc, void* stream) {
    return clip_norm2_txn(g1, n1, g2, n2, ws, extra, n_extra, max_norm, sumsq_dev, coef_dev, norm_dev, status1, status2, guard, txn, acc, stream);
}
