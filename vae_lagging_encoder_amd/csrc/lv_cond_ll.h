// lv_cond_ll.h -- the eval-mode LSTM decoder's log p(x|z) for one sentence and a tile of 16 latent codes, shared by the grid
// kernel of lv_grid_posterior.hip (gp_cond_ll_kernel) and the Metropolis-Hastings chain of lv_mh.hip (mh_chain_kernel): the
// workspace layout and its prep kernel, the z-dependent set-up (c0, h0, the z half of the gates), the T - 1 timesteps
// (exact-f32 16x16x4 MFMA, online vocabulary log-sum-exp, no logits in memory), the prior term, and the one accept rule of the
// two Metropolis-Hastings kernels.  One definition each, so the routes compute the same bits from the same operands.
// The algorithm is described at the top of lv_grid_posterior.hip.
#pragma once
#include "lv_device.h"

namespace {

constexpr int GP_S = 16;          // samples per workgroup (MFMA M)
constexpr int GP_MAXH = 128;          // Hp = 256 spills (the A fragments and z halves outgrow the registers)
constexpr int GP_MAXNZ = 64;
constexpr float GP_LOG_2PI = 1.8378770664093453f;

__device__ __forceinline__ void gp_lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) { m = mn; s = 0.f; return; }
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

__host__ __device__ __forceinline__ int gp_hp(int H) {
    int hp = 16;
    while (hp < H) hp *= 2;
    return hp;
}

struct GpLayout {                 // float offsets into the workspace (every segment a multiple of 16 floats)
    long whh, pred, wz, tr, gxe, total;
};

__host__ __device__ __forceinline__ GpLayout gp_layout(int V, int H, int nz, int B, int Td) {
    const long hp = gp_hp(H), vp = (V + 15) / 16 * 16, nzp = (nz + 3) / 4 * 4;
    GpLayout L;
    L.whh = 0;
    L.pred = L.whh + 4 * hp * hp;
    L.wz = L.pred + vp * hp;
    L.tr = L.wz + 4 * hp * nzp;
    L.gxe = L.tr + hp * nzp;
    L.total = L.gxe + (long)B * Td * 4 * hp;
    return L;
}

// zero-padded weight images and the per-sentence input projection; one thread per output float
__global__ __launch_bounds__(256) void gp_prep_kernel(const int64_t* __restrict__ x, int T, const float* __restrict__ embed,
                                                      const float* __restrict__ trans, const float* __restrict__ w_ih,
                                                      const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                      const float* __restrict__ b_hh, const float* __restrict__ pred,
                                                      float* __restrict__ ws, int B, int V, int ni, int H, int nz) {
    const int Td = T - 1, hp = gp_hp(H), vp = (V + 15) / 16 * 16, nzp = (nz + 3) / 4 * 4, ldi = ni + nz;
    const GpLayout L = gp_layout(V, H, nz, B, Td);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < L.total; i += (long)gridDim.x * 256) {
        float v = 0.f;
        if (i < L.pred) {                                   // W_hh [g][u][k]
            const long g = i / ((long)hp * hp), u = (i / hp) % hp, k = i % hp;
            if (u < H && k < H) v = w_hh[(g * H + u) * H + k];
        } else if (i < L.wz) {                              // pred_linear [v][k]
            const long j = i - L.pred, r = j / hp, k = j % hp;
            if (r < V && k < H) v = pred[r * H + k];
        } else if (i < L.tr) {                              // z columns of W_ih [g][u][d]
            const long j = i - L.wz, g = j / ((long)hp * nzp), u = (j / nzp) % hp, d = j % nzp;
            if (u < H && d < nz) v = w_ih[(g * H + u) * ldi + ni + d];
        } else if (i < L.gxe) {                             // trans_linear [u][d]
            const long j = i - L.tr, u = j / nzp, d = j % nzp;
            if (u < H && d < nz) v = trans[u * nz + d];
        } else {                                            // gxe [b][t][g][u]
            const long j = i - L.gxe, u = j % hp, g = (j / hp) % 4, bt = j / (4L * hp), b = bt / Td, t = bt % Td;
            if (u < H) {
                int64_t tok = x[b * T + t];
                tok = (tok < 0 || tok >= V) ? 0 : tok;      // (an id outside the vocabulary must not read outside the table)
                const float* e = embed + tok * ni;
                const float* w = w_ih + (g * H + u) * ldi;
                float a = 0.f;
                for (int k = 0; k < ni; ++k) a += e[k] * w[k];
                v = (a + b_ih[g * H + u]) + b_hh[g * H + u];
            }
        }
        ws[i] = v;
    }
}

// the prep launch (arguments already checked by the caller)
inline void gp_launch_prep(const int64_t* x, int B, int T, const float* embed, const float* trans, const float* w_ih,
                           const float* w_hh, const float* b_ih, const float* b_hh, const float* pred, int V, int ni, int H,
                           int nz, float* ws, void* stream) {
    const long total = gp_layout(V, H, nz, B, T - 1).total;
    LV_LAUNCH(gp_prep_kernel, dim3((unsigned)lv_cdiv(total < 256L * 4096 ? total : 256L * 4096, 256)), dim3(256), 0, stream,
              x, T, embed, trans, w_ih, w_hh, b_ih, b_hh, pred, ws, B, V, ni, H, nz);
}

// the LDS of one (sentence, 16 samples) workgroup; NKC = Hp / 16
template <int NKC>
struct GpShared {
    __attribute__((aligned(16))) float hbuf[2][GP_S][NKC * 16];
    float zs[GP_S][GP_MAXNZ];
    float red_m[4][GP_S], red_s[4][GP_S], tl[GP_S];
};

// 256 threads (4 waves) of one workgroup: log p(x_b | zs[s]) for the 16 codes in sh.zs (written and barrier-ordered by the
// caller).  Returns the running NLL of sample tid in threads tid < 16 (nothing meaningful elsewhere).  On return nobody reads
// sh.hbuf or sh.zs any more; threads tid < 16 may still be reading sh.red_* / sh.tl, which the next call writes only behind
// its own barriers.
template <int NKC>
__device__ __forceinline__ float gp_cond_nll(GpShared<NKC>& sh, const int64_t* __restrict__ x, int T, int b,
                                             const float* __restrict__ ws, int B, int V, int H, int nz) {
    constexpr int HP = NKC * 16;
    constexpr int UBW = (NKC + 3) / 4;                      // 16-unit blocks per wave
    const int Td = T - 1, vt_n = (V + 15) / 16, nzp = (nz + 3) / 4 * 4;
    const GpLayout L = gp_layout(V, H, nz, B, Td);
    const float* __restrict__ whh = ws + L.whh;
    const float* __restrict__ pred = ws + L.pred;
    const float* __restrict__ wz = ws + L.wz;
    const float* __restrict__ tr = ws + L.tr;
    const float* __restrict__ gxe = ws + L.gxe;
    const int tid = (int)threadIdx.x, w = tid >> 6, l = tid & 63, lc = l & 15, lq = l >> 4;

    // c0 = z . trans^T, h0 = tanh(c0); the time-invariant z half of the gates
    float c[UBW][4], zp[UBW][4][4];
#pragma unroll
    for (int j = 0; j < UBW; ++j) {
        const int ub = w + 4 * j;
        if (ub >= NKC) continue;
        const int u = ub * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = lq * 4 + r;
            float a = 0.f;
            for (int d = 0; d < nz; ++d) a += sh.zs[s][d] * tr[(long)u * nzp + d];
            c[j][r] = a;
            sh.hbuf[0][s][u] = tanhf(a);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float q = 0.f;
                for (int d = 0; d < nz; ++d) q += sh.zs[s][d] * wz[((long)g * HP + u) * nzp + d];
                zp[j][g][r] = q;
            }
        }
    }
    float nll = 0.f;                                         // thread tid < 16: sample tid's running NLL
    __syncthreads();

    for (int t = 0; t < Td; ++t) {
        const float(*hin)[HP] = sh.hbuf[t & 1];
        float(*hout)[HP] = sh.hbuf[(t & 1) ^ 1];
        // ---- gates and cell update: lane (lc, lq) holds samples lq*4 + r of unit ub*16 + lc ----
        float4 af[NKC];
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) af[kc] = *reinterpret_cast<const float4*>(&hin[lc][kc * 16 + lq * 4]);
        const float* gx = gxe + ((long)b * Td + t) * 4 * HP;
#pragma unroll
        for (int j = 0; j < UBW; ++j) {
            const int ub = w + 4 * j;
            if (ub >= NKC) continue;
            const int u = ub * 16 + lc;
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float* wr = whh + ((long)g * HP + u) * HP + lq * 4;
#pragma unroll
                for (int kc = 0; kc < NKC; ++kc) {
                    const float4 bf = *reinterpret_cast<const float4*>(wr + kc * 16);
                    acc[g] = lv_mfma_16x16x4(af[kc].x, bf.x, acc[g]);
                    acc[g] = lv_mfma_16x16x4(af[kc].y, bf.y, acc[g]);
                    acc[g] = lv_mfma_16x16x4(af[kc].z, bf.z, acc[g]);
                    acc[g] = lv_mfma_16x16x4(af[kc].w, bf.w, acc[g]);
                }
            }
            float gxu[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gxu[g] = gx[g * HP + u];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) a[g] = (gxu[g] + zp[j][g][r]) + acc[g][r];
                const float ig = lv_sigmoid(a[0]), fg = lv_sigmoid(a[1]), gg = tanhf(a[2]), og = lv_sigmoid(a[3]);
                c[j][r] = fg * c[j][r] + ig * gg;
                hout[lq * 4 + r][u] = og * tanhf(c[j][r]);
            }
        }
        __syncthreads();
        // ---- vocabulary projection with an online log-sum-exp; 16-column tiles, wave w takes tiles w, w + 4, ... ----
        int64_t tgt = x[(long)b * T + t + 1];
        tgt = (tgt < 0 || tgt >= V) ? 0 : tgt;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) af[kc] = *reinterpret_cast<const float4*>(&hout[lc][kc * 16 + lq * 4]);
        float m[4], sm[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; sm[r] = 0.f; }
        for (int vt = w; vt < vt_n; vt += 4) {
            const int col = vt * 16 + lc;
            const float* pr = pred + (long)col * HP + lq * 4;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) {
                const float4 bf = *reinterpret_cast<const float4*>(pr + kc * 16);
                acc = lv_mfma_16x16x4(af[kc].x, bf.x, acc);
                acc = lv_mfma_16x16x4(af[kc].y, bf.y, acc);
                acc = lv_mfma_16x16x4(af[kc].z, bf.z, acc);
                acc = lv_mfma_16x16x4(af[kc].w, bf.w, acc);
            }
            if (col < V) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[r];
                    if (v > m[r]) { sm[r] = sm[r] * expf(m[r] - v) + 1.f; m[r] = v; }
                    else sm[r] += expf(v - m[r]);
                }
                if (col == (int)tgt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sh.tl[lq * 4 + r] = acc[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float m2 = __shfl_xor(m[r], d, 64), s2 = __shfl_xor(sm[r], d, 64);
                gp_lse_merge(m[r], sm[r], m2, s2);
            }
            if (lc == 0) { sh.red_m[w][lq * 4 + r] = m[r]; sh.red_s[w][lq * 4 + r] = sm[r]; }
        }
        __syncthreads();
        if (tid < GP_S) {
            float M = sh.red_m[0][tid], S = sh.red_s[0][tid];
            for (int i = 1; i < 4; ++i) gp_lse_merge(M, S, sh.red_m[i][tid], sh.red_s[i][tid]);
            nll += (M + logf(S)) - sh.tl[tid];
        }
        // (the next gates phase writes the other h buffer and the next red / tl writes follow its barrier)
    }
    return nll;
}

// log N(z; 0, I) + cond for one code z [nz]
__device__ __forceinline__ float gp_log_joint(const float* __restrict__ zk, int nz, float cond) {
    float q = 0.f;
    for (int d = 0; d < nz; ++d) q += zk[d] * zk[d];
    return (-0.5f * q - 0.5f * ((float)nz * GP_LOG_2PI)) + cond;
}

// ---- random-walk Metropolis-Hastings (VAE.sample_from_posterior, vae.py:218-254): shared by both kernels of lv_mh.hip ----
// The proposal eps * std + cur as torch.normal(mean, std) forms it: the product is rounded, then the sum (two roundings, never
// one fused multiply-add); see sgd_velocity in lv_optim.hip for what the pragma is there for.
__device__ __forceinline__ float mh_propose(float eps, float std, float cur) {
#pragma clang fp contract(off)
    const float t = eps * std;
    return t + cur;
}

// u < min(exp(ratio), 1) for u in [0, 1), with a NaN ratio rejecting (both comparisons are false; fminf would drop the NaN)
__device__ __forceinline__ bool mh_accept(float ratio, float u) { return ratio >= 0.f || u < expf(ratio); }

// index of the kept sample that iteration `iter` of the chain produces, or -1
__device__ __forceinline__ int mh_keep_index(int iter, int burn_in, int thin, int nsamples) {
    if (iter < burn_in || (iter - burn_in) % thin != 0) return -1;
    const int k = (iter - burn_in) / thin;
    return k < nsamples ? k : -1;
}

}  // namespace
