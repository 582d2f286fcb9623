// lv_grid_posterior.hip -- the model posterior on a latent grid (VAE.eval_log_model_posterior / calc_model_posterior_mean,
// modules/vae.py:170-196, 256-273), the hot path of the synthetic experiment (toy.py:188-231, 391-462, 482-483).
//
// (a) lv_dec_cond_ll_f32: cond_ll[b][s] = log p(x_b | z_{b,s}) of the eval-mode LSTM decoder (dec_lstm.py:66-148, no dropout)
//     for K samples per sentence; z has a sentence stride, 0 = one grid [K][nz] shared by every sentence (never expanded).
//     Prep launch (once per call): zero-padded images of W_hh, pred_linear, the z columns of W_ih and trans_linear, and the
//     sentence-only half of the input projection gxe[b][t] = E[x_t] . W_ih[:, :ni]^T + b_ih + b_hh -- once per SENTENCE, not per
//     sample.  Main launch: one workgroup (4 waves) per (sentence, tile of 16 samples), the samples along M of
//     v_mfma_f32_16x16x4_f32 (exact f32).  Per timestep:
//       gates  = gxe[b][t] + z . W_z^T (nz FMAs per gate, hoisted out of the time loop) + h . W_hh^T: each wave owns whole
//                16-unit blocks and computes the four gates of a block with the same accumulator layout, so the cell update is
//                lane-local and c never leaves registers; h goes to LDS (double-buffered) as the next MFMA A operand;
//       logits = h . pred_linear^T in 16-column tiles (waves interleaved), folded at once into a per-lane online log-sum-exp;
//                the target column's value is picked out of its tile.  No logit is ever written to memory.
//     NLL per token = LSE - logit[x_{t+1}], every position counted (pads included: the loss weight is all ones);
//     the sum over t runs in order in one thread per sample.  Every reduction has a fixed order (shuffle trees, waves merged
//     0..3): no atomics, repeated runs are bit-identical.
//     Envelope (lv_dec_cond_ll_f32_supported): H <= 128 (hidden padded to Hp in {16, 32, 64, 128}: the A fragments of h
//     stay in registers, 2 x 16 x Hp floats of LDS; Hp = 256 spills), 1 <= nz <= 64, any V and ni, any T >= 2 (nothing but
//     the gxe workspace grows with T); B * ceil(K/16) workgroups.  Toy shape (V 1004, ni = H = 50, nz 1): Hp 64, 102 VGPRs,
//     12.9 KB LDS, no scratch.
// (b) lv_grid_posterior_f32: joint_k = log N(z_k; 0, I) + cond_ll[b][k], log_post = joint - LSE_k(joint) (max-shifted, as
//     modules/utils.py:3-16), mean[b][d] = sum_k exp(log_post_k) z_kd.  One workgroup per sentence, fixed-order block sums.
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

// main launch: grid = B * ceil(K / 16), 256 threads; NKC = Hp / 16 (1, 2, 4, 8)
template <int NKC>
__global__ __launch_bounds__(256) void gp_cond_ll_kernel(const int64_t* __restrict__ x, int T, const float* __restrict__ z,
                                                         long z_stride, int K, const float* __restrict__ ws,
                                                         float* __restrict__ cond_ll, int B, int V, int H, int nz) {
    constexpr int HP = NKC * 16;
    constexpr int UBW = (NKC + 3) / 4;                      // 16-unit blocks per wave
    __shared__ __attribute__((aligned(16))) float hbuf[2][GP_S][HP];
    __shared__ float zs[GP_S][GP_MAXNZ];
    __shared__ float red_m[4][GP_S], red_s[4][GP_S], tl[GP_S];

    const int Td = T - 1, vt_n = (V + 15) / 16, nzp = (nz + 3) / 4 * 4;
    const GpLayout L = gp_layout(V, H, nz, B, Td);
    const float* __restrict__ whh = ws + L.whh;
    const float* __restrict__ pred = ws + L.pred;
    const float* __restrict__ wz = ws + L.wz;
    const float* __restrict__ tr = ws + L.tr;
    const float* __restrict__ gxe = ws + L.gxe;

    const int ntile = (K + GP_S - 1) / GP_S;
    const int b = (int)blockIdx.x / ntile, s0 = ((int)blockIdx.x % ntile) * GP_S;
    const int tid = (int)threadIdx.x, w = tid >> 6, l = tid & 63, lc = l & 15, lq = l >> 4;

    for (int i = tid; i < GP_S * nz; i += 256) {
        const int s = i / nz, d = i % nz;
        zs[s][d] = s0 + s < K ? z[(long)b * z_stride + (long)(s0 + s) * nz + d] : 0.f;
    }
    __syncthreads();

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
            for (int d = 0; d < nz; ++d) a += zs[s][d] * tr[(long)u * nzp + d];
            c[j][r] = a;
            hbuf[0][s][u] = tanhf(a);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float q = 0.f;
                for (int d = 0; d < nz; ++d) q += zs[s][d] * wz[((long)g * HP + u) * nzp + d];
                zp[j][g][r] = q;
            }
        }
    }
    float nll = 0.f;                                         // thread tid < 16: sample tid's running NLL
    __syncthreads();

    for (int t = 0; t < Td; ++t) {
        const float(*hin)[HP] = hbuf[t & 1];
        float(*hout)[HP] = hbuf[(t & 1) ^ 1];
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
                    for (int r = 0; r < 4; ++r) tl[lq * 4 + r] = acc[r];
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
            if (lc == 0) { red_m[w][lq * 4 + r] = m[r]; red_s[w][lq * 4 + r] = sm[r]; }
        }
        __syncthreads();
        if (tid < GP_S) {
            float M = red_m[0][tid], S = red_s[0][tid];
            for (int i = 1; i < 4; ++i) gp_lse_merge(M, S, red_m[i][tid], red_s[i][tid]);
            nll += (M + logf(S)) - tl[tid];
        }
        // (the next gates phase writes the other h buffer and the next red / tl writes follow its barrier)
    }
    if (tid < GP_S && s0 + tid < K) cond_ll[(long)b * K + s0 + tid] = -nll;
}

// fixed-order block sum / max over 256 threads (4 waves); red: 4 floats of LDS
__device__ __forceinline__ float gp_block_sum(float v, float* red) {
    v = lv_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float gp_block_max(float v, float* red) {
    v = lv_wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ float gp_joint(const float* __restrict__ cond, const float* __restrict__ zb, int k, int nz) {
    const float* zk = zb + (long)k * nz;
    float q = 0.f;
    for (int d = 0; d < nz; ++d) q += zk[d] * zk[d];
    return (-0.5f * q - 0.5f * ((float)nz * GP_LOG_2PI)) + cond[k];
}

// one workgroup per sentence
__global__ __launch_bounds__(256) void gp_normalise_kernel(const float* __restrict__ cond_ll, const float* __restrict__ z,
                                                           long z_stride, int K, int nz, float* __restrict__ log_post,
                                                           float* __restrict__ mean) {
    __shared__ float red[4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float* cond = cond_ll + (long)b * K;
    const float* zb = z + (long)b * z_stride;
    float mx = -INFINITY;
    for (int k = tid; k < K; k += 256) mx = fmaxf(mx, gp_joint(cond, zb, k, nz));
    mx = gp_block_max(mx, red);
    float se = 0.f;
    for (int k = tid; k < K; k += 256) se += expf(gp_joint(cond, zb, k, nz) - mx);
    const float lse = mx + logf(gp_block_sum(se, red));
    if (log_post) {
        for (int k = tid; k < K; k += 256) log_post[(long)b * K + k] = gp_joint(cond, zb, k, nz) - lse;
    }
    for (int d = 0; d < nz; ++d) {
        float a = 0.f;
        for (int k = tid; k < K; k += 256) a += expf(gp_joint(cond, zb, k, nz) - lse) * zb[(long)k * nz + d];
        a = gp_block_sum(a, red);
        if (tid == 0) mean[(long)b * nz + d] = a;
    }
}

}  // namespace

extern "C" int lv_dec_cond_ll_f32_supported(int V, int ni, int H, int nz, int T) {
    return V >= 1 && ni >= 1 && H >= 1 && H <= GP_MAXH && nz >= 1 && nz <= GP_MAXNZ && T >= 2 ? 1 : 0;
}

extern "C" long lv_dec_cond_ll_f32_ws_floats(int V, int H, int nz, int B, int T) {
    if (V < 1 || H < 1 || nz < 1 || B < 1 || T < 2) return 0;
    return gp_layout(V, H, nz, B, T - 1).total;
}

// log p(x_b | z_{b,s}) of LSTMDecoder.log_probability (dec_lstm.py:66-148, 156-161) in eval mode for x [B][T] and K samples
// per sentence at z + b*z_stride ([K][nz]; z_stride = 0: one shared grid); ws: lv_dec_cond_ll_f32_ws_floats(V, H, nz, B, T)
// floats, 16-byte aligned; cond_ll [B][K]
extern "C" int lv_dec_cond_ll_f32(const int64_t* x, int B, int T, const float* z, long z_stride, int K, const float* embed,
                                  const float* trans, const float* w_ih, const float* w_hh, const float* b_ih,
                                  const float* b_hh, const float* pred, int V, int ni, int H, int nz, float* ws,
                                  float* cond_ll, void* stream) {
    if (!x || !z || !embed || !trans || !w_ih || !w_hh || !b_ih || !b_hh || !pred || !ws || !cond_ll) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || z_stride < 0 || (z_stride > 0 && z_stride < (long)K * nz)) return LV_ERR_SHAPE;
    if (!lv_dec_cond_ll_f32_supported(V, ni, H, nz, T)) return LV_ERR_UNSUPPORTED;
    if (((uintptr_t)ws & 15) != 0) return LV_ERR_ALIGN;
    const long total = lv_dec_cond_ll_f32_ws_floats(V, H, nz, B, T);
    LV_LAUNCH(gp_prep_kernel, dim3((unsigned)lv_cdiv(total < 256L * 4096 ? total : 256L * 4096, 256)), dim3(256), 0, stream,
              x, T, embed, trans, w_ih, w_hh, b_ih, b_hh, pred, ws, B, V, ni, H, nz);
    const long blocks = (long)B * ((K + GP_S - 1) / GP_S);
    if (blocks > 0x7fffffffL) return LV_ERR_SHAPE;
    const dim3 grid((unsigned)blocks);
    switch (gp_hp(H)) {
        case 16: LV_LAUNCH(gp_cond_ll_kernel<1>, grid, dim3(256), 0, stream, x, T, z, z_stride, K, (const float*)ws, cond_ll, B, V, H, nz); break;
        case 32: LV_LAUNCH(gp_cond_ll_kernel<2>, grid, dim3(256), 0, stream, x, T, z, z_stride, K, (const float*)ws, cond_ll, B, V, H, nz); break;
        case 64: LV_LAUNCH(gp_cond_ll_kernel<4>, grid, dim3(256), 0, stream, x, T, z, z_stride, K, (const float*)ws, cond_ll, B, V, H, nz); break;
        default: LV_LAUNCH(gp_cond_ll_kernel<8>, grid, dim3(256), 0, stream, x, T, z, z_stride, K, (const float*)ws, cond_ll, B, V, H, nz); break;
    }
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// the grid normalisation of VAE.eval_log_model_posterior / calc_model_posterior_mean (vae.py:170-196, 256-273): cond_ll [B][K],
// z at z + b*z_stride ([K][nz]; 0 = shared grid) -> log_post [B][K] (may be NULL), mean [B][nz]
extern "C" int lv_grid_posterior_f32(const float* cond_ll, const float* z, long z_stride, int B, int K, int nz, float* log_post,
                                     float* mean, void* stream) {
    if (!cond_ll || !z || !mean) return LV_ERR_ARG;
    if (B <= 0 || K <= 0 || nz <= 0 || z_stride < 0 || (z_stride > 0 && z_stride < (long)K * nz)) return LV_ERR_SHAPE;
    LV_LAUNCH(gp_normalise_kernel, dim3((unsigned)B), dim3(256), 0, stream, cond_ll, z, z_stride, K, nz, log_post, mean);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
