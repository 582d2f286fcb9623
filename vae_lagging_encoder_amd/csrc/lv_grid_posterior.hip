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
#include "lv_cond_ll.h"

namespace {

// main launch: grid = B * ceil(K / 16), 256 threads; NKC = Hp / 16 (1, 2, 4, 8).  The decoder itself is gp_cond_nll of
// lv_cond_ll.h (shared with the Metropolis-Hastings chain of lv_mh.hip).
template <int NKC>
__global__ __launch_bounds__(256) void gp_cond_ll_kernel(const int64_t* __restrict__ x, int T, const float* __restrict__ z,
                                                         long z_stride, int K, const float* __restrict__ ws,
                                                         float* __restrict__ cond_ll, int B, int V, int H, int nz) {
    __shared__ GpShared<NKC> sh;
    const int ntile = (K + GP_S - 1) / GP_S;
    const int b = (int)blockIdx.x / ntile, s0 = ((int)blockIdx.x % ntile) * GP_S;
    const int tid = (int)threadIdx.x;

    for (int i = tid; i < GP_S * nz; i += 256) {
        const int s = i / nz, d = i % nz;
        sh.zs[s][d] = s0 + s < K ? z[(long)b * z_stride + (long)(s0 + s) * nz + d] : 0.f;
    }
    __syncthreads();
    const float nll = gp_cond_nll<NKC>(sh, x, T, b, ws, B, V, H, nz);
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
    return gp_log_joint(zb + (long)k * nz, nz, cond[k]);
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
    gp_launch_prep(x, B, T, embed, trans, w_ih, w_hh, b_ih, b_hh, pred, V, ni, H, nz, ws, stream);
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
