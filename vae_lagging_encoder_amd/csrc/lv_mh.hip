// lv_mh.hip -- random-walk Metropolis-Hastings sampling from the model posterior p(z|x) (VAE.sample_from_posterior,
// modules/vae.py:218-254): a chain started at a draw from q(z|x), proposals next = eps * std + cur, scored by
// log p(z, x) = log N(z; 0, I) + log p(x|z), accepted where u < min(exp(next_ll - cur_ll), 1).
//
// (a) lv_mh_chain_f32: the fused route for the eval-mode LSTM decoder inside lv_dec_cond_ll_f32's envelope (H <= 128,
//     nz <= 64, any V / ni, T >= 2).  One workgroup owns one sentence and a tile of up to 16 chains (the 16 MFMA rows of
//     gp_cond_nll, lv_cond_ll.h: 16 independent chains of the same sentence) and runs n_iter consecutive iterations inside
//     the launch: form the 16 proposals, score them (c0, h0, the z half of the gates, the T - 1 timesteps -- the code of the
//     grid kernel, bit for bit), add the prior term, decide, select, count, store a kept sample when one is due.  No
//     hand-off between workgroups, no atomics, every reduction in a fixed order: repeated runs are bit-identical, and a chain
//     does not depend on which other chains share its tile.  cur / cur_ll / the acceptance counts live in caller-owned
//     buffers, read at the start of a launch and written at its end, so a chain can be cut into several launches with the
//     same result; `first` makes a launch score the starting point before its first proposal.  The weight images and the
//     per-sentence input projection are lv_mh_chain_prep_f32: once per chain, not per launch or iteration.
// (b) lv_mh_step_f32: the propose / accept glue for every other decoder, one launch per iteration and no host read: given
//     cond_ll [rows] of the current proposals it adds the prior term, decides, selects cur / cur_ll, counts, stores a kept
//     sample when due and overwrites the proposals with those of the next iteration; init mode scores the starting point
//     and writes the first proposals.  Any nz >= 1.
// Both take their noise as buffers (eps standard normal, u uniform in [0, 1)): the kernels hold no generator.  One accept
// rule (lv_cond_ll.h): select, never blend -- a proposal that scores NaN is rejected and leaves cur_ll as it was, where
// the reference's mask * next + (1 - mask) * cur would turn cur_ll into NaN for good.
#include "lv_cond_ll.h"

namespace {

// grid = B * ceil(C / 16), 256 threads; NKC = Hp / 16.  eps [n_iter][B][C][nz], u [n_iter][B][C] (this launch's slices),
// samples [B][nsamples][C][nz]; ratio_out / accept_out [n_iter][B][C] or NULL.
template <int NKC>
__global__ __launch_bounds__(256) void mh_chain_kernel(const int64_t* __restrict__ x, int T, const float* __restrict__ ws,
                                                       int B, int V, int H, int nz, int C, float* __restrict__ cur,
                                                       float* __restrict__ cur_ll, int* __restrict__ accepts,
                                                       const float* __restrict__ eps, const float* __restrict__ u,
                                                       int n_iter, int iter0, int burn_in, int thin, int nsamples, float std,
                                                       int first, float* __restrict__ samples, float* __restrict__ ratio_out,
                                                       int* __restrict__ accept_out) {
    __shared__ GpShared<NKC> sh;
    __shared__ float curz[GP_S][GP_MAXNZ];
    const int ntile = (C + GP_S - 1) / GP_S;
    const int b = (int)blockIdx.x / ntile, s0 = ((int)blockIdx.x % ntile) * GP_S;
    const int tid = (int)threadIdx.x;
    const bool mine = tid < GP_S && s0 + tid < C;           // this thread keeps chain s0 + tid
    const long row = (long)b * C + s0 + tid;                // ... whose state sits at this row of cur / cur_ll / accepts

    for (int i = tid; i < GP_S * nz; i += 256) {
        const int s = i / nz, d = i % nz;
        const float v = s0 + s < C ? cur[((long)b * C + s0 + s) * nz + d] : 0.f;
        curz[s][d] = v;
        sh.zs[s][d] = v;
    }
    float ll = 0.f;
    int cnt = 0;
    if (mine && !first) { ll = cur_ll[row]; cnt = accepts[row]; }
    __syncthreads();
    if (first) {                                            // score the starting point
        const float nll = gp_cond_nll<NKC>(sh, x, T, b, ws, B, V, H, nz);
        if (mine) ll = gp_log_joint(curz[tid], nz, -nll);
        __syncthreads();                                    // (sh.zs is rewritten below)
    }
    for (int it = 0; it < n_iter; ++it) {
        const float* e = eps + ((long)it * B + b) * C * nz;
        for (int i = tid; i < GP_S * nz; i += 256) {
            const int s = i / nz, d = i % nz;
            sh.zs[s][d] = s0 + s < C ? mh_propose(e[(long)(s0 + s) * nz + d], std, curz[s][d]) : 0.f;
        }
        __syncthreads();
        const float nll = gp_cond_nll<NKC>(sh, x, T, b, ws, B, V, H, nz);
        if (mine) {
            const float next_ll = gp_log_joint(sh.zs[tid], nz, -nll);
            const float ratio = next_ll - ll;
            const long ri = ((long)it * B + b) * C + s0 + tid;
            const bool acc = mh_accept(ratio, u[ri]);
            if (acc) {
                for (int d = 0; d < nz; ++d) curz[tid][d] = sh.zs[tid][d];
                ll = next_ll;
                ++cnt;
            }
            if (ratio_out) ratio_out[ri] = ratio;
            if (accept_out) accept_out[ri] = acc ? 1 : 0;
            const int k = mh_keep_index(iter0 + it, burn_in, thin, nsamples);
            if (k >= 0) {
                float* dst = samples + (((long)b * nsamples + k) * C + s0 + tid) * nz;
                for (int d = 0; d < nz; ++d) dst[d] = curz[tid][d];
            }
        }
        __syncthreads();                                    // curz and sh.zs are settled before the next proposals
    }
    if (mine) {
        for (int d = 0; d < nz; ++d) cur[row * nz + d] = curz[tid][d];
        cur_ll[row] = ll;
        accepts[row] = cnt;
    }
}

// one thread per row (chain); prop [rows][nz]: the proposals cond_ll was computed at (init: ignored on entry), replaced by
// the next iteration's; samples [rows / C][nsamples][C][nz]
__global__ __launch_bounds__(256) void mh_step_kernel(const float* __restrict__ cond_ll, float* __restrict__ prop,
                                                      float* __restrict__ cur, float* __restrict__ cur_ll,
                                                      int* __restrict__ accepts, const float* __restrict__ u,
                                                      const float* __restrict__ eps_next, float std,
                                                      float* __restrict__ samples, int rows, int C, int nz, int nsamples,
                                                      int keep, int init, float* __restrict__ ratio_out,
                                                      int* __restrict__ accept_out) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float* cz = cur + r * nz;
    float* pz = prop + r * nz;
    if (init) {
        cur_ll[r] = gp_log_joint(cz, nz, cond_ll[r]);
        accepts[r] = 0;
    } else {
        const float next_ll = gp_log_joint(pz, nz, cond_ll[r]);
        const float ratio = next_ll - cur_ll[r];
        const bool acc = mh_accept(ratio, u[r]);
        if (acc) {
            for (int d = 0; d < nz; ++d) cz[d] = pz[d];
            cur_ll[r] = next_ll;
            accepts[r] += 1;
        }
        if (ratio_out) ratio_out[r] = ratio;
        if (accept_out) accept_out[r] = acc ? 1 : 0;
        if (keep >= 0) {
            float* dst = samples + (((r / C) * nsamples + keep) * C + r % C) * nz;
            for (int d = 0; d < nz; ++d) dst[d] = cz[d];
        }
    }
    if (eps_next) {
        const float* e = eps_next + r * nz;
        for (int d = 0; d < nz; ++d) pz[d] = mh_propose(e[d], std, cz[d]);
    }
}

}  // namespace

// the envelope of lv_mh_chain_f32: that of lv_dec_cond_ll_f32 (lv_grid_posterior.hip)
extern "C" int lv_mh_chain_f32_supported(int V, int ni, int H, int nz, int T) {
    return V >= 1 && ni >= 1 && H >= 1 && H <= GP_MAXH && nz >= 1 && nz <= GP_MAXNZ && T >= 2 ? 1 : 0;
}

extern "C" long lv_mh_chain_f32_ws_floats(int V, int H, int nz, int B, int T) {
    if (V < 1 || H < 1 || nz < 1 || B < 1 || T < 2) return 0;
    return gp_layout(V, H, nz, B, T - 1).total;
}

// once per chain: the weight images and the per-sentence input projection of x [B][T] into ws
// (lv_mh_chain_f32_ws_floats(V, H, nz, B, T) floats, 16-byte aligned); weights as LSTMDecoder stores them
extern "C" int lv_mh_chain_prep_f32(const int64_t* x, int B, int T, const float* embed, const float* trans, const float* w_ih,
                                    const float* w_hh, const float* b_ih, const float* b_hh, const float* pred, int V, int ni,
                                    int H, int nz, float* ws, void* stream) {
    if (!x || !embed || !trans || !w_ih || !w_hh || !b_ih || !b_hh || !pred || !ws) return LV_ERR_ARG;
    if (B <= 0) return LV_ERR_SHAPE;
    if (!lv_mh_chain_f32_supported(V, ni, H, nz, T)) return LV_ERR_UNSUPPORTED;
    if (((uintptr_t)ws & 15) != 0) return LV_ERR_ALIGN;
    gp_launch_prep(x, B, T, embed, trans, w_ih, w_hh, b_ih, b_hh, pred, V, ni, H, nz, ws, stream);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// n_iter iterations (global indices iter0 .. iter0 + n_iter - 1) of C chains per sentence of VAE.sample_from_posterior
// (vae.py:218-254); see the top of this file
extern "C" int lv_mh_chain_f32(const int64_t* x, int B, int T, const float* ws, int V, int H, int nz, int C, float* cur,
                               float* cur_ll, int* accepts, const float* eps, const float* u, int n_iter, int iter0,
                               int burn_in, int thin, int nsamples, float std, int first, float* samples, float* ratio_out,
                               int* accept_out, void* stream) {
    if (!x || !ws || !cur || !cur_ll || !accepts || !samples || (n_iter > 0 && (!eps || !u))) return LV_ERR_ARG;
    if (B <= 0 || C <= 0 || n_iter < 0 || iter0 < 0 || burn_in < 0 || thin < 1 || nsamples < 1) return LV_ERR_SHAPE;
    if (!lv_mh_chain_f32_supported(V, 1, H, nz, T)) return LV_ERR_UNSUPPORTED;
    if (((uintptr_t)ws & 15) != 0) return LV_ERR_ALIGN;
    const long blocks = (long)B * ((C + GP_S - 1) / GP_S);
    if (blocks > 0x7fffffffL) return LV_ERR_SHAPE;
    if (n_iter == 0 && !first) return LV_OK;
    const dim3 grid((unsigned)blocks);
#define MH_CHAIN_ARGS x, T, ws, B, V, H, nz, C, cur, cur_ll, accepts, eps, u, n_iter, iter0, burn_in, thin, nsamples, std, first, samples, ratio_out, accept_out
    switch (gp_hp(H)) {
        case 16: LV_LAUNCH(mh_chain_kernel<1>, grid, dim3(256), 0, stream, MH_CHAIN_ARGS); break;
        case 32: LV_LAUNCH(mh_chain_kernel<2>, grid, dim3(256), 0, stream, MH_CHAIN_ARGS); break;
        case 64: LV_LAUNCH(mh_chain_kernel<4>, grid, dim3(256), 0, stream, MH_CHAIN_ARGS); break;
        default: LV_LAUNCH(mh_chain_kernel<8>, grid, dim3(256), 0, stream, MH_CHAIN_ARGS); break;
    }
#undef MH_CHAIN_ARGS
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// one iteration's propose / accept glue for rows = B * C chains (vae.py:232-251), or with init != 0 the scoring of the
// starting point (vae.py:227-228); see the top of this file.  keep: index of the kept sample this iteration produces, -1: none
extern "C" int lv_mh_step_f32(const float* cond_ll, float* prop, float* cur, float* cur_ll, int* accepts, const float* u,
                              const float* eps_next, float std, float* samples, int rows, int C, int nz, int nsamples, int keep,
                              int init, float* ratio_out, int* accept_out, void* stream) {
    if (!cond_ll || !prop || !cur || !cur_ll || !accepts || (!init && !u) || (!init && keep >= 0 && !samples)) return LV_ERR_ARG;
    if (rows <= 0 || C <= 0 || rows % C != 0 || nz <= 0 || nsamples < 1 || keep < -1 || keep >= nsamples) return LV_ERR_SHAPE;
    LV_LAUNCH(mh_step_kernel, dim3((unsigned)lv_cdiv(rows, 256)), dim3(256), 0, stream, cond_ll, prop, cur, cur_ll, accepts, u,
              eps_next, std, samples, rows, C, nz, nsamples, keep, init, ratio_out, accept_out);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
