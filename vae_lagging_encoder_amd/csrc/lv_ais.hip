// lv_ais.hip -- annealed importance sampling of log p(x) (Neal 2001; Wu et al. 2017): VAE.nll_ais.  The transitions are the
// random-walk Metropolis kernel of lv_mh.hip (reference modules/vae.py:218-254), run on the annealed target
// q0(z)^(1 - beta) * p(z, x)^beta, and every chain carries a running log-weight.  For a sentence x and chain c:
//
//   q0      = N(mu0, diag exp(lv0)); mu0 == NULL: the prior N(0, I)
//   g(z)    = (log p(z) - log q0(z)) + log p(x|z)             float32; with the prior as q0 the pair is skipped: g = log p(x|z)
//   z_0     ~ q0,  logw = 0 (float64)
//   for i = 1..N:
//       logw += (beta_i - beta_{i-1}) * (double) g(cur)        float64 accumulate, beta a float64 array
//       next  = eps_i * std_i + cur                            mh_propose: rounded product, then rounded sum
//       ratio = [log q0(next) + (float)beta_i * g(next)] - [log q0(cur) + (float)beta_i * g(cur)]
//       accept = ratio >= 0 || u_i < expf(ratio)               mh_accept: select, never blend; a NaN ratio rejects
//   log p^(x) = logsumexp_c logw_c - log C
//
// State per chain, in caller-owned buffers: cur [nz], g(cur), log q0(cur) (float32), logw (float64), the accept count.
// (a) lv_ais_chain_f32: sibling of mh_chain_kernel -- one workgroup per (sentence, 16 chains), n_iter iterations per launch,
//     lv_mh_chain_prep_f32's workspace unchanged; no hand-off between workgroups, no atomics, every reduction in a fixed order:
//     repeated runs are bit-identical, a chain does not depend on its tile neighbours or on where the chain is cut into launches.
// (b) lv_ais_step_f32: sibling of mh_step_kernel -- the glue for every other decoder, one thread per chain, one launch per
//     iteration: decide iteration i from cond_ll of its proposals, then form iteration i + 1's proposals and apply iteration
//     i + 1's log-weight increment (which needs only the state just selected).
// Both take their noise as buffers; the kernels hold no generator.
#include "lv_cond_ll.h"

namespace {

// log N(z; mu, diag exp(lv)) = -0.5 sum_d (z_d - mu_d)^2 exp(-lv_d) - 0.5 (nz log 2 pi + sum_d lv_d); prior: N(0, I), the
// bits of gp_log_joint's prior term (mu, iv unread, lvsum 0).  IVREADY: iv holds exp(-lv) already (the chain kernel's LDS
// copy), else iv is lv itself.
template <bool IVREADY>
__device__ __forceinline__ float ais_log_normal(const float* __restrict__ z, int nz, bool prior,
                                                const float* __restrict__ mu, const float* __restrict__ iv, float lvsum) {
    float q = 0.f;
    if (!prior) {
        for (int d = 0; d < nz; ++d) {
            const float dv = z[d] - mu[d];
            q += (dv * dv) * (IVREADY ? iv[d] : expf(-iv[d]));
        }
    } else {
        for (int d = 0; d < nz; ++d) q += z[d] * z[d];
    }
    return -0.5f * q - 0.5f * ((float)nz * GP_LOG_2PI + lvsum);
}

// g(z) from cond = log p(x|z) and lq0 = log q0(z); with the prior as q0 the pair log p(z) - log q0(z) is exactly 0: skipped
__device__ __forceinline__ float ais_g(const float* __restrict__ z, int nz, bool prior, float lq0, float cond) {
    if (prior) return cond;
    return (ais_log_normal<true>(z, nz, true, nullptr, nullptr, 0.f) - lq0) + cond;
}

__device__ __forceinline__ float ais_ratio(float lq_next, float g_next, float lq_cur, float g_cur, float beta) {
    return (lq_next + beta * g_next) - (lq_cur + beta * g_cur);
}

// grid = B * ceil(C / 16), 256 threads; NKC = Hp / 16.  eps [n_iter][B][C][nz], u [n_iter][B][C], beta [n_iter + 1] (beta[it]
// precedes local iteration it, beta[it + 1] is its temperature), std_it [n_iter]; mu0 / lv0 [B][nz] or both NULL;
// ratio_out / accept_out / logw_out [n_iter][B][C] or NULL.
template <int NKC>
__global__ __launch_bounds__(256) void ais_chain_kernel(const int64_t* __restrict__ x, int T, const float* __restrict__ ws,
                                                        int B, int V, int H, int nz, int C, float* __restrict__ cur,
                                                        float* __restrict__ g_cur, float* __restrict__ lq_cur,
                                                        double* __restrict__ logw, int* __restrict__ accepts,
                                                        const float* __restrict__ eps, const float* __restrict__ u,
                                                        const double* __restrict__ beta, const float* __restrict__ std_it,
                                                        const float* __restrict__ mu0, const float* __restrict__ lv0,
                                                        int n_iter, int first, float* __restrict__ ratio_out,
                                                        int* __restrict__ accept_out, double* __restrict__ logw_out) {
    __shared__ GpShared<NKC> sh;
    __shared__ float curz[GP_S][GP_MAXNZ];
    __shared__ float q0mu[GP_MAXNZ], q0iv[GP_MAXNZ];
    const int ntile = (C + GP_S - 1) / GP_S;
    const int b = (int)blockIdx.x / ntile, s0 = ((int)blockIdx.x % ntile) * GP_S;
    const int tid = (int)threadIdx.x;
    const bool mine = tid < GP_S && s0 + tid < C;           // this thread keeps chain s0 + tid
    const long row = (long)b * C + s0 + tid;                // ... whose state sits at this row of the state buffers
    const bool prior = mu0 == nullptr;

    for (int i = tid; i < GP_S * nz; i += 256) {
        const int s = i / nz, d = i % nz;
        const float v = s0 + s < C ? cur[((long)b * C + s0 + s) * nz + d] : 0.f;
        curz[s][d] = v;
        sh.zs[s][d] = v;
    }
    float lvsum = 0.f;
    if (!prior) {
        if (tid < nz) { q0mu[tid] = mu0[(long)b * nz + tid]; q0iv[tid] = expf(-lv0[(long)b * nz + tid]); }
        if (mine)
            for (int d = 0; d < nz; ++d) lvsum += lv0[(long)b * nz + d];
    }
    float g = 0.f, lq = 0.f;
    double lw = 0.0;
    int cnt = 0;
    if (mine && !first) { g = g_cur[row]; lq = lq_cur[row]; lw = logw[row]; cnt = accepts[row]; }
    __syncthreads();
    if (first) {                                            // score the starting point
        const float nll = gp_cond_nll<NKC>(sh, x, T, b, ws, B, V, H, nz);
        if (mine) {
            lq = ais_log_normal<true>(curz[tid], nz, prior, q0mu, q0iv, lvsum);
            g = ais_g(curz[tid], nz, prior, lq, -nll);
        }
        __syncthreads();                                    // (sh.zs is rewritten below)
    }
    for (int it = 0; it < n_iter; ++it) {
        const float* e = eps + ((long)it * B + b) * C * nz;
        const float std = std_it[it];
        for (int i = tid; i < GP_S * nz; i += 256) {
            const int s = i / nz, d = i % nz;
            sh.zs[s][d] = s0 + s < C ? mh_propose(e[(long)(s0 + s) * nz + d], std, curz[s][d]) : 0.f;
        }
        __syncthreads();
        const float nll = gp_cond_nll<NKC>(sh, x, T, b, ws, B, V, H, nz);
        if (mine) {
            const long ri = ((long)it * B + b) * C + s0 + tid;
            const double bi = beta[it + 1];
            lw += (bi - beta[it]) * (double)g;
            if (logw_out) logw_out[ri] = lw;
            const float lq_next = ais_log_normal<true>(sh.zs[tid], nz, prior, q0mu, q0iv, lvsum);
            const float g_next = ais_g(sh.zs[tid], nz, prior, lq_next, -nll);
            const float ratio = ais_ratio(lq_next, g_next, lq, g, (float)bi);
            const bool acc = mh_accept(ratio, u[ri]);
            if (acc) {
                for (int d = 0; d < nz; ++d) curz[tid][d] = sh.zs[tid][d];
                g = g_next;
                lq = lq_next;
                ++cnt;
            }
            if (ratio_out) ratio_out[ri] = ratio;
            if (accept_out) accept_out[ri] = acc ? 1 : 0;
        }
        __syncthreads();                                    // curz and sh.zs are settled before the next proposals
    }
    if (mine) {
        for (int d = 0; d < nz; ++d) cur[row * nz + d] = curz[tid][d];
        g_cur[row] = g;
        lq_cur[row] = lq;
        logw[row] = lw;
        accepts[row] = cnt;
    }
}

// one thread per row (chain); prop [rows][nz]: the proposals cond_ll was computed at (init: cond_ll was computed at cur and
// prop is ignored on entry), replaced by the next iteration's
__global__ __launch_bounds__(256) void ais_step_kernel(const float* __restrict__ cond_ll, float* __restrict__ prop,
                                                       float* __restrict__ cur, float* __restrict__ g_cur,
                                                       float* __restrict__ lq_cur, double* __restrict__ logw,
                                                       int* __restrict__ accepts, const float* __restrict__ u, double beta,
                                                       const float* __restrict__ eps_next, float std_next, double dbeta_next,
                                                       const float* __restrict__ mu0, const float* __restrict__ lv0, int rows,
                                                       int C, int nz, int init, float* __restrict__ ratio_out,
                                                       int* __restrict__ accept_out, double* __restrict__ logw_out_next) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float* cz = cur + r * nz;
    float* pz = prop + r * nz;
    const bool prior = mu0 == nullptr;
    const float* mu = prior ? nullptr : mu0 + (r / C) * nz;
    const float* lv = prior ? nullptr : lv0 + (r / C) * nz;
    float lvsum = 0.f;
    if (!prior)
        for (int d = 0; d < nz; ++d) lvsum += lv[d];
    float g, lq;
    double lw;
    if (init) {
        lq = ais_log_normal<false>(cz, nz, prior, mu, lv, lvsum);
        g = ais_g(cz, nz, prior, lq, cond_ll[r]);
        lw = 0.0;
        g_cur[r] = g;
        lq_cur[r] = lq;
        accepts[r] = 0;
    } else {
        g = g_cur[r];
        lq = lq_cur[r];
        lw = logw[r];
        const float lq_next = ais_log_normal<false>(pz, nz, prior, mu, lv, lvsum);
        const float g_next = ais_g(pz, nz, prior, lq_next, cond_ll[r]);
        const float ratio = ais_ratio(lq_next, g_next, lq, g, (float)beta);
        const bool acc = mh_accept(ratio, u[r]);
        if (acc) {
            for (int d = 0; d < nz; ++d) cz[d] = pz[d];
            g = g_next;
            lq = lq_next;
            g_cur[r] = g;
            lq_cur[r] = lq;
            accepts[r] += 1;
        }
        if (ratio_out) ratio_out[r] = ratio;
        if (accept_out) accept_out[r] = acc ? 1 : 0;
    }
    if (eps_next) {                                         // iteration i + 1: its increment and its proposals
        lw += dbeta_next * (double)g;
        if (logw_out_next) logw_out_next[r] = lw;
        const float* e = eps_next + r * nz;
        for (int d = 0; d < nz; ++d) pz[d] = mh_propose(e[d], std_next, cz[d]);
    }
    if (init || eps_next) logw[r] = lw;
}

}  // namespace

// the envelope of lv_ais_chain_f32: that of lv_mh_chain_f32 (all four instantiations fit the registers: DESIGN.md 3.1.2)
extern "C" int lv_ais_chain_f32_supported(int V, int ni, int H, int nz, int T) {
    return V >= 1 && ni >= 1 && H >= 1 && H <= GP_MAXH && nz >= 1 && nz <= GP_MAXNZ && T >= 2 ? 1 : 0;
}

// n_iter annealed iterations of C chains per sentence; see the top of this file.  ws: lv_mh_chain_prep_f32's, unchanged
extern "C" int lv_ais_chain_f32(const int64_t* x, int B, int T, const float* ws, int V, int H, int nz, int C, float* cur,
                                float* g_cur, float* lq_cur, double* logw, int* accepts, const float* eps, const float* u,
                                const double* beta, const float* std_it, const float* mu0, const float* lv0, int n_iter,
                                int first, float* ratio_out, int* accept_out, double* logw_out, void* stream) {
    if (!x || !ws || !cur || !g_cur || !lq_cur || !logw || !accepts || (n_iter > 0 && (!eps || !u || !beta || !std_it)) ||
        (mu0 == nullptr) != (lv0 == nullptr))
        return LV_ERR_ARG;
    if (B <= 0 || C <= 0 || n_iter < 0) return LV_ERR_SHAPE;
    if (!lv_ais_chain_f32_supported(V, 1, H, nz, T)) return LV_ERR_UNSUPPORTED;
    if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)logw & 7) != 0 || ((uintptr_t)beta & 7) != 0 || ((uintptr_t)logw_out & 7) != 0)
        return LV_ERR_ALIGN;
    const long blocks = (long)B * ((C + GP_S - 1) / GP_S);
    if (blocks > 0x7fffffffL) return LV_ERR_SHAPE;
    if (n_iter == 0 && !first) return LV_OK;
    const dim3 grid((unsigned)blocks);
#define AIS_CHAIN_ARGS x, T, ws, B, V, H, nz, C, cur, g_cur, lq_cur, logw, accepts, eps, u, beta, std_it, mu0, lv0, n_iter, first, ratio_out, accept_out, logw_out
    switch (gp_hp(H)) {
        case 16: LV_LAUNCH(ais_chain_kernel<1>, grid, dim3(256), 0, stream, AIS_CHAIN_ARGS); break;
        case 32: LV_LAUNCH(ais_chain_kernel<2>, grid, dim3(256), 0, stream, AIS_CHAIN_ARGS); break;
        case 64: LV_LAUNCH(ais_chain_kernel<4>, grid, dim3(256), 0, stream, AIS_CHAIN_ARGS); break;
        default: LV_LAUNCH(ais_chain_kernel<8>, grid, dim3(256), 0, stream, AIS_CHAIN_ARGS); break;
    }
#undef AIS_CHAIN_ARGS
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// one iteration's glue for rows = B * C chains of any decoder, or with init != 0 the scoring of z_0; see the top of this file
extern "C" int lv_ais_step_f32(const float* cond_ll, float* prop, float* cur, float* g_cur, float* lq_cur, double* logw,
                               int* accepts, const float* u, double beta, const float* eps_next, float std_next,
                               double dbeta_next, const float* mu0, const float* lv0, int rows, int C, int nz, int init,
                               float* ratio_out, int* accept_out, double* logw_out_next, void* stream) {
    if (!cond_ll || !prop || !cur || !g_cur || !lq_cur || !logw || !accepts || (!init && !u) ||
        (mu0 == nullptr) != (lv0 == nullptr))
        return LV_ERR_ARG;
    if (rows <= 0 || C <= 0 || rows % C != 0 || nz <= 0) return LV_ERR_SHAPE;
    if (((uintptr_t)logw & 7) != 0 || ((uintptr_t)logw_out_next & 7) != 0) return LV_ERR_ALIGN;
    LV_LAUNCH(ais_step_kernel, dim3((unsigned)lv_cdiv(rows, 256)), dim3(256), 0, stream, cond_ll, prop, cur, g_cur, lq_cur, logw,
              accepts, u, beta, eps_next, std_next, dbeta_next, mu0, lv0, rows, C, nz, init, ratio_out, accept_out,
              logw_out_next);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
