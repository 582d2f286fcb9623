// lv_iw.hip -- training on the importance-weighted bound (objective "iw"): loss_b = -(logsumexp_s log w_s - log ns) with
//   log w_s = log p(x|z_s) + beta * (log p(z_s) - log q(z_s|x)),   z_s = mu + eps_s * sigma,
// the quantity VAE.nll_iw(x, ns, ns) estimates (modules/vae.py:100-129), differentiated through the reparameterised samples.
// With log q in its eps form -- log q(z_s|x) = -1/2 sum_j eps_sj^2 - 1/2 sum_j logvar_j - (nz/2) log 2pi, exact for z = mu + eps * sigma,
// no division, no cancellation -- the 2pi terms of prior and posterior cancel:
//   log w_s = -rec_s - beta * (1/2 sum_j z_sj^2 - 1/2 sum_j eps_sj^2 - 1/2 sum_j logvar_j).
// Backward of mean_b(loss_b), g = g_loss[b], wn_s = softmax_s(log w_s):
//   d loss_b / d rec_s = wn_s            -> rowscale[b*ns + s] = g * wn_s seeds the decoder backward, which returns dz_s
//   d loss_b / d z_sj  (direct) = beta * wn_s * z_sj,   d / d logvar_j (direct) = -1/2 beta sum_s wn_s = -1/2 beta   (sum_s wn_s = 1;
//   the kernels keep the sum over c_s = beta * g * wn_s instead of the constant: an underflowed or rounded weight stays consistent)
//   dmu_j = sum_s t_sj,  dlogvar_j = sum_s t_sj * 1/2 eps_sj sigma_j - 1/2 sum_s c_s,   t_sj = dz_sj + c_s z_sj.
// lv_enc_head_iw_bwd_f32 (lv_head.hip) consumes wz = c in the fused step; lv_reparam_iw_bwd_f32 is the direct part for autograd.
//
// Estimator "dreg" (doubly reparameterised, Tucker et al. 2019): the value, rowscale and the decoder's gradient are
// the ones above; the encoder sees log q(z|x) as a function of z alone, d log w_s / d z_sj = -a_sj - beta (z_sj - eps_sj / sigma_j)
// with a_s = d rec_s / d z_s, under the coefficient u_s = (1 - beta) wn_s + beta wn_s^2 (beta = 1: wn_s^2).  With
//   r_s = u_s / wn_s = 1 - beta (1 - wn_s)       (exactly 1 at wn_s = 1, no division, wn_s = 0 harmless)
//   c'_s = beta g u_s = beta g wn_s r_s
//   t_sj = r_s dz_sj + c'_s (z_sj - eps_sj exp(-logvar_j / 2)),   dmu_j = sum_s t_sj,   dlogvar_j = sum_s t_sj 1/2 eps_sj sigma_j
// (no -1/2 term: the direct dependence on logvar is what was reparameterised away).  The dreg assemble entries write rs = r and
// wz = c'; lv_enc_head_dreg_bwd_f32 (lv_head.hip) and lv_reparam_iwdz_bwd_f32 consume them.
#include "lv_device.h"

namespace {

// One wave per SENTENCE, as loss_assemble_ns_kernel: for s = 0 .. ns-1 the wave sums nll[.][b*ns + s] over t (lanes stride over t,
// fixed-shape butterfly) and the three quadratic sums over nz (lanes stride over j); lane 0 then normalises the ns weights
// serially.  log w_s is parked in wz[b][s] and exp(log w_s - max) in rowscale[b*ns + s] between lane 0's passes (its own stores,
// read back by the same lane), so any ns works without a register array.  The normaliser is summed in double and rounded once:
// sum_s wn_s stays within a few ulp of 1 for any ns.
// DREG: rsv[b][s] = r_s is written as well and wz holds c'_s = (beta g wn_s) r_s; every other output is computed as without it.
constexpr int IW_WAVES = 16;
template <bool DREG>
__global__ __launch_bounds__(64 * IW_WAVES) void loss_assemble_iw_kernel(const float* __restrict__ nll, const float* __restrict__ mulv,
                                                                         const float* __restrict__ eps, const float* __restrict__ z,
                                                                         const float* __restrict__ kl, const float* __restrict__ klw,
                                                                         const float* __restrict__ g_loss, float* __restrict__ loss,
                                                                         float* __restrict__ rec, float* rowscale, float* wz,
                                                                         float* __restrict__ logw, float* __restrict__ rsv,
                                                                         float* __restrict__ acc, int T, int B, int ns, int nz,
                                                                         unsigned long long* rng_state, unsigned long long rng_inc) {
    __shared__ float red[3][IW_WAVES];
    const int tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    const float kw = klw[0];
    const long Bd = (long)B * ns;
    const float fns = (float)ns;
    float sl = 0.f, sr = 0.f, sk = 0.f;
    for (int b = w; b < B; b += IW_WAVES) {
        float a = 0.f;
        for (int j = l; j < nz; j += 64) a += mulv[(long)b * 2 * nz + nz + j];
        const float slv = lv_wave_sum(a);
        float tot = 0.f, mx = -INFINITY;
        for (int s = 0; s < ns; ++s) {
            const long row = (long)b * ns + s;
            a = 0.f;
            for (int t = l; t < T; t += 64) a += nll[(long)t * Bd + row];
            const float r = lv_wave_sum(a);
            float qz = 0.f, qe = 0.f;
            for (int j = l; j < nz; j += 64) {
                const float zz = z[row * nz + j], e = eps[row * nz + j];
                qz += zz * zz;
                qe += e * e;
            }
            qz = lv_wave_sum(qz);
            qe = lv_wave_sum(qe);
            const float lw = -r - kw * (0.5f * qz - 0.5f * qe - 0.5f * slv);
            tot += r;
            mx = fmaxf(mx, lw);
            if (l == 0) wz[row] = lw;
        }
        if (l == 0) {
            double den = 0.0;
            for (int s = 0; s < ns; ++s) {
                const long row = (long)b * ns + s;
                const float e = expf(wz[row] - mx);           // the largest weight gives exactly 1; far smaller ones underflow to 0
                rowscale[row] = e;
                den += (double)e;
            }
            const float sum = (float)den;
            const float r = tot / fns, k = kl[b], g = g_loss[b];
            const float lo = -((mx + logf(sum)) - logf(fns));
            for (int s = 0; s < ns; ++s) {
                const long row = (long)b * ns + s;
                const float lw = wz[row];
                const float wn = rowscale[row] / sum;
                const float rs = g * wn;
                rowscale[row] = rs;
                if constexpr (DREG) {
                    const float r = 1.f - kw * (1.f - wn);
                    rsv[row] = r;
                    wz[row] = (kw * rs) * r;
                } else {
                    wz[row] = kw * rs;
                }
                if (logw) logw[row] = lw;
            }
            rec[b] = r; loss[b] = lo;
            sl += lo; sr += r; sk += k;
        }
    }
    if (l == 0) { red[0][w] = sl; red[1][w] = sr; red[2][w] = sk; }
    __syncthreads();
    if (tid < 3) {
        float t = 0.f;
        for (int i = 0; i < IW_WAVES; ++i) t += red[tid][i];
        acc[tid] += t;
    }
    if (tid == 0 && rng_state) rng_state[1] += rng_inc;
}

// the direct terms of the weights' own gradient, one thread per (b, j)
__global__ __launch_bounds__(256) void reparam_iw_bwd_kernel(const float* __restrict__ mulv, const float* __restrict__ eps,
                                                             const float* __restrict__ wz, float* __restrict__ dmulv, int B, int ns,
                                                             int nz) {
    const long total = (long)B * nz, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int b = (int)(i / nz), j = (int)(i - (long)b * nz);
        const float m = mulv[(long)b * 2 * nz + j], lv = mulv[(long)b * 2 * nz + nz + j];
        const float sdv = expf(0.5f * lv);
        float gz = 0.f, gze = 0.f, sc = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float e = eps[((long)b * ns + s) * nz + j], c = wz[(long)b * ns + s];
            const float t = c * (m + e * sdv);
            gz += t;
            gze += t * e;
            sc += c;
        }
        dmulv[(long)b * 2 * nz + j] = gz;
        dmulv[(long)b * 2 * nz + nz + j] = gze * (0.5f * sdv) - 0.5f * sc;
    }
}

// the complete dmulv from the decoder's dz [B][ns][nz], one thread per (b, j), serial over s: the head backward's per-sample terms
// (lv_head.hip, modes IW and DREG) without the head's two products.  rs == NULL: t = dz + c z and the -1/2 sum_s c_s term;
// rs != NULL: t = r dz + c' (z - eps exp(-logvar/2)).  With wz all zeros (and rs NULL) the operations are reparam_kl_bwd_kernel's
// with dkl all zeros: the same bits.
template <bool DREG>
__global__ __launch_bounds__(256) void reparam_iwdz_bwd_kernel(const float* __restrict__ mulv, const float* __restrict__ eps,
                                                               const float* __restrict__ dz, const float* __restrict__ wz,
                                                               const float* __restrict__ rs, float* __restrict__ dmulv, int B, int ns,
                                                               int nz) {
    const long total = (long)B * nz, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int b = (int)(i / nz), j = (int)(i - (long)b * nz);
        const float m = mulv[(long)b * 2 * nz + j], lv = mulv[(long)b * 2 * nz + nz + j];
        const float sdv = expf(0.5f * lv);
        float gz = 0.f, gze = 0.f, dl;
        if constexpr (DREG) {
            const float isd = expf(-0.5f * lv);
            for (int s = 0; s < ns; ++s) {
                const long zi = ((long)b * ns + s) * nz + j;
                const float e = eps[zi], c = wz[(long)b * ns + s], r = rs[(long)b * ns + s];
                const float g = r * dz[zi] + c * ((m + e * sdv) - e * isd);
                gz += g;
                gze += g * e;
            }
            dl = gze * (0.5f * sdv);
        } else {
            float sc = 0.f;
            for (int s = 0; s < ns; ++s) {
                const long zi = ((long)b * ns + s) * nz + j;
                const float e = eps[zi], c = wz[(long)b * ns + s];
                const float g = dz[zi] + c * (m + e * sdv);
                gz += g;
                gze += g * e;
                sc += c;
            }
            dl = gze * (0.5f * sdv) - 0.5f * sc;
        }
        dmulv[(long)b * 2 * nz + j] = gz;
        dmulv[(long)b * 2 * nz + nz + j] = dl;
    }
}

int assemble_iw(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl, const float* klw,
                const float* g_loss, float* loss, float* rec, float* rowscale, float* wz, float* logw, float* acc, int T, int B, int ns,
                int nz, uint64_t* rng_state, uint64_t rng_inc, void* stream, bool dreg = false, float* rs = nullptr) {
    if (!nll || !mulv || !eps || !z || !kl || !klw || !g_loss || !loss || !rec || !rowscale || !wz || !acc) return LV_ERR_ARG;
    if (dreg && !rs) return LV_ERR_ARG;
    if (T < 0 || B <= 0 || ns <= 0 || nz <= 0) return LV_ERR_SHAPE;
    if (dreg)
        LV_LAUNCH(loss_assemble_iw_kernel<true>, dim3(1), dim3(64 * IW_WAVES), 0, stream, nll, mulv, eps, z, kl, klw, g_loss, loss, rec,
                  rowscale, wz, logw, rs, acc, T, B, ns, nz, reinterpret_cast<unsigned long long*>(rng_state), (unsigned long long)rng_inc);
    else
        LV_LAUNCH(loss_assemble_iw_kernel<false>, dim3(1), dim3(64 * IW_WAVES), 0, stream, nll, mulv, eps, z, kl, klw, g_loss, loss, rec,
                  rowscale, wz, logw, (float*)nullptr, acc, T, B, ns, nz, reinterpret_cast<unsigned long long*>(rng_state),
                  (unsigned long long)rng_inc);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

}  // namespace

// Loss assembly of the importance-weighted objective.  nll [T][B*ns] (T = 1: nll = rec_s, the drop-in route); mulv [B][2nz];
// eps, z [B][ns][nz]; kl, g_loss, loss, rec [B]; rowscale [B*ns]; wz [B][ns]; logw [B][ns] or NULL; acc: device float[3] (+=).
extern "C" int lv_loss_assemble_iw_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                       const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                       float* wz, float* logw, float* acc, int T, int B, int ns, int nz, void* stream) {
    return assemble_iw(nll, mulv, eps, z, kl, kl_weight_dev, g_loss, loss, rec, rowscale, wz, logw, acc, T, B, ns, nz, nullptr, 0, stream);
}

// ... and rng_state[1] += rng_inc, as lv_loss_assemble_ns_rng_f32
extern "C" int lv_loss_assemble_iw_rng_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                           const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                           float* wz, float* logw, float* acc, int T, int B, int ns, int nz, uint64_t* rng_state,
                                           uint64_t rng_inc, void* stream) {
    if (!rng_state) return LV_ERR_ARG;
    return assemble_iw(nll, mulv, eps, z, kl, kl_weight_dev, g_loss, loss, rec, rowscale, wz, logw, acc, T, B, ns, nz, rng_state, rng_inc,
                       stream);
}

// dmulv [B][2nz] ('=') from the weights' direct terms: dmu_j = sum_s c_s z_sj, dlogvar_j = sum_s c_s z_sj 1/2 eps_sj sigma_j - 1/2 sum_s c_s
extern "C" int lv_reparam_iw_bwd_f32(const float* mulv, const float* eps, const float* wz, float* dmulv, int B, int ns, int nz,
                                     void* stream) {
    if (!mulv || !eps || !wz || !dmulv) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0) return LV_ERR_SHAPE;
    const long nb = ((long)B * nz + 255) / 256;
    LV_LAUNCH(reparam_iw_bwd_kernel, dim3((unsigned)(nb > 1024 ? 1024 : nb)), dim3(256), 0, stream, mulv, eps, wz, dmulv, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// Loss assembly of the importance-weighted objective under the doubly-reparameterised estimator: every output of
// lv_loss_assemble_iw_f32 bit for bit, except wz [B][ns] = c'_s = beta g wn_s r_s, plus rs [B][ns] = r_s = 1 - beta (1 - wn_s).
extern "C" int lv_loss_assemble_dreg_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                         const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                         float* wz, float* rs, float* logw, float* acc, int T, int B, int ns, int nz, void* stream) {
    return assemble_iw(nll, mulv, eps, z, kl, kl_weight_dev, g_loss, loss, rec, rowscale, wz, logw, acc, T, B, ns, nz, nullptr, 0, stream,
                       true, rs);
}

// ... and rng_state[1] += rng_inc
extern "C" int lv_loss_assemble_dreg_rng_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                             const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                             float* wz, float* rs, float* logw, float* acc, int T, int B, int ns, int nz,
                                             uint64_t* rng_state, uint64_t rng_inc, void* stream) {
    if (!rng_state) return LV_ERR_ARG;
    return assemble_iw(nll, mulv, eps, z, kl, kl_weight_dev, g_loss, loss, rec, rowscale, wz, logw, acc, T, B, ns, nz, rng_state, rng_inc,
                       stream, true, rs);
}

// The complete dmulv [B][2nz] ('=') of the importance-weighted objective from the decoder's dz [B][ns][nz] (which carries g wn_s
// through rowscale), one launch: what lv_enc_head_iw_bwd_f32 / lv_enc_head_dreg_bwd_f32 compute in front of their two products.
// rs == NULL: the standard estimator, wz = c (lv_loss_assemble_iw_f32); rs != NULL: the doubly-reparameterised one, wz = c', rs = r
// (lv_loss_assemble_dreg_f32).  With rs NULL and wz all zeros the bits of lv_reparam_kl_bwd_f32 with dkl all zeros.
extern "C" int lv_reparam_iwdz_bwd_f32(const float* mulv, const float* eps, const float* dz, const float* wz, const float* rs,
                                       float* dmulv, int B, int ns, int nz, void* stream) {
    if (!mulv || !eps || !dz || !wz || !dmulv) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0) return LV_ERR_SHAPE;
    const long nb = ((long)B * nz + 255) / 256;
    const dim3 grid((unsigned)(nb > 1024 ? 1024 : nb));
    if (rs)
        LV_LAUNCH(reparam_iwdz_bwd_kernel<true>, grid, dim3(256), 0, stream, mulv, eps, dz, wz, rs, dmulv, B, ns, nz);
    else
        LV_LAUNCH(reparam_iwdz_bwd_kernel<false>, grid, dim3(256), 0, stream, mulv, eps, dz, wz, rs, dmulv, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
