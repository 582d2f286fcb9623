// lv_hmc.hip -- Hamiltonian Monte Carlo transitions for annealed importance sampling (VAE.nll_ais(transition="hmc"); Neal 2001,
// Wu et al. 2017, Cremer et al. 2018) and for posterior sampling (VAE.sample_from_posterior(transition="hmc")).  The decoder
// engine evaluates rec(z) = -log p(x|z) and d(z) = d rec / d z (backward_dz with drec = 1 per row) on all rows at once; this file
// is the sampler's side of such a pass: lv_svi_step_f32's counterpart for chains.
//
// THE CONTRACT.  Chain r = b * C + c of sentence b (decoder row order, the multi-sample decoder's b * ns + s with ns = C).  q0, g,
// mh_accept, the float64 beta values and the float64 logw are those of lv_ais.hip:
//   q0        = N(mu0, diag exp(lv0)), mu0 / lv0 [B][nz]; both NULL: the prior N(0, I)
//   g(z)      = (log p(z) - log q0(z)) + (-rec(z))      float32; with the prior as q0 the pair is skipped: g = -rec, bit for bit
//   target    log f_beta(z) = log q0(z) + (float)beta * g(z),   U_beta = -log f_beta
//   gradient  grad U_beta(z)_j = a_j + (float)beta * ((z_j - a_j) + d_j),   a_j = (z_j - mu0_j) * expf(-lv0_j)
//             (prior as q0: grad U_beta(z)_j = z_j + (float)beta * d_j)
//   z_0 ~ q0,  logw = 0 (float64),  eps_r = step_size
//   for i = 1..N (temperature beta_i, L leapfrog steps, momentum p <- mom_i[r] ~ N(0, I) and u_i[r] from buffers):
//       logw += (beta_i - beta_{i-1}) * (double) g(cur)
//       K0 = 0.5 sum_j p_j^2
//       p <- p - (eps / 2) * grad U_{beta_i}(cur)                  from the CACHED d(cur): no decoder pass
//       for l = 1..L:   z <- z + eps * p                           (z starts at cur)
//                       rec(z), d(z)                               one decoder forward + backward_dz on all B * C rows
//                       p <- p - (l < L ? eps : eps / 2) * grad U_{beta_i}(z)
//       dH = [log q0(z) + (float)beta_i g(z)] - [log q0(cur) + (float)beta_i g(cur)] + K0 - 0.5 sum_j p_j^2
//       accept = mh_accept(dH, u_i)                                select, never blend; a NaN dH or one at -inf rejects
//       accepted: (cur, g, lq, rec, d) <- those of z;  accepts += 1
//       eps_r <- min(max(eps_r * (accepted ? up : down), eps_min), eps_max)       (up = down = 1, bounds (0, inf): eps is fixed)
//   log p^(x) = logsumexp_c logw_c - log C                         (the float64 torch epilogue of nll_ais)
// A transition costs exactly L decoder passes: the gradient at its start is that of the state just selected, kept in d_cur and
// recombined for the new beta here.  Noise is never generated in a kernel.
//
// FLOAT32 EVALUATION ORDER (the build contracts no multiply-add; every operation below rounds on its own).  j is a coordinate.
//   d_j       = ((0 + dz[0][r][j]) + dz[1][r][j]) + ...            the tail's partial rows, in order
//   a_j       = (z_j - mu0_j) * expf(-lv0_j)
//   grad_j    = a_j + bf * ((z_j - a_j) + d_j)      prior: z_j + bf * d_j                   bf = (float)beta
//   kick      p_j <- p_j - (h * grad_j),  h = eps (full) or 0.5f * eps (half)
//   drift     z_j <- (eps * p_j) + z_j
//   sum over nz of a term t_j (wave_sum): lane l adds t_l, t_{l+64}, ... in order from 0, then the 64 lane sums are combined
//             by the butterfly v += shfl_xor(v, m), m = 32, 16, 8, 4, 2, 1
//   K         = 0.5f * wave_sum(p_j * p_j)
//   log q0(z) = -0.5f * wave_sum(((z_j - mu0_j) * (z_j - mu0_j)) * expf(-lv0_j)) - 0.5f * ((float)nz * log(2 pi) + wave_sum(lv0_j))
//               prior: -0.5f * wave_sum(z_j * z_j) - 0.5f * ((float)nz * log(2 pi) + 0)
//   g(z)      = (log prior(z) - log q0(z)) + (-rec)                prior as q0: -rec
//   dH        = ((lq_z + bf * g_z) - (lq_cur + bf * g_cur)) + (K0 - K1)
//   eps_r     = fminf(fmaxf(eps_r * f, eps_min), eps_max)
//   logw     += dbeta_next * (double) g                            float64
#include "lv_cond_ll.h"

namespace {

constexpr int HMC_WAVES = 4;
constexpr int HMC_INIT = 0, HMC_MID = 1, HMC_LAST = 2;

__device__ __forceinline__ float hmc_grad_u(float z, float d, float bf, bool prior, float mu, float iv) {
    if (prior) return z + bf * d;
    const float a = (z - mu) * iv;
    return a + bf * ((z - a) + d);
}

// One wave per chain row (as svi_step_kernel has one per sentence), lanes stride over nz, rows never interact.
//   init: the pass scored z_0 = pos.  cur <- pos, the state of z_0, logw = 0, accepts = 0; then OPEN the first transition.
//   mid:  full kick, drift, write pos / mom.
//   last: half kick, dH, decision, select, count, adapt; then OPEN the next transition.
//   OPEN (mom_next given): logw += dbeta_next * g(cur); p <- mom_next[r]; K0; half kick at beta_next from d_cur; drift; write
//   pos, mom, k0.  mom_next NULL: the chain ends, only the state is written.
__global__ __launch_bounds__(64 * HMC_WAVES) void hmc_leap_kernel(
    const float* __restrict__ rec, const float* __restrict__ dz, int parts, float* __restrict__ pos, float* __restrict__ mom,
    float* __restrict__ k0, float* __restrict__ cur, float* __restrict__ g_cur, float* __restrict__ lq_cur,
    float* __restrict__ rec_cur, float* __restrict__ d_cur, double* __restrict__ logw, int* __restrict__ accepts,
    float* __restrict__ eps, const float* __restrict__ u, const float* __restrict__ mom_next, double beta, double beta_next,
    double dbeta_next, const float* __restrict__ mu0, const float* __restrict__ lv0, int rows, int C, int nz, int mode, float up,
    float down, float eps_min, float eps_max, float* __restrict__ dh_out, int* __restrict__ flag_out,
    double* __restrict__ logw_out_next, float* __restrict__ keep_out) {
    const int tid = (int)threadIdx.x, l = tid & 63;
    const long r = (long)blockIdx.x * HMC_WAVES + (tid >> 6);
    if (r >= rows) return;                                // whole waves leave: no workgroup barrier below
    const bool prior = mu0 == nullptr;
    const float* mu = prior ? nullptr : mu0 + (r / C) * nz;
    const float* lv = prior ? nullptr : lv0 + (r / C) * nz;
    const long pstride = (long)rows * nz;
    float* z = pos + r * nz;
    float* p = mom + r * nz;
    float* cz = cur + r * nz;
    float* dc = d_cur + r * nz;
    auto dsum = [&](int j) {
        float d = 0.f;
        for (int q = 0; q < parts; ++q) d += dz[q * pstride + r * nz + j];
        return d;
    };
    float e = eps[r];
    if (mode == HMC_MID) {
        const float bf = (float)beta;
        for (int j = l; j < nz; j += 64) {
            const float gr = hmc_grad_u(z[j], dsum(j), bf, prior, prior ? 0.f : mu[j], prior ? 1.f : expf(-lv[j]));
            const float pj = p[j] - e * gr;
            p[j] = pj;
            z[j] = mh_propose(pj, e, z[j]);
        }
        return;
    }
    // the state of the point the pass scored: log q0(z), g(z), and (last) the kinetic energy after the closing half kick
    const float bf = (float)beta;
    float q = 0.f, zz = 0.f, lvs = 0.f, kk = 0.f;
    for (int j = l; j < nz; j += 64) {
        const float zj = z[j];
        if (!prior) {
            const float dv = zj - mu[j];
            q += (dv * dv) * expf(-lv[j]);
            lvs += lv[j];
        }
        zz += zj * zj;
        if (mode == HMC_LAST) {
            const float gr = hmc_grad_u(zj, dsum(j), bf, prior, prior ? 0.f : mu[j], prior ? 1.f : expf(-lv[j]));
            const float pj = p[j] - (0.5f * e) * gr;
            kk += pj * pj;
        }
    }
    const float lprior = -0.5f * lv_wave_sum(zz) - 0.5f * ((float)nz * GP_LOG_2PI + 0.f);
    const float rz = rec[r];
    float lq_z, g_z;
    if (prior) {
        lq_z = lprior;
        g_z = -rz;
    } else {
        lq_z = -0.5f * lv_wave_sum(q) - 0.5f * ((float)nz * GP_LOG_2PI + lv_wave_sum(lvs));
        g_z = (lprior - lq_z) + (-rz);
    }
    bool take;                                            // the scored point becomes the chain's state
    float g, lq;
    double lw;
    int cnt;
    if (mode == HMC_INIT) {
        take = true;
        g = g_z;
        lq = lq_z;
        lw = 0.0;
        cnt = 0;
    } else {
        const float K1 = 0.5f * lv_wave_sum(kk);
        const float gc = g_cur[r], lc = lq_cur[r];
        const float dH = ((lq_z + bf * g_z) - (lc + bf * gc)) + (k0[r] - K1);
        // lane 0 decides for the wave: every lane holds the same dH, the broadcast makes the branch below uniform by construction
        take = __shfl(mh_accept(dH, u[r]) ? 1 : 0, 0, 64) != 0;
        g = take ? g_z : gc;
        lq = take ? lq_z : lc;
        lw = logw[r];
        cnt = accepts[r] + (take ? 1 : 0);
        e = fminf(fmaxf(e * (take ? up : down), eps_min), eps_max);
        if (l == 0) {
            if (dh_out) dh_out[r] = dH;
            if (flag_out) flag_out[r] = take ? 1 : 0;
        }
    }
    if (mom_next) lw += dbeta_next * (double)g;
    if (l == 0) {
        if (take) { g_cur[r] = g; lq_cur[r] = lq; rec_cur[r] = rz; }
        accepts[r] = cnt;
        eps[r] = e;
        if (mode == HMC_INIT || mom_next) logw[r] = lw;
        if (mom_next && logw_out_next) logw_out_next[r] = lw;
    }
    // select, then open the next transition from the selected state; lane l owns coordinates l, l + 64, ...
    const float bn = (float)beta_next;
    float k = 0.f;
    for (int j = l; j < nz; j += 64) {
        float cj, dj;
        if (take) {
            cj = z[j];
            dj = dsum(j);
            cz[j] = cj;
            dc[j] = dj;
        } else {
            cj = cz[j];
            dj = dc[j];
        }
        if (keep_out) keep_out[r * nz + j] = cj;
        if (mom_next) {
            const float pn = mom_next[r * nz + j];
            k += pn * pn;
            const float gr = hmc_grad_u(cj, dj, bn, prior, prior ? 0.f : mu[j], prior ? 1.f : expf(-lv[j]));
            const float pj = pn - (0.5f * e) * gr;
            p[j] = pj;
            z[j] = mh_propose(pj, e, cj);
        }
    }
    if (mom_next) {
        const float K0 = 0.5f * lv_wave_sum(k);
        if (l == 0) k0[r] = K0;
    }
}

}  // namespace

// The sampler's side of one decoder pass for rows = B * C chains; the contract is at the top of this file.
//   rec [rows], dz [parts][rows][nz] (lv_dec_tail_dz_f32's partial sums; parts = 1: a plain gradient): the pass at pos
//   in flight: pos [rows][nz] (the decoder's z input), mom [rows][nz], k0 [rows]
//   state: cur [rows][nz], g_cur / lq_cur / rec_cur [rows], d_cur [rows][nz], logw [rows] float64, accepts [rows] int32, eps [rows]
//   u [rows] (mode last), mom_next [rows][nz] or NULL (no transition follows); mu0 / lv0 [B][nz] or both NULL
//   beta: this transition's temperature (mid, last); beta_next and dbeta_next = beta_next - beta: the transition mom_next opens
//   (all three float64, formed by the caller); L: the transition's leapfrog steps (a mid kick needs L >= 2)
//   mode 0 init, 1 mid, 2 last; up / down / eps_min / eps_max: the step-size adaptation of mode last
//   dh_out, flag_out [rows] (mode last), logw_out_next [rows] (with mom_next), keep_out [rows][nz] (the selected cur; init, last):
//   or NULL
extern "C" int lv_hmc_leap_f32(const float* rec, const float* dz, int parts, float* pos, float* mom, float* k0, float* cur,
                               float* g_cur, float* lq_cur, float* rec_cur, float* d_cur, double* logw, int* accepts, float* eps,
                               const float* u, const float* mom_next, double beta, double beta_next, double dbeta_next,
                               const float* mu0, const float* lv0, int rows, int C, int nz, int L, int mode, float up, float down,
                               float eps_min, float eps_max, float* dh_out, int* flag_out, double* logw_out_next, float* keep_out,
                               void* stream) {
    if (!rec || !dz || !pos || !mom || !k0 || !cur || !g_cur || !lq_cur || !rec_cur || !d_cur || !logw || !accepts || !eps ||
        (mu0 == nullptr) != (lv0 == nullptr))
        return LV_ERR_ARG;
    if (mode != HMC_INIT && mode != HMC_MID && mode != HMC_LAST) return LV_ERR_ARG;
    if (mode == HMC_LAST && !u) return LV_ERR_ARG;
    if (mode == HMC_LAST && (!(up > 0.f) || !(down > 0.f) || !(eps_min >= 0.f) || !(eps_max >= eps_min))) return LV_ERR_ARG;
    if (rows <= 0 || C <= 0 || rows % C != 0 || nz < 1 || L < 1 || parts < 1 || (mode == HMC_MID && L < 2)) return LV_ERR_SHAPE;
    if (((uintptr_t)logw & 7) != 0 || ((uintptr_t)logw_out_next & 7) != 0) return LV_ERR_ALIGN;
    LV_LAUNCH(hmc_leap_kernel, dim3((unsigned)lv_cdiv(rows, HMC_WAVES)), dim3(64 * HMC_WAVES), 0, stream, rec, dz, parts, pos, mom,
              k0, cur, g_cur, lq_cur, rec_cur, d_cur, logw, accepts, eps, u, mom_next, beta, beta_next, dbeta_next, mu0, lv0, rows, C,
              nz, mode, up, down, eps_min, eps_max, dh_out, flag_out, logw_out_next, keep_out);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
