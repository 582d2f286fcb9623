// lv_savae.hip -- the per-sentence arithmetic of semi-amortized training (SA-VAE, Kim et al. 2018; VAE.loss_savae):
// the ELBO is taken at the posterior lv_svi.hip's refinement reaches after K steps, and the step differentiates THROUGH the
// refinement.  With lambda = (mu | logvar) [2nz] per sentence, L_b as in lv_svi.hip and the refinement
//   g_k = grad L_b(lambda_k);  gh_k = g_k * min(1, clip / (|g_k|_2 + 1e-6));  v_{k+1} = m v_k + gh_k;  lambda_{k+1} = lambda_k - lr v_{k+1}
// the backward pass walks k = K-1 .. 0 with the adjoints lb (of lambda) and vb (of v):
//   vb -= lr * lb;   gb = J_clip(g_k)^T vb;   vb *= m;   lb += H_k gb   (and the decoder's gradient += d/dtheta of g_k . gb)
// where the Hessian-vector products are central differences of gradients at lambda_k +- e u, u = gb / |gb| over the WHOLE batch:
// one decoder pass on B * 2ns rows (samples 0..ns-1 at lambda_k + e u seeded +c/ns, samples ns..2ns-1 at lambda_k - e u seeded
// -c/ns, c = |gb| / (2e)) leaves c * (grad_theta F+ - grad_theta F-) in the weight gradients and the dz that lv_savae_hvp_f32 turns
// into c * (grad_lambda F+ - grad_lambda F-).  Three entries: the recording form of lv_svi_step_f32 (forward), the adjoint step and
// the Hessian-vector assembly (backward).  Nothing goes to the host.
#include "lv_device.h"

namespace {

// lv_svi.hip's svi_step_kernel without the loss record and the best-iterate tracking, and with two stores more: the unclipped
// gradient g_k and the iterate lambda_k it was taken at, into this step's [B][2nz] records.  The update, the samples and the KL are
// svi_step_kernel's expressions in its order (the library is built without contraction): phi, vel, z_next, kl_next carry the same bits.
constexpr int REC_WAVES = 4;
__global__ __launch_bounds__(64 * REC_WAVES) void svi_rec_step_kernel(const float* __restrict__ dz, int parts, const float* __restrict__ eps,
                                                                      const float* __restrict__ klw, float lr, float mom, float clip,
                                                                      float* mulv, float* __restrict__ vel, float* __restrict__ g_rec,
                                                                      float* __restrict__ phi_rec, float* __restrict__ z_next,
                                                                      float* __restrict__ kl_next, int B, int ns, int nz) {
    const int tid = (int)threadIdx.x, l = tid & 63;
    const int b = (int)blockIdx.x * REC_WAVES + (tid >> 6);
    if (b >= B) return;                                   // whole waves leave: no workgroup barrier below
    const float kw = klw[0];
    float* phi = mulv + (long)b * 2 * nz;
    const long pstride = (long)B * ns * nz;
    auto grad = [&](int j, float& gm, float& gl) {
        const float m = phi[j], lv = phi[nz + j];
        const float sd = expf(0.5f * lv);
        float gz = 0.f, gze = 0.f;
        for (int s = 0; s < ns; ++s) {
            const long zi = ((long)b * ns + s) * nz + j;
            float g = 0.f;
            for (int p = 0; p < parts; ++p) g += dz[p * pstride + zi];
            gz += g;
            gze += g * eps[zi];
        }
        gm = gz + kw * m;
        gl = gze * (0.5f * sd) + kw * (0.5f * (expf(lv) - 1.f));
    };
    float sq = 0.f;
    for (int j = l; j < nz; j += 64) {
        float gm, gl;
        grad(j, gm, gl);
        sq += gm * gm;
        sq += gl * gl;
    }
    const float norm = sqrtf(lv_wave_sum(sq));
    const float coef = fminf(1.f, clip / (norm + 1e-6f));
    for (int j = l; j < nz; j += 64) {
        float gm, gl;
        grad(j, gm, gl);                                  // reads phi[j], phi[nz + j]: written below by this lane only
        float* gr = g_rec + (long)b * 2 * nz;
        float* pr = phi_rec + (long)b * 2 * nz;
        gr[j] = gm; gr[nz + j] = gl;
        pr[j] = phi[j]; pr[nz + j] = phi[nz + j];
        float* vb = vel + (long)b * 2 * nz;
        const float vm = mom * vb[j] + gm * coef, vl = mom * vb[nz + j] + gl * coef;
        vb[j] = vm; vb[nz + j] = vl;
        phi[j] = phi[j] - lr * vm;
        phi[nz + j] = phi[nz + j] - lr * vl;
    }
    // next iterate's samples and KL: lane l re-reads what IT stored (j = l mod 64, and l < 32 covers nz <= 32)
    const int G = nz <= 32 ? 32 : 64;
    float part = 0.f;
    if (l < G) {
        for (int j = l; j < nz; j += G) {
            const float m = phi[j], lv = phi[nz + j];
            const float sd = expf(0.5f * lv);
            part += (m * m + expf(lv)) - lv - 1.f;
            for (int s = 0; s < ns; ++s) {
                const long zi = ((long)b * ns + s) * nz + j;
                z_next[zi] = m + eps[zi] * sd;
            }
        }
    }
    if (G == 64) part += __shfl_xor(part, 32, 64);
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if (l == 0) kl_next[b] = 0.5f * part;
}

// One workgroup for the whole batch (B * 2nz is a few thousand values at most and the direction's norm couples every sentence).
//   phase 1, one wave per sentence (lanes over nz, butterfly reductions):
//     vb = vbar - lr * lbar;   r = |g|_2 (svi_step_kernel's summation order: the same clip decision), s = clip / (r + 1e-6)
//     gb = vb                                                   where s >= 1 (clip inactive)
//     gb = s * vb - clip * (g . vb) / (r * (r + 1e-6)^2) * g    otherwise
//     vbar = m * vb;   u = gb (not yet normalised);   the wave's sum of gb^2 in double and its max |lambda|
//   phase 2: n = sqrt(sum gb^2) over all B * 2nz entries (double), e = fd_eps * max(1, max |lambda|), c = n / (2e)  -> scal[0..2]
//   phase 3: u = gb / n (n = 0: u = 0, c = 0);  z+- = (mu +- e u_mu) + eps_s * exp((logvar +- e u_lv) / 2) in decoder row order
//            b * 2ns + s (plus) and b * 2ns + ns + s (minus);  seeds[row] = +-c / ns.
constexpr int ADJ_WAVES = 4;
__global__ __launch_bounds__(64 * ADJ_WAVES) void savae_adjoint_kernel(const float* __restrict__ lbar, float* __restrict__ vbar,
                                                                       const float* __restrict__ g, const float* __restrict__ lam,
                                                                       const float* __restrict__ eps, float lr, float mom, float clip,
                                                                       float fd_eps, float* u, float* __restrict__ scal,
                                                                       float* __restrict__ zpm, float* __restrict__ seeds, int B, int ns,
                                                                       int nz) {
    __shared__ double red_sq[ADJ_WAVES];
    __shared__ float red_mx[ADJ_WAVES];
    const int tid = (int)threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int n2 = 2 * nz;
    double sq_all = 0.0;
    float mx = 0.f;
    for (int b = wv; b < B; b += ADJ_WAVES) {
        const long o = (long)b * n2;
        float sq = 0.f, dot = 0.f;
        for (int j = l; j < nz; j += 64) {
            const float gm = g[o + j], gl = g[o + nz + j];
            sq += gm * gm;
            sq += gl * gl;
            const float vm = vbar[o + j] - lr * lbar[o + j], vl = vbar[o + nz + j] - lr * lbar[o + nz + j];
            dot += gm * vm;
            dot += gl * vl;
        }
        const float r = sqrtf(lv_wave_sum(sq));
        dot = lv_wave_sum(dot);
        const float s = clip / (r + 1e-6f);
        const bool active = !(s >= 1.f);
        const float back = active ? clip * dot / (r * ((r + 1e-6f) * (r + 1e-6f))) : 0.f;
        for (int j = l; j < n2; j += 64) {
            const float vb = vbar[o + j] - lr * lbar[o + j];
            const float gb = active ? s * vb - back * g[o + j] : vb;
            vbar[o + j] = mom * vb;
            u[o + j] = gb;
            sq_all += (double)gb * (double)gb;
            mx = fmaxf(mx, fabsf(lam[o + j]));
        }
    }
    sq_all = lv_wave_sum(sq_all);
    mx = lv_wave_max(mx);
    if (l == 0) { red_sq[wv] = sq_all; red_mx[wv] = mx; }
    __syncthreads();                                      // also orders phase 1's stores to u before phase 3's loads
    const double tot = (red_sq[0] + red_sq[1]) + (red_sq[2] + red_sq[3]);
    const float n = (float)sqrt(tot);
    const float e = fd_eps * fmaxf(1.f, fmaxf(fmaxf(red_mx[0], red_mx[1]), fmaxf(red_mx[2], red_mx[3])));
    const float c = n / (2.f * e);                        // n = 0: c = 0, every seed 0
    if (tid == 0) { scal[0] = n; scal[1] = e; scal[2] = c; }
    const int rows = 2 * ns;
    for (int i = tid; i < B * nz; i += 64 * ADJ_WAVES) {
        const int b = i / nz, j = i - b * nz;
        const long o = (long)b * n2;
        const float um = n > 0.f ? u[o + j] / n : 0.f, ul = n > 0.f ? u[o + nz + j] / n : 0.f;
        u[o + j] = um; u[o + nz + j] = ul;
        const float m = lam[o + j], lv = lam[o + nz + j];
        const float mp = m + e * um, mm = m - e * um;
        const float sdp = expf(0.5f * (lv + e * ul)), sdm = expf(0.5f * (lv - e * ul));
        for (int s = 0; s < ns; ++s) {
            const float ep = eps[((long)b * ns + s) * nz + j];
            zpm[((long)b * rows + s) * nz + j] = mp + ep * sdp;
            zpm[((long)b * rows + ns + s) * nz + j] = mm + ep * sdm;
        }
    }
    const float cs = c / (float)ns;
    for (int i = tid; i < B * rows; i += 64 * ADJ_WAVES) seeds[i] = (i % rows) < ns ? cs : -cs;
}

// One thread per (sentence, coordinate), as reparam_kl_bwd_kernel.  dz [parts][B*2ns][nz] of the pass savae_adjoint_kernel laid out
// (its rows carry the seeds +-c/ns), summed over the parts in order:
//   lbar_mu += sum_s (dz+_s + dz-_s)                                   + c beta (mu+ - mu-)
//   lbar_lv += sum_s eps_s (dz+_s sigma+ / 2 + dz-_s sigma- / 2)       + c beta (e^lv+ - e^lv-) / 2
// with mu+-, lv+- = lambda_k +- e u and sigma+- = exp(lv+- / 2): the reparameterisation chain rule and the analytic KL's gradient
// at the perturbed points.  scal[0] = n = 0: nothing is written.
__global__ __launch_bounds__(256) void savae_hvp_kernel(const float* __restrict__ dz, int parts, const float* __restrict__ eps,
                                                        const float* __restrict__ lam, const float* __restrict__ u,
                                                        const float* __restrict__ scal, const float* __restrict__ klw,
                                                        float* __restrict__ lbar, int B, int ns, int nz) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * nz) return;
    if (!(scal[0] > 0.f)) return;
    const float e = scal[1], c = scal[2], kw = klw[0];
    const int b = (int)(idx / nz), j = (int)(idx % nz);
    const long o = (long)b * 2 * nz;
    const float m = lam[o + j], lv = lam[o + nz + j], um = u[o + j], ul = u[o + nz + j];
    const float mp = m + e * um, mm = m - e * um, lp = lv + e * ul, lm = lv - e * ul;
    const float sdp = expf(0.5f * lp), sdm = expf(0.5f * lm);
    const int rows = 2 * ns;
    const long pstride = (long)B * rows * nz;
    float gzp = 0.f, gzep = 0.f, gzm = 0.f, gzem = 0.f;
    for (int s = 0; s < ns; ++s) {
        const long zp = ((long)b * rows + s) * nz + j, zm = ((long)b * rows + ns + s) * nz + j;
        const float ep = eps[((long)b * ns + s) * nz + j];
        float gp = 0.f, gm = 0.f;
        for (int p = 0; p < parts; ++p) {
            gp += dz[p * pstride + zp];
            gm += dz[p * pstride + zm];
        }
        gzp += gp;
        gzep += gp * ep;
        gzm += gm;
        gzem += gm * ep;
    }
    const float ck = c * kw;
    lbar[o + j] = lbar[o + j] + ((gzp + gzm) + ck * (mp - mm));
    lbar[o + nz + j] = lbar[o + nz + j] + ((gzep * (0.5f * sdp) + gzem * (0.5f * sdm)) + ck * (0.5f * (expf(lp) - expf(lm))));
}

}  // namespace

// The recording form of lv_svi_step_f32's update (see the kernel): dz [dz_parts][B*ns][nz], eps [B][ns][nz], kl_weight_dev: device
// float (beta); in/out mulv, vel [B][2nz]; out g_rec, phi_rec [B][2nz] (this step's rows of the [K][B][2nz] records: the unclipped
// gradient and the iterate BEFORE the update), z_next [B][ns][nz], kl_next [B].
extern "C" int lv_svi_rec_step_f32(const float* dz, int dz_parts, const float* eps, const float* kl_weight_dev, float lr, float momentum,
                                   float clip, float* mulv, float* vel, float* g_rec, float* phi_rec, float* z_next, float* kl_next,
                                   int B, int ns, int nz, void* stream) {
    if (!dz || !eps || !kl_weight_dev || !mulv || !vel || !g_rec || !phi_rec || !z_next || !kl_next) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0 || dz_parts <= 0) return LV_ERR_SHAPE;
    if (!(lr > 0.f) || !(clip > 0.f) || !(momentum >= 0.f && momentum < 1.f)) return LV_ERR_ARG;
    LV_LAUNCH(svi_rec_step_kernel, dim3((unsigned)lv_cdiv(B, REC_WAVES)), dim3(64 * REC_WAVES), 0, stream, dz, dz_parts, eps, kl_weight_dev,
              lr, momentum, clip, mulv, vel, g_rec, phi_rec, z_next, kl_next, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// One backward iteration's adjoint step (see the kernel).  lbar [B][2nz] (read), vbar [B][2nz] (in/out), g, lam [B][2nz] (step k's
// records), eps [B][ns][nz]; out u [B][2nz], scal [3] = (n, e, c), z_pm [B][2ns][nz], seeds [B*2ns].
extern "C" int lv_savae_adjoint_f32(const float* lbar, float* vbar, const float* g, const float* lam, const float* eps, float lr,
                                    float momentum, float clip, float fd_eps, float* u, float* scal, float* z_pm, float* seeds, int B,
                                    int ns, int nz, void* stream) {
    if (!lbar || !vbar || !g || !lam || !eps || !u || !scal || !z_pm || !seeds) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0) return LV_ERR_SHAPE;
    if (!(lr > 0.f) || !(clip > 0.f) || !(momentum >= 0.f && momentum < 1.f) || !(fd_eps > 0.f)) return LV_ERR_ARG;
    LV_LAUNCH(savae_adjoint_kernel, dim3(1), dim3(64 * ADJ_WAVES), 0, stream, lbar, vbar, g, lam, eps, lr, momentum, clip, fd_eps, u,
              scal, z_pm, seeds, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lbar += c * (grad_lambda F(lam + e u) - grad_lambda F(lam - e u)) from the perturbed pass's dz (see the kernel).
// dz [dz_parts][B*2ns][nz], eps [B][ns][nz], lam, u [B][2nz], scal [3] and kl_weight_dev on the device; lbar [B][2nz] in/out.
extern "C" int lv_savae_hvp_f32(const float* dz, int dz_parts, const float* eps, const float* lam, const float* u, const float* scal,
                                const float* kl_weight_dev, float* lbar, int B, int ns, int nz, void* stream) {
    if (!dz || !eps || !lam || !u || !scal || !kl_weight_dev || !lbar) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0 || dz_parts <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(savae_hvp_kernel, dim3((unsigned)lv_cdiv((long)B * nz, 256)), dim3(256), 0, stream, dz, dz_parts, eps, lam, u, scal,
              kl_weight_dev, lbar, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
