// lv_svi.hip -- stochastic variational inference on the encoder's output (VAE.refine_posterior): the decoder is
// frozen, each sentence's phi = (mu | logvar) [2nz] is a free parameter and descends its own
//   L_b(phi) = (1/ns) sum_s rec(x_b, mu + eps_s * sigma) + beta * KL(phi),   sigma = exp(logvar / 2),
// with the noise eps held fixed (common random numbers: L_b is a deterministic function of phi).  One launch does the whole
// variational side of an iteration: record L_b of the CURRENT iterate (trace row, best-iterate tracking), form the gradient of
// lv_reparam_kl_bwd_f32 from the decoder's dz, clip it per sentence, apply heavy-ball momentum, and emit the next iterate's
// samples and analytic KL as lv_reparam_kl_fwd_f32 would.
#include "lv_device.h"

namespace {

// One wave per SENTENCE (as loss_assemble_iw_kernel), lanes stride over nz, butterfly reductions; sentences never interact.
//   L        = (sum_s rec[b*ns + s]) / ns + beta * kl[b]                    -> trace[b]; L < best_loss[b] (strict: a tie keeps the
//                                                                             earlier iterate) copies phi into best_mulv[b]
//   g_mu_j   = sum_s dz_sj + beta * mu_j                                     (dz_sj = sum over the parts, in order; it carries the
//   g_lv_j   = (sum_s dz_sj eps_sj) * sigma_j / 2 + beta * (e^lv_j - 1) / 2   1/ns seed of the decoder backward)
//   g       *= min(1, clip / (|g|_2 + 1e-6))                                 (norm over this sentence's 2nz values)
//   v        = m * v + g;   phi -= lr * v
//   z_next   = mu + eps * sigma,  kl_next = KL(phi)                          (reparam_kl_fwd_kernel's expressions and summation
//                                                                             order: the same bits)
// dz == nullptr: finish mode, nothing behind the best-tracking runs.
constexpr int SVI_WAVES = 4;
__global__ __launch_bounds__(64 * SVI_WAVES) void svi_step_kernel(const float* __restrict__ rec, const float* __restrict__ dz, int parts,
                                                                  const float* __restrict__ eps, const float* __restrict__ kl,
                                                                  const float* __restrict__ klw, float lr, float mom, float clip,
                                                                  float* mulv, float* __restrict__ vel, float* __restrict__ best_mulv,
                                                                  float* __restrict__ best_loss, float* __restrict__ trace,
                                                                  float* __restrict__ z_next, float* __restrict__ kl_next, int B, int ns,
                                                                  int nz) {
    const int tid = (int)threadIdx.x, l = tid & 63;
    const int b = (int)blockIdx.x * SVI_WAVES + (tid >> 6);
    if (b >= B) return;                                   // whole waves leave: no workgroup barrier below
    const float kw = klw[0];
    float* phi = mulv + (long)b * 2 * nz;
    float r = 0.f;
    for (int s = 0; s < ns; ++s) r += rec[(long)b * ns + s];
    const float L = r / (float)ns + kw * kl[b];
    // lane 0 reads the running minimum for the wave and is the one that replaces it: the broadcast orders its store behind every
    // lane's copy of the comparison
    const bool better = L < __shfl(l == 0 ? best_loss[b] : 0.f, 0, 64);
    if (l == 0) trace[b] = L;
    if (better) {
        for (int j = l; j < 2 * nz; j += 64) best_mulv[(long)b * 2 * nz + j] = phi[j];
        if (l == 0) best_loss[b] = L;
    }
    if (!dz) return;
    const long pstride = (long)B * ns * nz;
    // the gradient of coordinate j (both halves); evaluated twice -- once for the norm, once for the update -- from the same
    // loads in the same order, so no per-lane array is needed for nz > 64
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

}  // namespace

// One refinement iteration's variational side (see the kernel).  rec [B*ns] (decoder row order b*ns + s); dz [dz_parts][B*ns][nz]
// (lv_dec_tail_dz_f32's partial sums, or one plain gradient) or NULL for finish mode; eps [B][ns][nz]; kl [B] of the current
// iterate; kl_weight_dev: device float (beta); in/out mulv, vel, best_mulv [B][2nz], best_loss [B]; out trace_row [B],
// z_next [B][ns][nz], kl_next [B].  Finish mode reads neither eps, vel, z_next nor kl_next (they may be NULL).
extern "C" int lv_svi_step_f32(const float* rec, const float* dz, int dz_parts, const float* eps, const float* kl,
                               const float* kl_weight_dev, float lr, float momentum, float clip, float* mulv, float* vel,
                               float* best_mulv, float* best_loss, float* trace_row, float* z_next, float* kl_next, int B, int ns,
                               int nz, void* stream) {
    if (!rec || !kl || !kl_weight_dev || !mulv || !best_mulv || !best_loss || !trace_row) return LV_ERR_ARG;
    if (dz && (!eps || !vel || !z_next || !kl_next)) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0 || (dz && dz_parts <= 0)) return LV_ERR_SHAPE;
    if (dz && (!(lr > 0.f) || !(clip > 0.f) || !(momentum >= 0.f && momentum < 1.f))) return LV_ERR_ARG;
    LV_LAUNCH(svi_step_kernel, dim3((unsigned)lv_cdiv(B, SVI_WAVES)), dim3(64 * SVI_WAVES), 0, stream, rec, dz, dz_parts, eps, kl,
              kl_weight_dev, lr, momentum, clip, mulv, vel, best_mulv, best_loss, trace_row, z_next, kl_next, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
