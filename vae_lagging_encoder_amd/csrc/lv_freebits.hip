// lv_freebits.hip -- the free-bits (KL thresholding) objective: Kingma et al. 2016, Chen et al. 2017, Li et al. 2019.
//
// THE CONTRACT.  Per sentence b and latent dimension j, KL_bj = 0.5 (mu_bj^2 + exp(lv_bj) - lv_bj - 1).  lambda = free_bits >= 0, in
// nats PER LATENT DIMENSION in every mode.  The gate g is a constant of the step: no gradient flows through it.  All comparisons are
// strict (>).
//
//   mode            statistic compared                                     gate                    thresholded KL of sentence b
//   0 "dim"         KL_bj                                                  g_bj = KL_bj > lambda   sum_j (g_bj ? KL_bj : lambda)
//   1 "batch_dim"   m_j = (sum_b KL_bj) / B, summed in ascending b         g_bj = g_j = m_j > lam  sum_j (g_j ? KL_bj : lambda)
//   2 "batch"       m = (sum_b kl_b) / B, ascending b, kl_b = sum_j KL_bj  g_bj = g = m > tau      g ? kl_b : tau
//                   tau = (float)(nz * lambda), formed on the host in double
//
//   loss_b = rec_b + w * kl_obj_b  (for "batch_dim": mean_b loss_b = mean_b rec_b + w sum_j max(lambda, m_j), the textbook objective)
//   d kl_obj_b / d mu_bj = g_bj mu_bj,   d kl_obj_b / d lv_bj = g_bj 0.5 (exp(lv_bj) - 1);  the path through z is unchanged.
//   The REPORTED KL (VAE.loss's third value, kl_sum of the trainers) stays the analytic, unthresholded one; loss_sum reports the
//   objective that was minimised.  No evaluation function applies free bits.
//
// Everything here is exact f32 (-ffp-contract=off) with a fixed order of addition: with every gate open kl_obj is the kl of
// lv_reparam_kl_fwd_f32 (lv_loss.hip) bit for bit -- the same per-term expression, the same lanes-then-butterfly order.
#include "lv_device.h"

namespace {

constexpr int FB_THREADS = 1024;     // one workgroup: the batch statistics need no hand-off between workgroups
constexpr int FB_STAGE = 4096;       // floats of LDS the batch sums are staged through (B is not bounded by it: rows go in chunks)

// Rows of mulv dealt to groups of G lanes (G = 32 when nz <= 32, else 64: lv_reparam_kl_fwd_f32's split), lane j0 adding its terms
// j0, j0 + G, ... in order, then the butterfly.  t_bj = 2 KL_bj is what is added (the 0.5 is applied to the sum, as the ungated
// kernel does); a closed dimension adds 2 lambda.  GATE_SRC: 0 decide here from KL_bj (and write the gate), 1 read the gate that
// the column pass wrote, 2 no gate (plain kl_b, mode 2's first pass).
template <int G, int GATE_SRC>
__device__ __forceinline__ void fb_row_pass(const float* __restrict__ mulv, float lam, float* kl_obj, float* gate, float* stat,
                                            int B, int nz, int tid) {
    const int j0 = tid % G, grp = tid / G;
    const float lam2 = 2.f * lam;
    for (int row0 = 0; row0 < B; row0 += FB_THREADS / G) {          // (every lane of a group takes the same trips: the shuffles are uniform)
        const int row = row0 + grp;
        const bool ok = row < B;
        const float* mu = mulv + (long)(ok ? row : 0) * 2 * nz;
        const float* lv = mu + nz;
        float part = 0.f;
        for (int j = j0; j < nz; j += G) {
            if (!ok) break;
            const float m = mu[j], l = lv[j];
            const float t = (m * m + expf(l)) - l - 1.f;
            bool g = true;
            if (GATE_SRC == 0) {
                const float k = 0.5f * t;
                g = k > lam;
                gate[(long)row * nz + j] = g ? 1.f : 0.f;
                if (stat) stat[(long)row * nz + j] = k;
            } else if (GATE_SRC == 1) {
                g = gate[(long)row * nz + j] != 0.f;
            }
            part += g ? t : lam2;
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
        if (ok && j0 == 0) kl_obj[row] = 0.5f * part;
    }
}

template <int G>
__global__ __launch_bounds__(FB_THREADS) void kl_freebits_fwd_kernel(const float* __restrict__ mulv, float lam, float tau, int mode,
                                                                     float* kl_obj, float* gate, float* stat, int B, int nz) {
    __shared__ float sbuf[FB_STAGE];
    __shared__ float sg[FB_THREADS];
    const int tid = (int)threadIdx.x;
    if (mode == 0) {
        fb_row_pass<G, 0>(mulv, lam, kl_obj, gate, stat, B, nz, tid);
        return;
    }
    if (mode == 1) {
        // column pass: tiles of up to FB_THREADS dimensions, a thread per dimension; the KL_bj of a chunk of rows are formed by all
        // threads into LDS, then each dimension's thread adds its column in ascending b
        for (int c0 = 0; c0 < nz; c0 += FB_THREADS) {
            const int tw = nz - c0 < FB_THREADS ? nz - c0 : FB_THREADS;
            const int cb = FB_STAGE / tw;                           // rows per chunk (>= 4)
            float run = 0.f;
            for (int b0 = 0; b0 < B; b0 += cb) {
                const int nb = B - b0 < cb ? B - b0 : cb;
                for (int i = tid; i < nb * tw; i += FB_THREADS) {
                    const int bb = i / tw, jj = i % tw;
                    const float* mu = mulv + (long)(b0 + bb) * 2 * nz;
                    const float m = mu[c0 + jj], l = mu[nz + c0 + jj];
                    sbuf[i] = 0.5f * ((m * m + expf(l)) - l - 1.f);
                }
                __syncthreads();
                if (tid < tw)
                    for (int bb = 0; bb < nb; ++bb) run += sbuf[bb * tw + tid];
                __syncthreads();
            }
            if (tid < tw) {
                const float mj = run / (float)B;
                sg[tid] = mj > lam ? 1.f : 0.f;
                if (stat) stat[c0 + tid] = mj;
            }
            __syncthreads();
            for (long i = tid; i < (long)B * tw; i += FB_THREADS) gate[(i / tw) * nz + c0 + (int)(i % tw)] = sg[i % tw];
            __syncthreads();
        }
        // (the gate is read back by other threads of this workgroup than wrote it: behind the barrier above)
        fb_row_pass<G, 1>(mulv, lam, kl_obj, gate, stat, B, nz, tid);
        return;
    }
    // mode 2: kl_b of every row first, their sum in ascending b by one thread out of LDS, then the one decision for the batch
    fb_row_pass<G, 2>(mulv, lam, kl_obj, gate, stat, B, nz, tid);
    __syncthreads();
    float run = 0.f;
    for (int b0 = 0; b0 < B; b0 += FB_STAGE) {
        const int nb = B - b0 < FB_STAGE ? B - b0 : FB_STAGE;
        for (int i = tid; i < nb; i += FB_THREADS) sbuf[i] = kl_obj[b0 + i];
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < nb; ++i) run += sbuf[i];
        __syncthreads();
    }
    if (tid == 0) {
        const float m = run / (float)B;
        sg[0] = m > tau ? 1.f : 0.f;
        if (stat) stat[0] = m;
    }
    __syncthreads();
    const float g = sg[0];
    if (g == 0.f)
        for (int b = tid; b < B; b += FB_THREADS) kl_obj[b] = tau;
    for (long i = tid; i < (long)B * nz; i += FB_THREADS) gate[i] = g;
}

// lv_reparam_kl_bwd_f32's kernel with dkl_b * gate_bj in place of dkl_b
__global__ __launch_bounds__(256) void reparam_kl_gated_bwd_kernel(const float* __restrict__ mulv, const float* __restrict__ eps,
                                                                   const float* __restrict__ dz, const float* __restrict__ dkl,
                                                                   const float* __restrict__ gate, float* __restrict__ dmulv,
                                                                   int B, int ns, int nz) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * nz) return;
    const int b = (int)(idx / nz), j = (int)(idx % nz);
    const float m = mulv[(long)b * 2 * nz + j], l = mulv[(long)b * 2 * nz + nz + j];
    const float sd = expf(0.5f * l);
    float gz = 0.f, gze = 0.f;
    for (int s = 0; s < ns; ++s) {
        const long zi = ((long)b * ns + s) * nz + j;
        const float g = dz[zi];
        gz += g;
        gze += g * eps[zi];
    }
    const float gk = dkl[b] * gate[(long)b * nz + j];
    dmulv[(long)b * 2 * nz + j] = gz + gk * m;
    dmulv[(long)b * 2 * nz + nz + j] = gze * (0.5f * sd) + gk * (0.5f * (expf(l) - 1.f));
}

// loss_assemble_ns_kernel (lv_multisample.hip) with the thresholded KL in the loss and the analytic one in the report sum
constexpr int FB_LAN_WAVES = 16;
__global__ __launch_bounds__(64 * FB_LAN_WAVES) void loss_assemble_fb_kernel(const float* __restrict__ nll, const float* __restrict__ kl,
                                                                             const float* __restrict__ kl_obj,
                                                                             const float* __restrict__ klw, const float* __restrict__ g_loss,
                                                                             float* __restrict__ loss, float* __restrict__ rec,
                                                                             float* __restrict__ rowscale, float* __restrict__ dkl,
                                                                             float* __restrict__ acc, int T, int B, int ns,
                                                                             unsigned long long* rng_state, unsigned long long rng_inc) {
    __shared__ float red[3][FB_LAN_WAVES];
    const int tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    const float kw = klw[0];
    const long Bd = (long)B * ns;
    const float fns = (float)ns;
    float sl = 0.f, sr = 0.f, sk = 0.f;
    for (int b = w; b < B; b += FB_LAN_WAVES) {
        float tot = 0.f;
        for (int s = 0; s < ns; ++s) {
            float a = 0.f;
            for (int t = l; t < T; t += 64) a += nll[(long)t * Bd + (long)b * ns + s];
            tot += lv_wave_sum(a);
        }
        if (l == 0) {
            const float r = tot / fns;
            const float k = kl[b], lo = r + kw * kl_obj[b], g = g_loss[b];
            rec[b] = r; loss[b] = lo;
            dkl[b] = kw * g;
            const float rs = g / fns;
            for (int s = 0; s < ns; ++s) rowscale[(long)b * ns + s] = rs;
            sl += lo; sr += r; sk += k;
        }
    }
    if (l == 0) { red[0][w] = sl; red[1][w] = sr; red[2][w] = sk; }
    __syncthreads();
    if (tid < 3) {
        float t = 0.f;
        for (int i = 0; i < FB_LAN_WAVES; ++i) t += red[tid][i];
        acc[tid] += t;
    }
    if (tid == 0 && rng_state) rng_state[1] += rng_inc;
}

}  // namespace

// mulv [B][2nz] -> kl_obj [B] (the thresholded KL), gate [B][nz] (0.0f / 1.0f), stat (may be null): the statistic that was
// compared -- [B][nz] in mode 0, [nz] in mode 1, [1] in mode 2.  One launch of one workgroup; any B >= 1 and nz >= 1.  This raw
// entry takes any lam (a negative one opens every gate); the public layers refuse lam < 0.
extern "C" int lv_kl_freebits_fwd_f32(const float* mulv, float lam, int mode, float* kl_obj, float* gate, float* stat, int B, int nz,
                                      void* stream) {
    if (!mulv || !kl_obj || !gate) return LV_ERR_ARG;
    if (mode < 0 || mode > 2) return LV_ERR_ARG;
    if (B <= 0 || nz <= 0) return LV_ERR_SHAPE;
    const float tau = (float)((double)nz * (double)lam);
    if (nz <= 32)
        LV_LAUNCH((kl_freebits_fwd_kernel<32>), dim3(1), dim3(FB_THREADS), 0, stream, mulv, lam, tau, mode, kl_obj, gate, stat, B, nz);
    else
        LV_LAUNCH((kl_freebits_fwd_kernel<64>), dim3(1), dim3(FB_THREADS), 0, stream, mulv, lam, tau, mode, kl_obj, gate, stat, B, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_reparam_kl_bwd_f32 with the gate [B][nz] on the KL seed; a gate of all ones gives its bits
extern "C" int lv_reparam_kl_gated_bwd_f32(const float* mulv, const float* eps, const float* dz, const float* dkl, const float* gate,
                                           float* dmulv, int B, int ns, int nz, void* stream) {
    if (!mulv || !eps || !dz || !dkl || !gate || !dmulv) return LV_ERR_ARG;
    if (B <= 0 || ns <= 0 || nz <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(reparam_kl_gated_bwd_kernel, dim3((unsigned)lv_cdiv((long)B * nz, 256)), dim3(256), 0, stream, mulv, eps, dz, dkl, gate,
              dmulv, B, ns, nz);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_loss_assemble_ns_f32 with loss_b = rec_b + w kl_obj_b; acc[2] += sum_b kl_b stays the analytic KL.  kl_obj = kl gives
// lv_loss_assemble_ns_f32's bits.
extern "C" int lv_loss_assemble_fb_f32(const float* nll, const float* kl, const float* kl_obj, const float* kl_weight_dev,
                                       const float* g_loss, float* loss, float* rec, float* rowscale, float* dkl, float* acc, int T,
                                       int B, int ns, void* stream) {
    if (!nll || !kl || !kl_obj || !kl_weight_dev || !g_loss || !loss || !rec || !rowscale || !dkl || !acc) return LV_ERR_ARG;
    if (T < 0 || B <= 0 || ns <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(loss_assemble_fb_kernel, dim3(1), dim3(64 * FB_LAN_WAVES), 0, stream, nll, kl, kl_obj, kl_weight_dev, g_loss, loss, rec,
              rowscale, dkl, acc, T, B, ns, (unsigned long long*)nullptr, 0ULL);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// ... and rng_state[1] += rng_inc, as lv_loss_assemble_ns_rng_f32
extern "C" int lv_loss_assemble_fb_rng_f32(const float* nll, const float* kl, const float* kl_obj, const float* kl_weight_dev,
                                           const float* g_loss, float* loss, float* rec, float* rowscale, float* dkl, float* acc, int T,
                                           int B, int ns, uint64_t* rng_state, uint64_t rng_inc, void* stream) {
    if (!nll || !kl || !kl_obj || !kl_weight_dev || !g_loss || !loss || !rec || !rowscale || !dkl || !acc || !rng_state)
        return LV_ERR_ARG;
    if (T < 0 || B <= 0 || ns <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(loss_assemble_fb_kernel, dim3(1), dim3(64 * FB_LAN_WAVES), 0, stream, nll, kl, kl_obj, kl_weight_dev, g_loss, loss, rec,
              rowscale, dkl, acc, T, B, ns, reinterpret_cast<unsigned long long*>(rng_state), (unsigned long long)rng_inc);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
