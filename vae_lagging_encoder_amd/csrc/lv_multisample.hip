// lv_multisample.hip -- the kernels of multi-sample training (VAE.loss(x, kl_weight, nsamples = ns), modules/vae.py:79-98).
//
// The reference expands every sentence ns times before the decoder LSTM (dec_lstm.py:83-99: word embeddings, after dropout_in,
// `.expand(batch, ns, ...)`, viewed as batch * ns rows, row b * ns + s) and averages the reconstruction term over the samples
// (dec_lstm.py:146-148, vae.py:95-98).  The word half of the decoder's input projection is therefore the same for the ns
// rows of a sentence: it is computed on B rows and expanded here (lv_gx_expand_add_f32); its backward sums the gate gradients
// of a sentence's rows first (lv_sample_sum_*), so that dX, dW_ih[:, :ni] and the embedding scatter run on B rows as well.
// Decoder row order everywhere: bd = b * ns + s.
#include "lv_device.h"

namespace {

constexpr int MS_MAX_BLOCKS = 2048;      // streaming kernels: grid capped, grid-stride loop over the rest
// The streaming kernels are templated on the type of the flat work-item index: 32-bit where the item count allows (every shape of
// the text models; the index is split into (row, column) by a division per item), 64-bit otherwise.  Addresses are always 64-bit.
#define MS_LAUNCH_INDEXED(kern, items, ...)                                                                   \
    do {                                                                                                      \
        if ((items) < (1L << 30)) LV_LAUNCH(kern<int>, dim3(ms_grid(items)), dim3(256), 0, stream, __VA_ARGS__);  \
        else LV_LAUNCH(kern<long>, dim3(ms_grid(items)), dim3(256), 0, stream, __VA_ARGS__);                      \
    } while (0)

// gx[t][b*ns + s][c] = gxw[t][b][c] + zp[b*ns + s][c]; one float4 of gxw is loaded once and stored ns times from registers.
// Work item = (t, b, c4): consecutive threads walk c, so every load and store of a wave is 1 KB contiguous.
template <class I>
__global__ __launch_bounds__(256) void gx_expand_add_v4_kernel(const float* __restrict__ gxw, const float* __restrict__ zp,
                                                                float* __restrict__ gx, long rows, int B, int ns, int C4) {
    const I total = (I)(rows * C4);                   // rows = Td * B
    const I stride = (I)gridDim.x * 256;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C4;                           // t * B + b
        const int c = (int)(i - r * C4) * 4;
        const int b = (int)(r % B);
        const long C = (long)C4 * 4;
        const float4 w = *reinterpret_cast<const float4*>(gxw + r * C + c);
        const float* zrow = zp + (long)b * ns * C + c;
        float* orow = gx + (long)r * ns * C + c;
        for (int s = 0; s < ns; ++s) {
            const float4 z = *reinterpret_cast<const float4*>(zrow + (long)s * C);
            *reinterpret_cast<float4*>(orow + (long)s * C) = make_float4(w.x + z.x, w.y + z.y, w.z + z.z, w.w + z.w);
        }
    }
}

// the same for a C that is not a multiple of 4 (or unaligned pointers): one float per work item
template <class I>
__global__ __launch_bounds__(256) void gx_expand_add_kernel(const float* __restrict__ gxw, const float* __restrict__ zp,
                                                             float* __restrict__ gx, long rows, int B, int ns, int C) {
    const I total = (I)(rows * C);
    const I stride = (I)gridDim.x * 256;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C;
        const int c = (int)(i - r * C);
        const int b = (int)(r % B);
        const float w = gxw[i];
        for (int s = 0; s < ns; ++s) gx[((long)r * ns + s) * C + c] = w + zp[((long)b * ns + s) * C + c];
    }
}

// dgs[r][c] = sum_{s = 0 .. ns-1} dg[r*ns + s][c], added left to right in f32
template <class I>
__global__ __launch_bounds__(256) void sample_sum_v4_kernel(const float* __restrict__ dg, float* __restrict__ dgs, long rows, int ns,
                                                             int C4) {
    const I total = (I)(rows * C4);
    const I stride = (I)gridDim.x * 256;
    const long C = (long)C4 * 4;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C4;
        const int c = (int)(i - r * C4) * 4;
        const float* in = dg + (long)r * ns * C + c;
        float4 a = *reinterpret_cast<const float4*>(in);
        for (int s = 1; s < ns; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(in + (long)s * C);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        *reinterpret_cast<float4*>(dgs + r * C + c) = a;
    }
}

template <class I>
__global__ __launch_bounds__(256) void sample_sum_kernel(const float* __restrict__ dg, float* __restrict__ dgs, long rows, int ns, int C) {
    const I total = (I)(rows * C);
    const I stride = (I)gridDim.x * 256;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C;
        const int c = (int)(i - r * C);
        float a = dg[(long)r * ns * C + c];
        for (int s = 1; s < ns; ++s) a += dg[((long)r * ns + s) * C + c];
        dgs[i] = a;
    }
}

// 16-bit-image twin: bf16 in, f32 sum left to right, ONE rounding (nearest even) to bf16 out.  8 values (16 bytes) per work item.
template <class I>
__global__ __launch_bounds__(256) void sample_sum_b16_v8_kernel(const uint16_t* __restrict__ dg, long ld_in, uint16_t* __restrict__ dgs,
                                                                 long ld_out, long rows, int ns, int C8) {
    const I total = (I)(rows * C8);
    const I stride = (I)gridDim.x * 256;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C8;
        const int c = (int)(i - r * C8) * 8;
        const uint16_t* in = dg + (long)r * ns * ld_in + c;
        float a[8];
        {
            const uint4 q = *reinterpret_cast<const uint4*>(in);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int h = 0; h < 4; ++h) { a[2 * h] = lv_bf16_bits_to_f32(w[h] & 0xFFFFu); a[2 * h + 1] = lv_bf16_bits_to_f32(w[h] >> 16); }
        }
        for (int s = 1; s < ns; ++s) {
            const uint4 q = *reinterpret_cast<const uint4*>(in + (long)s * ld_in);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int h = 0; h < 4; ++h) { a[2 * h] += lv_bf16_bits_to_f32(w[h] & 0xFFFFu); a[2 * h + 1] += lv_bf16_bits_to_f32(w[h] >> 16); }
        }
        *reinterpret_cast<uint4*>(dgs + r * ld_out + c) = make_uint4(lv_pack_bf16x2(a[0], a[1]), lv_pack_bf16x2(a[2], a[3]),
                                                                      lv_pack_bf16x2(a[4], a[5]), lv_pack_bf16x2(a[6], a[7]));
    }
}

template <class I>
__global__ __launch_bounds__(256) void sample_sum_b16_kernel(const uint16_t* __restrict__ dg, long ld_in, uint16_t* __restrict__ dgs,
                                                              long ld_out, long rows, int ns, int C) {
    const I total = (I)(rows * C);
    const I stride = (I)gridDim.x * 256;
    for (I i = (I)blockIdx.x * 256 + (I)threadIdx.x; i < total; i += stride) {
        const I r = i / C;
        const int c = (int)(i - r * C);
        float a = lv_bf16_bits_to_f32(dg[(long)r * ns * ld_in + c]);
        for (int s = 1; s < ns; ++s) a += lv_bf16_bits_to_f32(dg[((long)r * ns + s) * ld_in + c]);
        dgs[r * ld_out + c] = (uint16_t)lv_f32_to_bf16_bits(a);
    }
}

// x_rep[b*ns + s][t] = x[b][t]
__global__ __launch_bounds__(256) void repeat_rows_i64_kernel(const int64_t* __restrict__ x, int64_t* __restrict__ x_rep, long n_in, int T,
                                                              int ns) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_in; i += stride) {
        const long b = i / T;
        const int t = (int)(i - b * T);
        const int64_t v = x[i];
        for (int s = 0; s < ns; ++s) x_rep[(b * ns + s) * T + t] = v;
    }
}

// loss_assemble_kernel (lv_loss.hip) with samples: one wave per SENTENCE; for s = 0 .. ns-1 the wave sums nll[.][b*ns + s] over t
// exactly as the ns = 1 kernel does (lanes stride over t, fixed-shape butterfly), lane 0 adds the ns sums in order.
constexpr int LAN_WAVES = 16;
__global__ __launch_bounds__(64 * LAN_WAVES) void loss_assemble_ns_kernel(const float* __restrict__ nll, const float* __restrict__ kl,
                                                                          const float* __restrict__ klw, const float* __restrict__ g_loss,
                                                                          float* __restrict__ loss, float* __restrict__ rec,
                                                                          float* __restrict__ rowscale, float* __restrict__ dkl,
                                                                          float* __restrict__ acc, int T, int B, int ns,
                                                                          unsigned long long* rng_state, unsigned long long rng_inc) {
    __shared__ float red[3][LAN_WAVES];
    const int tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    const float kw = klw[0];
    const long Bd = (long)B * ns;
    const float fns = (float)ns;
    float sl = 0.f, sr = 0.f, sk = 0.f;
    for (int b = w; b < B; b += LAN_WAVES) {
        float tot = 0.f;
        for (int s = 0; s < ns; ++s) {
            float a = 0.f;
            for (int t = l; t < T; t += 64) a += nll[(long)t * Bd + (long)b * ns + s];
            tot += lv_wave_sum(a);
        }
        if (l == 0) {
            const float r = tot / fns;
            const float k = kl[b], lo = r + kw * k, g = g_loss[b];
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
        for (int i = 0; i < LAN_WAVES; ++i) t += red[tid][i];
        acc[tid] += t;
    }
    if (tid == 0 && rng_state) rng_state[1] += rng_inc;
}

inline bool ms_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

inline unsigned ms_grid(long items) {
    const long nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : (nb > MS_MAX_BLOCKS ? MS_MAX_BLOCKS : nb));
}

}  // namespace

// Word half of the decoder's input projection, expanded over the samples (dec_lstm.py:83-99).  gxw [Td][B][C], zp [B*ns][C],
// gx [Td][B*ns][C], all dense.
extern "C" int lv_gx_expand_add_f32(const float* gxw, const float* zp, float* gx, int Td, int B, int ns, int C, void* stream) {
    if (!gxw || !zp || !gx) return LV_ERR_ARG;
    if (Td < 0 || B <= 0 || ns <= 0 || C <= 0) return LV_ERR_SHAPE;
    if (Td == 0) return LV_OK;
    const long rows = (long)Td * B;
    if (C % 4 == 0 && ms_aligned16(gxw) && ms_aligned16(zp) && ms_aligned16(gx))
        MS_LAUNCH_INDEXED(gx_expand_add_v4_kernel, rows * (C / 4), gxw, zp, gx, rows, B, ns, C / 4);
    else
        MS_LAUNCH_INDEXED(gx_expand_add_kernel, rows * C, gxw, zp, gx, rows, B, ns, C);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// dgs[t][b][:] = sum_s dg[t][b*ns + s][:]  (s = 0 .. ns-1 in order); dg [Td][B*ns][C], dgs [Td][B][C], dense.
extern "C" int lv_sample_sum_f32(const float* dg, float* dgs, int Td, int B, int ns, int C, void* stream) {
    if (!dg || !dgs) return LV_ERR_ARG;
    if (Td < 0 || B <= 0 || ns <= 0 || C <= 0) return LV_ERR_SHAPE;
    if (Td == 0) return LV_OK;
    const long rows = (long)Td * B;
    if (C % 4 == 0 && ms_aligned16(dg) && ms_aligned16(dgs))
        MS_LAUNCH_INDEXED(sample_sum_v4_kernel, rows * (C / 4), dg, dgs, rows, ns, C / 4);
    else
        MS_LAUNCH_INDEXED(sample_sum_kernel, rows * C, dg, dgs, rows, ns, C);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// The same on bf16 images (rows of ld_in / ld_out elements): f32 sum, one rounding to nearest even.
extern "C" int lv_sample_sum_b16(const uint16_t* dg, long ld_in, uint16_t* dgs, long ld_out, int Td, int B, int ns, int C, void* stream) {
    if (!dg || !dgs) return LV_ERR_ARG;
    if (Td < 0 || B <= 0 || ns <= 0 || C <= 0 || ld_in < C || ld_out < C) return LV_ERR_SHAPE;
    if (Td == 0) return LV_OK;
    const long rows = (long)Td * B;
    if (C % 8 == 0 && ld_in % 8 == 0 && ld_out % 8 == 0 && ms_aligned16(dg) && ms_aligned16(dgs))
        MS_LAUNCH_INDEXED(sample_sum_b16_v8_kernel, rows * (C / 8), dg, ld_in, dgs, ld_out, rows, ns, C / 8);
    else
        MS_LAUNCH_INDEXED(sample_sum_b16_kernel, rows * C, dg, ld_in, dgs, ld_out, rows, ns, C);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// x_rep[b*ns + s][:] = x[b][:]  (x int64 [B][T] dense): the token ids in decoder row order
extern "C" int lv_repeat_rows_i64(const int64_t* x, int64_t* x_rep, int B, int T, int ns, void* stream) {
    if (!x || !x_rep) return LV_ERR_ARG;
    if (B <= 0 || T <= 0 || ns <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(repeat_rows_i64_kernel, dim3(ms_grid((long)B * T)), dim3(256), 0, stream, x, x_rep, (long)B * T, T, ns);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// lv_loss_assemble_f32 with samples.  nll [T][B*ns]; kl, g_loss, loss, rec, dkl [B]; rowscale [B*ns]; acc: device float[3] (+=).
extern "C" int lv_loss_assemble_ns_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                                       float* loss, float* rec, float* rowscale, float* dkl, float* acc, int T, int B, int ns,
                                       void* stream) {
    if (!nll || !kl || !kl_weight_dev || !g_loss || !loss || !rec || !rowscale || !dkl || !acc) return LV_ERR_ARG;
    if (T < 0 || B <= 0 || ns <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(loss_assemble_ns_kernel, dim3(1), dim3(64 * LAN_WAVES), 0, stream, nll, kl, kl_weight_dev, g_loss, loss, rec, rowscale,
              dkl, acc, T, B, ns, (unsigned long long*)nullptr, 0ULL);
    LV_CHECK_LAUNCH();
    return LV_OK;
}

// ... and rng_state[1] += rng_inc, as lv_loss_assemble_rng_f32
extern "C" int lv_loss_assemble_ns_rng_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                                           float* loss, float* rec, float* rowscale, float* dkl, float* acc, int T, int B, int ns,
                                           uint64_t* rng_state, uint64_t rng_inc, void* stream) {
    if (!nll || !kl || !kl_weight_dev || !g_loss || !loss || !rec || !rowscale || !dkl || !acc || !rng_state) return LV_ERR_ARG;
    if (T < 0 || B <= 0 || ns <= 0) return LV_ERR_SHAPE;
    LV_LAUNCH(loss_assemble_ns_kernel, dim3(1), dim3(64 * LAN_WAVES), 0, stream, nll, kl, kl_weight_dev, g_loss, loss, rec, rowscale,
              dkl, acc, T, B, ns, reinterpret_cast<unsigned long long*>(rng_state), (unsigned long long)rng_inc);
    LV_CHECK_LAUNCH();
    return LV_OK;
}
