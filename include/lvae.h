/* lvae.h -- C ABI of liblvae_hip.so: the MI355X (gfx950) kernels behind the aggressive-VAE training hot path.
 *
 * The reference (jxhe/vae-lagging-encoder) has no FFI layer: its hot path calls PyTorch/ATen ops from Python
 * (SURVEY.md 2.2, 8b).  Each entry point below replaces one implicit ATen op (or a fused group of them) at the
 * reference call site cited next to it.  Conventions for every function:
 *   - plain device pointers + sizes + a hipStream_t passed as void*; no torch types, no C++ types, no exceptions;
 *   - return int: 0 = ok, > 0 = hipError_t of the launch, < 0 = argument check (-1 arg, -2 shape, -3 alignment,
 *     -4 unsupported);
 *   - the caller owns every buffer including workspaces; functions never allocate, free or synchronise, and are
 *     stream-ordered on `stream` (graph-capture safe); re-entrant, no global mutable state;
 *   - scalars that change between hipGraph replays (kl weight, lr, clip coefficient, Adam step) are read from
 *     device memory (`*_dev` arguments).
 * Layouts: token ids int64 batch-first [B][ids_stride] (as data/text_data.py:219-255 builds them); activations
 * time-major, row r = t*B + b; dropout keep-masks uint8 batch-first [B][T][C] (the reference's tensor layout).
 */
#ifndef LVAE_H
#define LVAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense contractions (exact f32 on v_mfma_f32_32x32x2_f32) ------------------------------------------------
 * C[M,N](ldc) = alpha * op(A)[M,K] . op(B)[K,N] (+ add1[(row % mod1)*ld1 + col]) (+ add2[...]) (+ C if accumulate)
 * transA = 0: A stored [M][K];  1: stored [K][M].   transB = 0: B stored [K][N];  1: stored [N][K].
 * Replaces aten::mm/addmm under nn.LSTM's input projection (modules/encoders/enc_lstm.py:60,
 * modules/decoders/dec_lstm.py:104), nn.Linear (enc_lstm.py:62; dec_lstm.py:99,109) and their backward
 * (text.py:384).  The add1/add2 epilogue carries the two LSTM biases and the decoder's z-projection, so
 * torch.cat((word_embed, z_), -1) (dec_lstm.py:97) is never materialised. */
int lv_gemm_f32(int transA, int transB, int M, int N, int K, float alpha,
                const float* A, long lda, const float* B, long ldb, float* C, long ldc, int accumulate,
                const float* add1, long ld1, int mod1, const float* add2, long ld2, int mod2,
                float* ws /* optional split-K scratch */, long ws_floats, void* stream);

/* Same contract on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16): f32 operands in HBM are rounded to bf16 while
 * being staged, accumulation and outputs are f32.  The throughput configuration of BASELINE.json (bf16). */
int lv_gemm_bf16(int transA, int transB, int M, int N, int K, float alpha,
                 const float* A, long lda, const float* B, long ldb, float* C, long ldc, int accumulate,
                 const float* add1, long ld1, int mod1, const float* add2, long ld2, int mod2,
                 float* ws, long ws_floats, void* stream);

/* bf16 matrix pipe over operands that are already bf16 in HBM (raw bits, uint16_t): the vocabulary-sized
 * contractions of LSTMDecoder (pred_linear forward dec_lstm.py:117 and its two backward products).  B is stored
 * [N][K]; A is stored [M][K] (transA = 0) or [K][M] (transA = 1); lda % 8 == 0, ldb % 8 == 0, both 16 B-aligned
 * (else LV_ERR_ALIGN).  Same epilogue / split-K contract as lv_gemm_f32.  Operands
 * rounded with lv_cvt_bf16_f32 / lv_softmax_nll_bwd_b16 give results bit-identical to lv_gemm_bf16 on the f32 data. */
int lv_gemm_b16(int transA, int M, int N, int K, float alpha,
                const uint16_t* A, long lda, const uint16_t* B, long ldb, float* C, long ldc, int accumulate,
                const float* add1, long ld1, int mod1, const float* add2, long ld2, int mod2,
                float* ws, long ws_floats, void* stream);
/* LSTMDecoder's vocabulary projection fused with the statistics of nn.CrossEntropyLoss (modules/decoders/dec_lstm.py:117,
 * 140-146): logits = A . B^T (operands as lv_gemm_b16, transA = 0) written once as IEEE binary16 [M][ldl16] (RNE of the f32
 * accumulators; the f32 logits image is never produced) + per-row statistics over 64-column pieces, part [M][parts] (max,
 * sum exp(x - max)) with parts = lv_gemm_b16_nll_parts(N), + tgt_logit [M] = the logit of row r's target token
 * ids[(r % Bsz) * ids_stride + r / Bsz + tgt_off].  lv_softmax_nll_merge_f32 finishes lse / nll; lv_softmax_nll_bwd_h16 is the
 * backward over the binary16 image.  ldl16 % 8 == 0. */
/* ONE product, TWO destinations: C1 [M][nsplit] = columns [0, nsplit) of op(A) . B^T, C2 [M][N - nsplit] the rest (lv_gemm_b16 otherwise:
 * bf16 operand images, f32 accumulation; no addends).  The two weight gradients of an LSTM layer that share their A operand --
 * dW_ih = dG^T X and dW_hh = dG^T h_prev, the backward of nn.LSTM at enc_lstm.py:55 / dec_lstm.py:104 -- as one launch over the image
 * [X^T ; h_prev^T] ([ni + H][T*B]) and one reduction stage.  lv_gemm_b16_dual_supported: 1 where the shape takes the split-K route
 * the column split rides in (not the 256 x 256 tile), else 0 and the entry returns LV_ERR_UNSUPPORTED. */
int lv_gemm_b16_dual_supported(int M, int N, int K, long ws_floats);
int lv_gemm_b16_dual(int transA, int M, int N, int K, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                     float* C1, long ldc1, int nsplit, float* C2, long ldc2, float* ws, long ws_floats, void* stream);
/* TWO independent products in ONE launch of one workgroup per CU: C0 (| C0b) = op(A0) . B0^T and C1 = A1 . B1^T (operands, layouts and
 * alignment as lv_gemm_b16; plain outputs; nsplit0 > 0: columns >= nsplit0 of the first product go to C0b as in lv_gemm_b16_dual; the
 * second product is in the transA = 0 form; M1 == 0: one product).  The backward of one nn.LSTM layer's input side (enc_lstm.py:55 /
 * dec_lstm.py:104 under autograd): [dW_ih | dW_hh] = dG^T [X ; h_prev] and dX = dG . W_ih, which as single launches leave 256 x 256 tiles
 * for 96 and 50 of the 256 CUs.  Both products run on the 256 x 256 quadrant K loop; a tile whose K range is shared between workgroups
 * is summed INSIDE the launch, in descending K order whoever does it (deterministic): by the workgroup that closes the tile's K range if
 * it finds the others arrived (a bounded look; its own piece then never leaves its registers), else by whichever draws the last ticket
 * (no reduction launch, no wait that progress depends on).
 * lv_gemm_b16_pair_supported: 1 where that is possible AND worth it (both products present, >= 12 K tiles per workgroup), else 0; the
 * entry itself only refuses the impossible (LV_ERR_UNSUPPORTED: second product transposed, > 1024 tiles, ws_floats < 2 * 256 * 65536). */
int lv_gemm_b16_pair_supported(int transA0, int M0, int N0, int K0, int transA1, int M1, int N1, int K1, long ws_floats);
int lv_gemm_b16_pair_pending(int* pending, void* stream);   /* diagnostic: *pending (device int) = arrival counters not back at zero; 0 between launches */
int lv_gemm_b16_pair(int transA0, int M0, int N0, int K0, const uint16_t* A0, long lda0, const uint16_t* B0, long ldb0,
                     float* C0, long ldc0, int nsplit0, float* C0b, long ldc0b,
                     int transA1, int M1, int N1, int K1, const uint16_t* A1, long lda1, const uint16_t* B1, long ldb1,
                     float* C1, long ldc1, float* ws, long ws_floats, void* stream);
/* C [M][N] = (A . B^T) * (keep ? kscale : 0): lv_gemm_b16 (transA = 0, plain output, ldc = N) with the backward of nn.Dropout on the
 * LSTM output (dec_lstm.py:106; dO = dlogits . W_pred then masked) applied in the product's reduction stage instead of by a pass of
 * its own; rows time-major (r = t * Bsz + b), keep = the reference-layout mask [Bsz][M / Bsz][N], uint8. */
int lv_gemm_b16_keep(int M, int N, int K, const uint16_t* A, long lda, const uint16_t* B, long ldb, float* C,
                     const uint8_t* keep, float kscale, int Bsz, float* ws, long ws_floats, void* stream);
/* C = op(A) . B^T as lv_gemm_b16 computes it (alpha 1, no addends) and, in the same pass, the product's sum of squares:
 * sq[0 .. parts) receives one partial per wave of the kernels that hold C's final values (fixed slots: deterministic), parts =
 * lv_gemm_b16_sumsq_parts(M, N, K, ws_floats); 0 parts = the shape does not take the 256 x 256 tile and lv_gemm_b16_sumsq refuses it
 * (LV_ERR_ARG).  sq_only != 0: C is NOT written -- a weight gradient that only enters the norm of clip_grad_norm_ (text.py:383-387:
 * the inner loop clips over all parameters and steps the encoder alone; dW_pred is such a gradient). */
int lv_gemm_b16_sumsq_parts(int M, int N, int K, long ws_floats);
int lv_gemm_b16_sumsq(int transA, int M, int N, int K, const uint16_t* A, long lda, const uint16_t* B, long ldb, float* C, long ldc,
                      float* ws, long ws_floats, float* sq, int sq_only, void* stream);
int lv_gemm_b16_nll_parts(int N);
/* The same two entries with the tile edge named by the caller instead of chosen by shape: tile = 0 (by shape: the 256 x 256 x 64
 * kernel, one workgroup per CU, for products of >= 1e11 flop -- the three vocabulary-sized GEMMs of dec_lstm.py:117,140-146 --
 * else 128 x 128 x 64), 128 or 256 (tests, microbenchmarks; anything else LV_ERR_ARG).  A per-call argument: the library keeps no
 * process-wide state. */
int lv_gemm_b16_tile(int tile, int transA, int M, int N, int K, float alpha,
                     const uint16_t* A, long lda, const uint16_t* B, long ldb, float* C, long ldc, int accumulate,
                     const float* add1, long ld1, int mod1, const float* add2, long ld2, int mod2,
                     float* ws, long ws_floats, void* stream);
int lv_gemm_b16_nll_tile(int tile, int M, int N, int K, const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* logits16,
                         long ldl16, const int64_t* ids, long ids_stride, int tgt_off, int Bsz, float* part, float* tgt_logit,
                         void* stream);
int lv_gemm_b16_nll(int M, int N, int K, const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* logits16, long ldl16,
                    const int64_t* ids, long ids_stride, int tgt_off, int Bsz, float* part, float* tgt_logit, void* stream);
int lv_softmax_nll_merge_f32(const float* part, int nparts, const float* tgt_logit, float* lse, float* nll, int R, void* stream);
int lv_softmax_nll_bwd_h16(const uint16_t* logits16, long ldl, const float* lse, const int64_t* ids, long ids_stride, int tgt_off,
                           const float* rowscale, uint16_t* dlogits, long ldo, int T, int B, int V, void* stream);
/* src f32 [R][C](lds) -> dst bf16 [R][C](ldd) and/or dstT bf16 [C][R](ldt), round-to-nearest-even; either may be NULL */
int lv_cvt_bf16_f32(const float* src, long lds, int R, int C, uint16_t* dst, long ldd, uint16_t* dstT, long ldt,
                    void* stream);
/* the same images with nn.Dropout folded in (dec_lstm.py:106, dropout_out on the decoder LSTM's output): src = h time-major
 * [T*Bsz][C] (row t*Bsz + b), keep = the reference-layout mask [Bsz][T][C] (uint8): images of h * (keep ? kscale : 0).  And its
 * backward on dO, in place.  (The persistent recurrences then run without a mask: +0.3 us per timestep otherwise.) */
int lv_cvt_bf16_keep_f32(const float* src, long lds, int T, int Bsz, int C, const uint8_t* keep, float kscale,
                         uint16_t* dst, long ldd, uint16_t* dstT, long ldt, void* stream);
/* The decoder's three images of its hidden states in ONE pass: src = hs [(T + 1) * Bsz][C] time-major with the initial state in
 * front (row t*Bsz + b = h_{t-1}[b]).  hT [C][T*Bsz](ldh) = the transposed image of rows [0, T*Bsz) (h_{t-1}: the operand of dW_hh),
 * exactly lv_cvt_bf16_f32's; dst [T*Bsz][C](ldd) / dstT [C][T*Bsz](ldt) = the images of rows [Bsz, (T + 1)*Bsz) (h_t, the LSTM output),
 * exactly lv_cvt_bf16_keep_f32's with (keep, kscale), or lv_cvt_bf16_f32's when keep is NULL.  All three are required. */
int lv_cvt_bf16_hs3_f32(const float* src, long lds, int T, int Bsz, int C, const uint8_t* keep, float kscale, uint16_t* dst, long ldd,
                        uint16_t* dstT, long ldt, uint16_t* hT, long ldh, void* stream);
/* dst f32 [n] = bf16 src [n] * scale: unpacks a bf16 gradient payload of the data-parallel exchange (dist.GradSync payload="bf16") */
int lv_cvt_f32_bf16_scaled(const uint16_t* src, long n, float scale, float* dst, void* stream);
int lv_keep_scale_f32(float* x, const uint8_t* keep, float kscale, int T, int Bsz, int C, void* stream);

/* LSTM gate weight W [4H][C] (rows g*H + u): dst = bf16 image with rows in unit-major order (4u + g), dstT = bf16 image
 * of W^T [C][4H] in the standard order; either may be NULL */
int lv_cvt_bf16_gates_f32(const float* src, long lds, int H, int C, uint16_t* dst, long ldd, uint16_t* dstT, long ldt,
                          void* stream);
/* The LOW half of a split-bf16 operand, bf16(x - bf16(x)), in the layouts of the three conversions above: a plain matrix [R][C]
 * (gate_H = 0, ids = NULL), an LSTM gate weight with unit-major rows (gate_H = H, R = 4H), or gathered embedding rows (ids [Bsz]
 * [ids_stride], R = T*Bsz).  x = hi + lo up to 2^-17 |x|; hi.hi' + hi.lo' + lo.hi' on the bf16 pipe (lv_gemm_b16 with
 * accumulate = 1) is an f32-like product.  Used by the encoder's exact forward (enc_lstm.py:47-64 -> encoder.py:55: the KL is a
 * function of the forward's last state, and WEIGHT rounding is what moves it -- profiles/r05a_kl_ablation.txt). */
int lv_cvt_bf16_lo_f32(const float* src, long lds, int R, int C, int gate_H, const int64_t* ids, long ids_stride, int Bsz, int V,
                       uint16_t* dst, long ldd, uint16_t* dstT, long ldt, void* stream);
/* Operand images for a forward product on the BINARY16 matrix pipe: dst = IEEE half (RNE) in the plain / unit-major gate rows / gathered
 * embedding rows layouts (arguments as lv_cvt_bf16_lo_f32), dstT = the transposed BF16 image the gradient products of the same operand
 * read.  lv_gemm_h16 = lv_gemm_b16 (transA = 0, 128 x 128 tile) on such operands: v_mfma_f32_32x32x16_f16, f32 accumulation.  The
 * encoder's input projection X W_ih^T (enc_lstm.py:50-55).  Values beyond +-65504 saturate. */
int lv_cvt_h16_f32(const float* src, long lds, int R, int C, int gate_H, const int64_t* ids, long ids_stride, int Bsz, int V,
                   uint16_t* dst, long ldd, uint16_t* dstT, long ldt, void* stream);
int lv_gemm_h16(int M, int N, int K, float alpha, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                float* C, long ldc, int accumulate, const float* add1, long ld1, int mod1,
                const float* add2, long ld2, int mod2, float* ws, long ws_floats, void* stream);
/* out[cols][rows] = in[rows][cols]^T  (W_hh^T for BPTT) */
int lv_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
int lv_transpose_ld_f32(const float* in, long in_ld, float* out, long out_ld, int rows, int cols, void* stream);

/* ---- LSTM time recurrence: nn.LSTM forward (enc_lstm.py:60, dec_lstm.py:104) and its autograd backward --------
 * gx [T][B][4H] input projection (+biases, + z term); whh [4H][H] (rows i|f|g|o); hs, cs [T+1][B][H] with index 0
 * = initial state supplied by the caller; gates: T*B*4H floats of activated gates saved for BPTT (opaque: unit-major
 * (i,f,g,o) records, written by the forward and read back only by lv_lstm_bwd_*).
 * dmask (optional) uint8 [B][T][H] keep-mask of nn.Dropout on the outputs (dec_lstm.py:106): hdrop[t] =
 * hs[t+1]*mask*dscale;  with dmask == NULL and hdrop != NULL, hdrop is a copy of the outputs. */
int lv_lstm_fwd_f32(const float* gx, const float* whh, float* hs, float* cs, float* gates,
                    const uint8_t* dmask, float dscale, float* hdrop, float* ws, int T, int B, int H, void* stream);
/* same recurrence with the h W_hh^T product on the bf16 matrix pipe (throughput configuration; f32 accumulate/state) */
int lv_lstm_fwd_bf16(const float* gx, const float* whh, float* hs, float* cs, float* gates,
                     const uint8_t* dmask, float dscale, float* hdrop, float* ws, int T, int B, int H, void* stream);
/* lv_lstm_fwd_bf16 for a gx whose 4H columns are UNIT-major (column 4u + g instead of g*H + u): each workgroup then
 * fetches a unit's four gate pre-activations with one 16-byte load.  Such a gx is what lv_gemm_b16 produces from the
 * lv_cvt_bf16_gates_f32 image of W_ih and lv_gate_interleave_f32-ed epilogue addends. */
int lv_lstm_fwd_bf16_ug(const float* gx, const float* whh, float* hs, float* cs, float* gates,
                        const uint8_t* dmask, float dscale, float* hdrop, float* ws, int T, int B, int H, void* stream);
/* the exact-f32 recurrence (lv_lstm_fwd_f32) on a UNIT-major gx: nn.LSTM of enc_lstm.py:55 in f32 behind an input projection in
 * the bf16-image path's column order */
int lv_lstm_fwd_f32_ug(const float* gx, const float* whh, float* hs, float* cs, float* gates,
                       const uint8_t* dmask, float dscale, float* hdrop, float* ws, int T, int B, int H, void* stream);
/* The same recurrences as ONE persistent launch each (lv_lstm_persist16.hip; nn.LSTM of enc_lstm.py:55 / dec_lstm.py:104, forward
 * and BPTT): 256 workgroups in 8 XCD-sized groups (blockIdx % 8), each group carries a slice of the batch through all T steps with
 * its slice of W_hh held in registers and hands h_t (forward: all-gather) or partial dh sums (BPTT: reduce-scatter) around inside
 * the group through tagged 16-byte granules (every dword under a tag of its own: no 16-byte atomicity assumed).  R rows per group (1 <= R <= 16, 8 R >= B), groups [0, ceil(B / R)) carry the batch and
 * the workgroups of the remaining groups return at once -- B = 32 runs 4 rows on each of the 8 groups, B = 128 sixteen (BASELINE.json
 * configs[4]), and R = 8 at B = 32 runs a recurrence on FOUR XCDs.  Contraction on the 16 x 16 x 32 MFMA with the weights as the A
 * operand.  gx unit-major as for lv_lstm_fwd_bf16_ug.  Weight images: lv_lstm_persist16_pack(whh, wpk, backward, H)
 * (lv_lstm_persist16_wpk_floats() floats each; a caller whose weights do not change between calls -- the decoder during the
 * aggressive inner loop, text.py:371-400 -- packs once); exchange buffer: lv_lstm_persist16_xch_floats() floats; *status (device
 * int, zeroed by the caller) becomes non-zero if a bounded hand-off spin ran out (see lv_clip_norm2_txn_f32 for what the fused
 * driver does about it).  No in-kernel
 * dropout (the caller applies dropout_out on the bf16 images of h and once on dO).  flags bit 0: the hand-off granules are stored
 * without the agent-scope write-through, i.e. they stay in the XCD's L2 instead of travelling to memory (valid while every group is
 * XCD-local, which the round-robin workgroup placement of a 256-CU device gives; a violated assumption shows up as a hand-off
 * timeout in *status).  LV_ERR_UNSUPPORTED unless H == 1024 and the device has >= 256 CUs.
 * saved: what the forward keeps for the BPTT (the gates i, f, g, o and the cell states c_0 .. c_{T-1}), in the kernels' own
 * WORKGROUP-MAJOR order -- saved[group][member][t]{ gates [R][32 units][4], c [R][32 units] }: lv_lstm_persist16_saved_floats(T, R)
 * floats, opaque to the caller, and the BPTT call must be given the T, B, R of the forward that wrote it.  (In [t][b][...] order
 * every timestep of every array is a different page at B = 128, and the address translations of a block of loads serialise in
 * front of the next hand-off poll: 1.5 us of a 7.9 us BPTT timestep.)  hs: [T + 1][B][H] as everywhere; cs: [T + 1][B][H], of which
 * these kernels read slot 0 (the initial state) and write slot T (the final one) only. */
long lv_lstm_persist16_wpk_floats(void);
/* exchange buffer [forward half 0 | forward half 1 | BPTT half 0 | BPTT half 1].  flags bit 1 (2) of the two launches: double-buffered
 * -- bit 2 (4) names the half this launch uses, which must be zero (allocate zeroed; alternate strictly per kind of launch); the launch
 * zeroes the OTHER half of its kind in its prologue, so no memset launch precedes it.  BPTT: bits 3..4 name the instantiation (1 / 2 / 3 =
 * up to 4 / 8 / 16 rows per group; 0 = this launch's own) of the launch that last used the other half = the extent to clear.  Without
 * bit 1: half 0 behind a hipMemsetAsync (hipGraph replays cannot alternate).  lv_lstm_persist16_xch_clear zeroes the whole buffer. */
long lv_lstm_persist16_xch_floats(void);
int lv_lstm_persist16_xch_clear(float* xch, void* stream);
long lv_lstm_persist16_saved_floats(int T, int R);
int lv_lstm_persist16_pack(const float* whh, float* wpk, int backward, int H, void* stream);
int lv_lstm_persist16_pack2(const float* whh, float* wpk_fwd, float* wpk_bwd, int H, void* stream);   /* both images, one launch */
/* BINARY16 recurrent operands for the FORWARD (flags bit 5 = 32 of lv_lstm_fwd_bf16_persist16; weight image from
 * lv_lstm_persist16_pack(.., backward = 2, ..) or lv_lstm_persist16_pack2_h16, which also writes the bf16 BPTT image): W_hh and the h
 * granules as IEEE half on v_mfma_f32_16x16x32_f16 -- 11 instead of 8 bits of significand at the same cost.  For the ENCODER
 * (enc_lstm.py:55-62): the KL of encoder.py:55 is a function of the forward's last state, and what moves that state in the bf16
 * configuration is the rounding of the WEIGHTS (the same perturbation at every timestep), not of h.  LSTM weights and h in (-1, 1) are
 * far inside binary16's range; the BPTT stays bf16 (gradients need the exponent range). */
int lv_lstm_persist16_pack2_h16(const float* whh, float* wpk_fwd, float* wpk_bwd, int H, void* stream);
int lv_lstm_fwd_bf16_persist16(const float* gx, const float* wpk, float* hs, float* cs, float* saved, float* xch, int* status,
                               int T, int B, int R, int flags, int H, void* stream);
/* The persistent forward COMPUTING ITS OWN INPUT PROJECTION (4 rows per group): instead of gx it takes the 16-bit image of the layer
 * input x16 [T * B][ldx] (bf16; binary16 with flags bit 5), the unit-major 16-bit image of W_ih wih16 [4H][ni] (row 4u + g, same format)
 * and the projection's unit-major f32 addend -- one row (addend_row_stride = 0) or row b at addend + b * addend_row_stride -- and forms
 * gx[t][b] = x16[t * B + b] . wih16^T + addend[b] four timesteps at a time in the hand-off wait of the recurrence.  The other
 * arguments as lv_lstm_fwd_bf16_persist16.  ni = 512, H = 1024 and R <= 4 only: LV_ERR_UNSUPPORTED, nothing launched, otherwise. */
int lv_lstm_fwd_bf16_persist16_x(const void* x16, long ldx, const void* wih16, int ni, const float* addend, long addend_row_stride,
                                 const float* wpk, float* hs, float* cs, float* saved, float* xch, int* status,
                                 int T, int B, int R, int flags, int H, void* stream);
int lv_lstm_bwd_bf16_persist16(const float* dh_ext, const float* dh_last, const float* wpk, const float* saved, const float* hs,
                               const float* cs, uint16_t* dG16, float* dGsum, float* xch, int* status, float* dh0, float* dc0,
                               int tanh_init, int T, int B, int R, int flags, int H, void* stream);
/* Saved activations of a forward that ran on the launch-per-timestep kernels (gates [T][B][H][4] records, cs [T+1][B][H]) -> the
 * record buffer lv_lstm_bwd_bf16_persist16 reads, for the same T, B, R.  Used when the ENCODER's forward recurrence runs in exact
 * f32 (the KL of encoder.py:55 is a function of its last state, enc_lstm.py:60-62) in front of the persistent BPTT. */
int lv_lstm_persist16_import_saved(const float* gates, const float* cs, float* saved, int T, int B, int R, int H, void* stream);
/* out[r][4u + g] = a[r][g*H + u] (+ b[r][g*H + u]): gate-major rows (biases, the decoder's z-projection) -> unit-major */
int lv_gate_interleave_f32(const float* a, const float* b, int R, int H, float* out, void* stream);
int lv_lstm_bwd_bf16(const float* dh_ext, const float* dh_last, const uint8_t* dmask, float dscale,
                     const float* whh, const float* gates, const float* hs, const float* cs,
                     float* dG, float* dGsum, float* ws, float* dh0, float* dc0, int tanh_init,
                     int T, int B, int H, void* stream);
/* lv_lstm_bwd_bf16 that also (or only) writes dG16, the bf16 image of dG ([T][B][4H], bits identical to
 * lv_cvt_bf16_f32 of dG) that lv_gemm_b16 consumes for dX / dW_ih / dW_hh; either of dG / dG16 may be NULL, not both. */
int lv_lstm_bwd_bf16_img(const float* dh_ext, const float* dh_last, const uint8_t* dmask, float dscale,
                           const float* whh, const float* gates, const float* hs, const float* cs,
                           float* dG, uint16_t* dG16, float* dGsum, float* ws, float* dh0, float* dc0, int tanh_init,
                           int T, int B, int H, void* stream);
/* floats of caller-owned scratch (16-byte aligned) both LSTM entry points need: MFMA-fragment-major packed copies of
 * W_hh and of the recurrent state, split-K slabs */
long lv_lstm_ws_floats(int B, int H);
/* number of split-K slabs the BPTT matmul writes per step (informational) */
int lv_lstm_bwd_ksplit(int H);
/* BPTT.  dh_ext (optional) [T][B][H] grad wrt every output (times dmask*dscale when dmask given); dh_last
 * (optional) [B][H] grad wrt the final output only (encoder: enc_lstm.py:60-62 uses last_state only).
 * Outputs: dG [T][B][4H] grad wrt pre-activations; dGsum [B][4H] = sum_t dG[t]; dc0/dh0 (optional) grads wrt the
 * initial state; tanh_init = 1 when h0 = tanh(c0) (dec_lstm.py:99-101): then dc0 includes the path through h0. */
int lv_lstm_bwd_f32(const float* dh_ext, const float* dh_last, const uint8_t* dmask, float dscale,
                    const float* whh, const float* gates, const float* hs, const float* cs,
                    float* dG, float* dGsum, float* ws, float* dh0, float* dc0, int tanh_init,
                    int T, int B, int H, void* stream);
/* Variable-length batches: nn.LSTM on a pack_padded_sequence (VarLSTMEncoder enc_lstm.py:97-101, VarLSTMDecoder
 * dec_lstm.py:419-428) as the recurrences above on the PADDED time-major buffers.  steps: int32 [B] on the device, row b is
 * active at timestep t when t < steps[b] (encoder: the sentence length; decoder: length - 1); max_steps: the host's bound on its
 * entries, 0 <= max_steps <= T (refused otherwise; the kernels only compare t < steps[b], so no entry can reach past T).
 * lv_lstm_fwd_len_f32 = lv_lstm_fwd_f32 where every step is active; an inactive step carries hs[t+1][b] = hs[t][b],
 * cs[t+1][b] = cs[t][b] (hs[T] is each row's own last state: last_state of enc_lstm.py:101), writes hdrop[t][b] = 0 (the zero
 * rows of pad_packed_sequence, dec_lstm.py:428) and leaves its gate record unspecified.
 * lv_lstm_bwd_len_f32 = lv_lstm_bwd_f32 where every step is active; at an inactive step dG[t][b] = 0 exactly and dh_ext[t][b],
 * the gate record and cs[t+1][b] are not read; dh_last enters row b at its own last step t = steps[b] - 1.  A row with
 * steps[b] <= 0 gets dG = dGsum = dh0 = dc0 = 0.  Same scratch as the equal-length entries (lv_lstm_ws_floats). */
int lv_lstm_fwd_len_f32(const float* gx, const float* whh, float* hs, float* cs, float* gates,
                        const uint8_t* dmask, float dscale, float* hdrop, float* ws,
                        const int* steps, int max_steps, int T, int B, int H, void* stream);
int lv_lstm_bwd_len_f32(const float* dh_ext, const float* dh_last, const uint8_t* dmask, float dscale,
                        const float* whh, const float* gates, const float* hs, const float* cs,
                        float* dG, float* dGsum, float* ws, float* dh0, float* dc0, int tanh_init,
                        const int* steps, int max_steps, int T, int B, int H, void* stream);
/* token NLL [T][B] of such a batch: entries with t >= steps[b] set to zero in front of lv_vae_loss_f32 -- the weight-0 <pad>
 * targets of VarLSTMDecoder's loss (dec_lstm.py:376-378, 471-476) */
int lv_nll_mask_len_f32(float* nll, const int* steps, int max_steps, int T, int B, void* stream);

/* ---- embeddings: nn.Embedding forward (enc_lstm.py:58, dec_lstm.py:80) fused with dropout_in (dec_lstm.py:81);
 * aten::embedding_dense_backward as a deterministic sorted-segment sum (padding_idx row skipped: dec_lstm.py:28) */
int lv_embed_gather_f32(const float* emb, const int64_t* ids, long ids_stride, const uint8_t* mask, float scale,
                        float* X, int T, int B, int ni, int V, void* stream);
/* The same lookup written straight into the bf16 operand images lv_gemm_b16 consumes (throughput configuration): dst [T*Bsz][C]
 * (row t*Bsz + b) and/or dstT [C][T*Bsz]; keep = the dropout keep-mask [Bsz][T][C] or NULL.  Bit-identical to
 * lv_embed_gather_f32 + lv_cvt_bf16_f32 (enc_lstm.py:50-52, dec_lstm.py:86-93). */
int lv_embed_gather_b16(const float* emb, const int64_t* ids, long ids_stride, const uint8_t* keep, float kscale,
                        int T, int Bsz, int C, int V, uint16_t* dst, long ldd, uint16_t* dstT, long ldt, void* stream);
int lv_token_sort(const int64_t* ids, long ids_stride, int T, int B, int V,
                  int* out_rows, int* out_tok, int* tmp /* 2*T*B ints */, void* stream);
int lv_embed_scatter_f32(const float* dX, const uint8_t* mask, float scale, const int* sorted_rows,
                         const int* sorted_tok, int T, int B, float* dE, int ni, int pad_idx, int accumulate,
                         void* stream);
/* the same sums with dE [V][ni] COMPLETE: the rows of tokens that do not occur in the batch (and pad_idx) are written as zeros
 * by the same launch -- the embedding gradient of nn.Embedding (enc_lstm.py:33, dec_lstm.py:34) without a fill of the table */
int lv_embed_scatter_full_f32(const float* dX, const uint8_t* mask, float scale, const int* sorted_rows,
                              const int* sorted_tok, int T, int B, float* dE, int ni, int V, int pad_idx, void* stream);
/* lv_embed_scatter_full_f32 and, in the same pass, the sum of squares of the table gradient it completes: sq[0 .. parts) receives
 * one partial per wave (parts = lv_embed_scatter_sumsq_parts(T, B)); sq_only != 0: dE is NOT written (see lv_gemm_b16_sumsq). */
int lv_embed_scatter_sumsq_parts(int T, int B);
int lv_embed_scatter_full_sumsq_f32(const float* dX, const uint8_t* mask, float scale, const int* sorted_rows,
                                    const int* sorted_tok, int T, int B, float* dE, int ni, int V, int pad_idx, float* sq, int sq_only,
                                    void* stream);
/* Data parallel, row-list exchange of the embedding gradient (new design; the reference has no distributed code): the
 * dense MEAN gradient dE [V][ni] rebuilt from every rank's (sorted token ids, gradient rows) list -- ids_all int64 [world][cap]
 * (ascending, -1 padded), rows_all [world][cap][ni] f32 (b16 = 0) or bf16 (b16 = 1) --, rows added in rank order (deterministic),
 * times scale (1 / world); rows no rank touched are written as zeros. */
int lv_rows_merge_f32(const int64_t* ids_all, const void* rows_all, int b16, int world, int cap, int ni, int V, float scale,
                      float* dE, void* stream);

/* ---- reparameterise + analytic KL: GaussianEncoderBase.encode / reparameterize (modules/encoders/encoder.py:40-79)
 * mulv [B][2nz] = mu | logvar; eps [B][ns][nz] is an input (host RNG in parity mode, lv_rng_* otherwise). */
int lv_reparam_kl_fwd_f32(const float* mulv, const float* eps, float* z, float* kl, int B, int ns, int nz, void* stream);
int lv_reparam_kl_bwd_f32(const float* mulv, const float* eps, const float* dz, const float* dkl, float* dmulv,
                          int B, int ns, int nz, void* stream);

/* ---- token NLL: nn.CrossEntropyLoss(reduce=False) + view().sum(-1) (dec_lstm.py:45-47,143-148) ----------------
 * logits [T*B][ldl]; target of row (t,b) = ids[b*ids_stride + t + tgt_off].  bwd rewrites logits in place with
 * (softmax - onehot) * rowscale[b]. */
int lv_softmax_nll_fwd_f32(const float* logits, long ldl, const int64_t* ids, long ids_stride, int tgt_off,
                           float* lse, float* nll, int T, int B, int V, void* stream);
int lv_softmax_nll_bwd_f32(float* logits, long ldl, const float* lse, const int64_t* ids, long ids_stride, int tgt_off,
                           const float* rowscale, int T, int B, int V, void* stream);
/* same gradient written as bf16 into dlogits [T*B][ldo] (pad columns zeroed); logits are left untouched */
int lv_softmax_nll_bwd_b16(const float* logits, long ldl, const float* lse, const int64_t* ids, long ids_stride, int tgt_off,
                           const float* rowscale, uint16_t* dlogits, long ldo, int T, int B, int V, void* stream);
/* VAE.loss assembly (modules/vae.py:95-98): rec[b] = sum_t nll[t][b]; loss[b] = rec[b] + kl_weight*kl[b] */
int lv_vae_loss_f32(const float* nll, const float* kl, const float* kl_weight_dev, float* loss, float* rec,
                    int T, int B, void* stream);
/* upstream grads (each may be NULL) -> rowscale[b] = g_loss+g_rec, dkl[b] = kl_weight*g_loss+g_kl */
int lv_loss_bwd_scales_f32(const float* g_loss, const float* g_rec, const float* g_kl, const float* kl_weight_dev,
                           float* rowscale, float* dkl, int B, void* stream);
/* The fused driver's form of the three entries above plus the running report sums (text.py:381,426-427), one launch:
 * rec[b] = sum_t nll[t][b]; loss[b] = rec[b] + w*kl[b]; acc_dev[0..2] += sum_b (loss, rec, kl); rowscale[b] = g_loss[b];
 * dkl[b] = w*g_loss[b] (the seeds of loss.mean().backward(), text.py:382-384) */
int lv_loss_assemble_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                         float* loss, float* rec, float* rowscale, float* dkl, float* acc_dev, int T, int B, void* stream);
/* the same + rng_state[1] += rng_inc (the {seed, offset} state of lv_rng_noise_step, which the fused step then calls with inc = 0) */
int lv_loss_assemble_rng_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                             float* loss, float* rec, float* rowscale, float* dkl, float* acc, int T, int B,
                             uint64_t* rng_state, uint64_t rng_inc, void* stream);

/* ---- multi-sample training, VAE.loss(x, kl_weight, nsamples = ns) (lv_multisample.hip) -----------------------------------
 * The reference expands a sentence's word embeddings (after dropout_in) over the ns samples and runs the decoder on B*ns rows,
 * row b*ns + s (dec_lstm.py:83-99); the word half of the input projection is the same for a sentence's ns rows, so it is
 * computed on B rows and expanded: gx[t][b*ns + s][:] = gxw[t][b][:] + zp[b*ns + s][:].  gxw [Td][B][C] (X . W_ih[:, :ni]^T),
 * zp [B*ns][C] (lv_dec_init_f32's z-projection, biases included), gx [Td][B*ns][C]; any column order the two share. */
int lv_gx_expand_add_f32(const float* gxw, const float* zp, float* gx, int Td, int B, int ns, int C, void* stream);
/* its backward counterpart (autograd of the .expand in dec_lstm.py:86-89): dgs[t][b][:] = sum_s dg[t][b*ns + s][:], added in
 * the order s = 0 .. ns-1 in f32; dg [Td][B*ns][C], dgs [Td][B][C] */
int lv_sample_sum_f32(const float* dg, float* dgs, int Td, int B, int ns, int C, void* stream);
/* the same on bf16 images with row strides ld_in / ld_out (elements): summed in f32, rounded to nearest even once */
int lv_sample_sum_b16(const uint16_t* dg, long ld_in, uint16_t* dgs, long ld_out, int Td, int B, int ns, int C, void* stream);
/* token ids in decoder row order, x_rep[b*ns + s][:] = x[b][:] (the target `tgt.expand(batch, ns, seq).view(-1)` of
 * dec_lstm.py:135-141): x int64 [B][T] -> x_rep [B*ns][T] */
int lv_repeat_rows_i64(const int64_t* x, int64_t* x_rep, int B, int T, int ns, void* stream);
/* lv_loss_assemble_f32 with samples (dec_lstm.py:146-148 `.mean(dim=1)`, vae.py:95-98): nll [T][B*ns];
 * rec[b] = (1/ns) sum_s sum_t nll[t][b*ns + s]; loss[b] = rec[b] + w*kl[b]; acc_dev[0..2] += sum_b (loss, rec, kl);
 * rowscale[b*ns + s] = g_loss[b] / ns; dkl[b] = w*g_loss[b].  ns = 1 gives lv_loss_assemble_f32's bits. */
int lv_loss_assemble_ns_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                            float* loss, float* rec, float* rowscale, float* dkl, float* acc_dev, int T, int B, int ns,
                            void* stream);
/* the same + rng_state[1] += rng_inc, as lv_loss_assemble_rng_f32 */
int lv_loss_assemble_ns_rng_f32(const float* nll, const float* kl, const float* kl_weight_dev, const float* g_loss,
                                float* loss, float* rec, float* rowscale, float* dkl, float* acc_dev, int T, int B, int ns,
                                uint64_t* rng_state, uint64_t rng_inc, void* stream);

/* ---- training on the importance-weighted bound, objective "iw" (lv_iw.hip): loss_b = -(logsumexp_s log w_s - log ns),
 * log w_s = -rec_s - w*(sum_j z_sj^2 / 2 - sum_j eps_sj^2 / 2 - sum_j logvar_j / 2) (log q in its eps form, exact for
 * z = mu + eps*sigma; w = kl_weight_dev[0]; w = 1 is VAE.nll_iw(x, ns, ns), vae.py:100-129), wn = softmax_s(log w), max-subtracted:
 * a weight may underflow to exactly 0.  nll [T][B*ns] (T = 1: nll holds rec_s itself); mulv [B][2nz]; eps, z [B][ns][nz];
 * rec[b] = (1/ns) sum_s rec_s; rowscale[b*ns + s] = g_loss[b]*wn_s (seed of the decoder backward); wz[b][s] = w*rowscale[b*ns + s];
 * logw [B][ns] may be NULL; acc_dev[0..2] += sum_b (loss, rec, kl) with kl [B] the analytic KL, reported only.  Any ns >= 1;
 * ns = 1 gives wn = 1 and rowscale = g_loss bit for bit. */
int lv_loss_assemble_iw_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                            const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                            float* wz, float* logw, float* acc_dev, int T, int B, int ns, int nz, void* stream);
/* the same + rng_state[1] += rng_inc, as lv_loss_assemble_ns_rng_f32 */
int lv_loss_assemble_iw_rng_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                float* wz, float* logw, float* acc_dev, int T, int B, int ns, int nz, uint64_t* rng_state,
                                uint64_t rng_inc, void* stream);
/* the weights' direct gradient for the autograd route (dz itself travels through lv_reparam_kl_bwd_f32): dmulv [B][2nz] ('='),
 * dmu_j = sum_s c_s z_sj, dlogvar_j = sum_s c_s z_sj eps_sj sigma_j / 2 - sum_s c_s / 2, c = wz [B][ns] */
int lv_reparam_iw_bwd_f32(const float* mulv, const float* eps, const float* wz, float* dmulv, int B, int ns, int nz, void* stream);
/* the doubly-reparameterised estimator of the same objective (DReG, Tucker et al. 2019): every output of
 * lv_loss_assemble_iw_f32 bit for bit except wz, plus rs [B][ns] = r_s = 1 - w*(1 - wn_s) (exactly 1 at wn_s = 1, so at ns = 1) and
 * wz[b][s] = c'_s = (w*rowscale[b*ns + s])*r_s = w*g*u_s with u_s = (1 - w)*wn_s + w*wn_s^2. */
int lv_loss_assemble_dreg_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                              const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                              float* wz, float* rs, float* logw, float* acc_dev, int T, int B, int ns, int nz, void* stream);
int lv_loss_assemble_dreg_rng_f32(const float* nll, const float* mulv, const float* eps, const float* z, const float* kl,
                                  const float* kl_weight_dev, const float* g_loss, float* loss, float* rec, float* rowscale,
                                  float* wz, float* rs, float* logw, float* acc_dev, int T, int B, int ns, int nz,
                                  uint64_t* rng_state, uint64_t rng_inc, void* stream);
/* the complete dmulv [B][2nz] ('=') from the decoder's dz [B][ns][nz] (carrying g*wn_s), one launch, one thread per (b, j), serial
 * over s.  rs == NULL (wz = c of lv_loss_assemble_iw_f32): t_sj = dz_sj + c_s z_sj, dmu_j = sum_s t_sj,
 * dlogvar_j = sum_s t_sj eps_sj sigma_j / 2 - sum_s c_s / 2; with wz all zeros the bits of lv_reparam_kl_bwd_f32 with dkl all zeros.
 * rs != NULL (wz = c', rs = r of lv_loss_assemble_dreg_f32): t_sj = r_s dz_sj + c'_s (z_sj - eps_sj exp(-logvar_j/2)),
 * dmu_j = sum_s t_sj, dlogvar_j = sum_s t_sj eps_sj sigma_j / 2. */
int lv_reparam_iwdz_bwd_f32(const float* mulv, const float* eps, const float* dz, const float* wz, const float* rs, float* dmulv,
                            int B, int ns, int nz, void* stream);

/* ---- the free-bits (KL thresholding) objective (lv_freebits.hip; Kingma et al. 2016, Chen et al. 2017, Li et al. 2019) ----
 * Per sentence b and latent dimension j, KL_bj = 0.5 (mu_bj^2 + exp(lv_bj) - lv_bj - 1).  lam = free_bits >= 0, in nats PER LATENT
 * DIMENSION in every mode.  The gate g is a constant of the step (no gradient flows through it); all comparisons are strict (>).
 *   mode 0 "dim":        statistic KL_bj;                                       g_bj = KL_bj > lam;    kl_obj_b = sum_j (g_bj ? KL_bj : lam)
 *   mode 1 "batch_dim":  m_j = (sum_b KL_bj) / B, summed in ascending b;        g_bj = g_j = m_j > lam; kl_obj_b = sum_j (g_j ? KL_bj : lam)
 *   mode 2 "batch":      m = (sum_b kl_b) / B, ascending b, kl_b = sum_j KL_bj; g_bj = g = m > tau;    kl_obj_b = g ? kl_b : tau,
 *                        tau = (float)(nz * lam) formed on the host in double
 * loss_b = rec_b + w * kl_obj_b ("batch_dim": mean_b loss_b = mean_b rec_b + w sum_j max(lam, m_j)).  Gradient of the KL term:
 * d kl_obj_b / d mu_bj = g_bj mu_bj, d kl_obj_b / d lv_bj = g_bj 0.5 (exp(lv_bj) - 1); the path through z is unchanged.  The
 * REPORTED KL (VAE.loss's third value, the trainers' kl_sum) stays the analytic, unthresholded one; loss_sum is the objective that
 * was minimised; no evaluation function applies free bits.
 *
 * mulv [B][2nz] -> kl_obj [B], gate [B][nz] (0.0f / 1.0f), stat (may be NULL; [B][nz] / [nz] / [1] in mode 0 / 1 / 2: the
 * statistic that was compared).  One workgroup, no atomics, batch sums in ascending b; any B >= 1, nz >= 1.  A mode outside 0..2
 * or a NULL output returns before any write.  This raw entry takes any lam (a negative one opens every gate; the public layers
 * refuse it).  With every gate open kl_obj is lv_reparam_kl_fwd_f32's kl bit for bit. */
int lv_kl_freebits_fwd_f32(const float* mulv, float lam, int mode, float* kl_obj, float* gate, float* stat, int B, int nz,
                           void* stream);
/* lv_reparam_kl_bwd_f32 with dkl[b] * gate[b][j] in place of dkl[b]; a gate of all ones gives its bits */
int lv_reparam_kl_gated_bwd_f32(const float* mulv, const float* eps, const float* dz, const float* dkl, const float* gate,
                                float* dmulv, int B, int ns, int nz, void* stream);
/* lv_loss_assemble_ns_f32 with loss[b] = rec[b] + w*kl_obj[b]; acc_dev[2] += sum_b kl[b] stays the analytic KL.  kl_obj = kl
 * gives lv_loss_assemble_ns_f32's bits. */
int lv_loss_assemble_fb_f32(const float* nll, const float* kl, const float* kl_obj, const float* kl_weight_dev, const float* g_loss,
                            float* loss, float* rec, float* rowscale, float* dkl, float* acc_dev, int T, int B, int ns,
                            void* stream);
/* the same + rng_state[1] += rng_inc, as lv_loss_assemble_ns_rng_f32 */
int lv_loss_assemble_fb_rng_f32(const float* nll, const float* kl, const float* kl_obj, const float* kl_weight_dev,
                                const float* g_loss, float* loss, float* rec, float* rowscale, float* dkl, float* acc_dev, int T,
                                int B, int ns, uint64_t* rng_state, uint64_t rng_inc, void* stream);

/* ---- the batch-sized ends of the two LSTM networks, one launch each (lv_head.hip) --------------------------------------
 * LSTMEncoder's head + GaussianEncoderBase.encode (enc_lstm.py:62-64, encoder.py:40-57): mulv = hT . W_lin^T,
 * z = mu + eps*exp(logvar/2), kl = 0.5*sum(mu^2 + exp(logvar) - logvar - 1).  hT [B][H], W_lin [2nz][H], eps/z [B][ns][nz] */
int lv_enc_head_fwd_f32(const float* hT, const float* w_lin, const float* eps, float* mulv, float* z, float* kl,
                        int B, int H, int ns, int nz, void* stream);
/* ... and its backward: (dz, dkl) -> dmulv [B][2nz], dhT [B][H], gW_lin [2nz][H] ('=').  dz: [dz_parts][B][ns][nz],
 * summed over the leading index in order (1 for a plain gradient; lv_dec_tail_parts(H) after lv_dec_tail_bwd_f32) */
int lv_enc_head_bwd_f32(const float* mulv, const float* eps, const float* dz, int dz_parts, const float* dkl,
                        const float* hT, const float* w_lin, float* dmulv, float* dhT, float* gw_lin, int B, int H, int ns,
                        int nz, void* stream);
/* the same for the importance-weighted objective: wz [B][ns] (c_s of lv_loss_assemble_iw_f32) in place of dkl;
 * t_sj = dz_sj + c_s z_sj, dmu_j = sum_s t_sj, dlogvar_j = sum_s t_sj eps_sj sigma_j / 2 - sum_s c_s / 2.  With wz all zeros the
 * three outputs are bit-identical to lv_enc_head_bwd_f32 with dkl all zeros. */
int lv_enc_head_iw_bwd_f32(const float* mulv, const float* eps, const float* dz, int dz_parts, const float* wz,
                           const float* hT, const float* w_lin, float* dmulv, float* dhT, float* gw_lin, int B, int H, int ns,
                           int nz, void* stream);
/* the same under the doubly-reparameterised estimator: wz = c', rs = r [B][ns] of lv_loss_assemble_dreg_f32, the per-sample terms of
 * lv_reparam_iwdz_bwd_f32 with rs != NULL.  With wz all zeros and rs all ones the three outputs are bit-identical to
 * lv_enc_head_bwd_f32 with dkl all zeros.  rs is read from global memory: the LDS envelope is lv_enc_head_bwd_f32's. */
int lv_enc_head_dreg_bwd_f32(const float* mulv, const float* eps, const float* dz, int dz_parts, const float* wz, const float* rs,
                             const float* hT, const float* w_lin, float* dmulv, float* dhT, float* gw_lin, int B, int H, int ns,
                             int nz, void* stream);
/* lv_enc_head_bwd_f32 under free bits: dkl[b] * gate[b][j] (gate [B][nz] of lv_kl_freebits_fwd_f32) in place of dkl[b].  With a
 * gate of all ones every output is bit-identical to lv_enc_head_bwd_f32's. */
int lv_enc_head_gated_bwd_f32(const float* mulv, const float* eps, const float* dz, int dz_parts, const float* dkl,
                              const float* gate, const float* hT, const float* w_lin, float* dmulv, float* dhT, float* gw_lin,
                              int B, int H, int ns, int nz, void* stream);
/* LSTMDecoder.decode's z-dependent prologue (dec_lstm.py:95-101): c0 = z W_trans^T, h0 = tanh(c0) (G7) and
 * Zp = z W_ih[:, col0:col0+nz]^T + b_ih + b_hh, the contribution of cat((word_embed, z_), -1) to the input projection;
 * Zp gate-major [B][4H], or with column 4u+g (unit_major != 0) for the unit-major Gx epilogue */
int lv_dec_init_f32(const float* z, const float* w_trans, const float* w_ih, long ld_wih, int col0, const float* b_ih,
                    const float* b_hh, float* c0, float* h0, float* zp, int unit_major, int B, int H, int nz, void* stream);
/* ... and its backward from the BPTT's sums: dGsum [B][4H] (gate-major), dc0 [B][H] -> gW_ih[:, col0:col0+nz] (ld_gwih),
 * g_b_ih, g_b_hh, gW_trans ('=') and dz = dGsum . W_ih[:, col0:] + dc0 . W_trans as lv_dec_tail_parts(H) partial sums
 * dz_parts [parts][B][nz] over slices of the contraction (summed in order by lv_enc_head_bwd_f32 / lv_colsum_f32) */
int lv_dec_tail_parts(int H);
int lv_dec_tail_bwd_f32(const float* dGsum, const float* dc0, const float* z, const float* w_ih, long ld_wih, int col0,
                        const float* w_trans, float* gw_ih, long ld_gwih, float* gw_trans, float* gb_ih, float* gb_hh,
                        float* dz_parts, int B, int H, int nz, void* stream);
/* the dz half of the same for a frozen decoder (VAE.refine_posterior): dz_parts [parts][B][nz] only, bit-equal to
 * lv_dec_tail_bwd_f32's; no weight or bias gradient is formed or written */
int lv_dec_tail_dz_f32(const float* dGsum, const float* dc0, const float* w_ih, long ld_wih, int col0, const float* w_trans,
                       float* dz_parts, int B, int H, int nz, void* stream);

/* ---- posterior refinement by SVI on the encoder's output (lv_svi.hip; Cremer et al. 2018, the inference half of SA-VAE) ---
 * Per sentence b, phi = mulv[b] = (mu | logvar), fixed noise eps [B][ns][nz], beta = kl_weight_dev[0]:
 *   L_b(phi) = (1/ns) sum_s rec(x_b, mu + eps_s*exp(logvar/2)) + beta * 0.5*sum_j(mu_j^2 + exp(logvar_j) - logvar_j - 1).
 * One launch per iteration: trace_row[b] = (1/ns) sum_s rec[b*ns + s] + beta*kl[b] (the CURRENT iterate's L_b); where that is
 * strictly below best_loss[b] it replaces it and phi is copied to best_mulv[b] (a tie keeps the earlier iterate); then, unless
 * dz is NULL (finish mode: nothing else is read or written),
 *   g = gradient of lv_reparam_kl_bwd_f32 with seeds dz (summed over dz_parts in order; the decoder backward carries 1/ns) and
 *       dkl = beta;  g *= min(1, clip / (|g|_2 + 1e-6)) over the sentence's 2nz values;  vel = momentum*vel + g;
 *   mulv -= lr*vel;  z_next [B][ns][nz], kl_next [B] = lv_reparam_kl_fwd_f32 of the updated mulv, bit for bit.
 * rec [B*ns], kl [B]; mulv, vel, best_mulv [B][2nz] and best_loss [B] are in/out.  lr, clip > 0, 0 <= momentum < 1. */
int lv_svi_step_f32(const float* rec, const float* dz, int dz_parts, const float* eps, const float* kl,
                    const float* kl_weight_dev, float lr, float momentum, float clip, float* mulv, float* vel,
                    float* best_mulv, float* best_loss, float* trace_row, float* z_next, float* kl_next, int B, int ns,
                    int nz, void* stream);

/* ---- semi-amortized training: the backward pass through the K refinement steps (lv_savae.hip; SA-VAE, Kim et al. 2018) ------
 * lv_svi_rec_step_f32: lv_svi_step_f32's update without the loss record and the best-iterate tracking; it also stores the
 * unclipped gradient g_k and the iterate lambda_k (before the update) into g_rec, phi_rec [B][2nz], step k's rows of the
 * [K][B][2nz] records.  mulv, vel, z_next, kl_next: bit-equal to lv_svi_step_f32 on the same inputs.
 * lv_savae_adjoint_f32, one launch (one workgroup) per backward iteration k = K-1 .. 0, with lbar / vbar the adjoints of lambda / v:
 *   vb = vbar - lr*lbar;  per sentence r = |g|_2, s = clip/(r + 1e-6):  gb = vb where s >= 1, else
 *   gb = s*vb - clip*(g.vb)/(r*(r + 1e-6)^2)*g;  vbar = momentum*vb;  n = |gb|_2 over all B*2nz entries (summed in double);
 *   e = fd_eps*max(1, max|lam|);  c = n/(2e);  scal = (n, e, c);  u = gb/n (n = 0: u = 0, c = 0);
 *   z_pm [B][2ns][nz]: samples 0..ns-1 (mu + e*u_mu) + eps_s*exp((logvar + e*u_lv)/2), samples ns..2ns-1 the same at -e;
 *   seeds [B*2ns]: +c/ns on the first ns rows of a sentence, -c/ns on the others.
 * lv_savae_hvp_f32: from dz [dz_parts][B*2ns][nz] of the decoder pass at z_pm seeded with `seeds`,
 *   lbar += c*(grad_lambda F(lam + e*u) - grad_lambda F(lam - e*u)),  F = sum_b L_b,  beta = kl_weight_dev[0];
 *   the reparameterisation chain rule and the analytic-KL terms are evaluated at the perturbed points.  n = 0: lbar untouched. */
int lv_svi_rec_step_f32(const float* dz, int dz_parts, const float* eps, const float* kl_weight_dev, float lr, float momentum,
                        float clip, float* mulv, float* vel, float* g_rec, float* phi_rec, float* z_next, float* kl_next, int B,
                        int ns, int nz, void* stream);
int lv_savae_adjoint_f32(const float* lbar, float* vbar, const float* g, const float* lam, const float* eps, float lr,
                         float momentum, float clip, float fd_eps, float* u, float* scal, float* z_pm, float* seeds, int B, int ns,
                         int nz, void* stream);
int lv_savae_hvp_f32(const float* dz, int dz_parts, const float* eps, const float* lam, const float* u, const float* scal,
                     const float* kl_weight_dev, float* lbar, int B, int ns, int nz, void* stream);

/* small elementwise / reductions used by the sequencing (h0 = tanh(c0) dec_lstm.py:100; bias grads) */
int lv_tanh_f32(const float* in, float* out, long n, void* stream);
int lv_colsum_f32(const float* in, long ld, int R, int C, float* out, float* out2, void* stream);
int lv_add_f32(const float* a, const float* b, float* out, long n, void* stream);
int lv_sum_accum_f32(const float* x, long n, float* out_dev, void* stream);   /* out_dev[0] += sum(x) (text.py:381) */
int lv_add_scalar_f32(float* x_dev, float v, void* stream);

/* ---- clip_grad_norm_ (text.py:385, image.py:312) + optim.SGD (text.py:325,387) / optim.Adam (image.py:267,314)
 * over flat parameter/gradient buffers */
int lv_sumsq_workspace_floats(void);
int lv_sumsq_f32(const float* x, long n, float* ws, float* out_dev, int accumulate, void* stream);
int lv_clip_coef_f32(const float* sumsq_dev, float max_norm, float* coef_dev, float* norm_out_dev, void* stream);
/* clip_grad_norm_ over two flat gradient buffers at once (encoder + decoder: the norm spans both, G1): one streaming pass
 * over both, then sum + norm + coefficient in one single-workgroup launch.  ws: lv_sumsq_workspace_floats() floats */
int lv_clip_norm2_f32(const float* g1, long n1, const float* g2, long n2, float* ws, float max_norm,
                      float* sumsq_dev, float* coef_dev, float* norm_dev, void* stream);
int lv_sgd_step_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev, int write_back_clipped,
                    void* stream);
int lv_scale_f32(float* x, long n, const float* coef_dev, void* stream);
/* The same clip + update with a device-side TRANSACTION GATE (round 4).  The fused driver keeps the reference's per-iteration
 * host read (text.py:381 loss.sum().item()) off the step, so nothing on the host looks at a step before its update is applied
 * (text.py:385-387); a persistent LSTM launch that hit its bounded hand-off spin must therefore be caught on the DEVICE: the gate
 * runs in the clip coefficient's single thread, reads the engines' status words (and, data parallel, a guard element of the
 * exchanged gradient buffer that lv_txn_guard_f32 set), and either commits the step -- txn[1] += 1, acc[0..2] += the pending
 * (loss, rec, kl) sums txn[2..4] that lv_loss_assemble_f32 left -- or raises the sticky void flag txn[0], under which
 * lv_sgd_step_txn_f32 / lv_scale_txn_f32 are no-ops.  txn: device float[5]; acc: device float[3] or NULL; status / guard may be NULL. */
int lv_clip_norm2_txn_f32(const float* g1, long n1, const float* g2, long n2, float* ws, float max_norm,
                          float* sumsq_dev, float* coef_dev, float* norm_dev, const int* status1, const int* status2,
                          const float* guard, float* txn, float* acc, void* stream);
/* lv_clip_norm2_txn_f32 where part of the gradient arrives as the partial sums of squares its producers emitted (extra[0 .. n_extra):
 * lv_gemm_b16_sumsq, lv_embed_scatter_full_sumsq_f32): g1 / g2 are then the REST of the two flat gradients. */
int lv_clip_norm2_fold_txn_f32(const float* g1, long n1, const float* g2, long n2, float* ws, const float* extra, int n_extra,
                               float max_norm, float* sumsq_dev, float* coef_dev, float* norm_dev, const int* status1,
                               const int* status2, const float* guard, float* txn, float* acc, void* stream);
int lv_clip_coef_txn_f32(const float* sumsq_dev, float max_norm, float* coef_dev, float* norm_out_dev, const int* status1,
                         const int* status2, const float* guard, float* txn, float* acc, void* stream);
int lv_txn_guard_f32(const int* status1, const int* status2, float* guard, void* stream);
int lv_sgd_step_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev, int write_back_clipped,
                        const float* void_flag_dev, void* stream);
int lv_scale_txn_f32(float* x, long n, const float* coef_dev, const float* void_flag_dev, void* stream);
/* lv_sgd_step_txn_f32 on (p, g) and lv_scale_txn_f32 on x2 -- the gradient buffer of the side that is NOT stepped, which
 * clip_grad_norm_ (text.py:385) scales all the same -- in one launch */
int lv_sgd_step_scale_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev, int write_back_clipped,
                              float* x2, long n2, const float* void_flag_dev, void* stream);
/* The same step where elements [emb_off, emb_off + V * ni) of (p, g) are an embedding table whose gradient was written THIS step by
 * lv_embed_scatter_full* from the sorted token list sorted_tok[0 .. N) (tokens in [0, V)) and not added to since: every row no token
 * names holds +0, so p - lr * coef * 0 leaves it as it is and the launch neither reads nor writes it.  Results equal
 * lv_sgd_step_scale_txn_f32 bit for bit (void flag and write_back_clipped included); when lr or the coefficient read from the
 * device is negative, inf or NaN -- where a zero gradient does move p -- the launch walks every row like the dense entry. */
int lv_sgd_step_scale_rows_txn_f32(float* p, float* g, long n, const float* lr_dev, const float* coef_dev, int write_back_clipped,
                                   float* x2, long n2, const float* void_flag_dev, long emb_off, int V, int ni, const int* sorted_tok,
                                   int N, void* stream);
/* torch.optim.SGD(lr, momentum) with momentum > 0 (text.py --momentum: text.py:30, 325-326, re-created after a decay at 492-493;
 * dampening 0, no nesterov, no weight decay) over a flat buffer, one velocity element per parameter element in `buf`:
 *     g' = g * coef;  buf = round(round(buf * momentum) + g');  p = fma(-lr, buf, p)
 * -- the roundings of torch's buf.mul_(momentum).add_(g') and p.add_(buf, alpha=-lr), so p and buf equal torch's bit for bit.  A zeroed
 * buf is torch's missing momentum_buffer (first step: buf = g'); re-creating the optimizer is zeroing it.  g' is written back to g when
 * write_back_clipped and coef != 1.  coef_dev may be NULL (coefficient 1). */
int lv_sgd_momentum_step_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev, float momentum,
                             int write_back_clipped, void* stream);
/* lv_sgd_momentum_step_f32 behind the transaction gate (text.py:385-387 with --momentum in the fused trainer): while
 * void_flag_dev[0] != 0, p, g and buf keep their bit patterns -- a voided step moves neither the weights nor the velocity. */
int lv_sgd_momentum_step_txn_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev, float momentum,
                                 int write_back_clipped, const float* void_flag_dev, void* stream);
/* lv_sgd_momentum_step_txn_f32 on (p, g, buf) and lv_scale_txn_f32 on x2, the gradient of the side that is NOT stepped (text.py:385
 * scales it all the same), in one launch */
int lv_sgd_momentum_step_scale_txn_f32(float* p, float* g, float* buf, long n, const float* lr_dev, const float* coef_dev, float momentum,
                                       int write_back_clipped, float* x2, long n2, const float* void_flag_dev, void* stream);
int lv_adam_step_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev,
                     const float* step_dev, float beta1, float beta2, float eps, int write_back_clipped, void* stream);
/* lv_adam_step_f32 behind the transaction gate (the fused text trainer's optimizer="adam"): torch.optim.Adam (amsgrad=False,
 * weight_decay=0) on the clipped gradient, with bias corrections for step number step_dev[0] + 1; a one-thread launch queued behind the
 * update then advances step_dev[0] (the optimizer's committed-step count, one per optimizer).  While void_flag_dev[0] != 0, p, g, m, v
 * and step_dev stay bit-unchanged.  The betas are doubles, as torch's Python floats are: 1 - beta and the bias corrections are formed
 * in double and rounded to f32 where they meet the tensors, as torch rounds them. */
int lv_adam_step_txn_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev, float* step_dev,
                         double beta1, double beta2, float eps, int write_back_clipped, const float* void_flag_dev, void* stream);
/* lv_adam_step_txn_f32 on (p, g, m, v) and lv_scale_txn_f32 on x2, the gradient of the side that is NOT stepped, in one launch */
int lv_adam_step_scale_txn_f32(float* p, float* g, float* m, float* v, long n, const float* lr_dev, const float* coef_dev,
                               float* step_dev, double beta1, double beta2, float eps, int write_back_clipped, float* x2, long n2,
                               const float* void_flag_dev, void* stream);

/* ---- Philox4x32-10 draws for throughput mode (stand-in for torch's generator at encoder.py:77, dec_lstm.py:81,106)
 * state_dev: uint64[2] = {seed, offset} in device memory */
int lv_rng_normal_f32(float* out, long n, const uint64_t* state_dev, uint64_t substream, void* stream);
int lv_rng_keepmask_u8(uint8_t* out, long n, float keep_prob, const uint64_t* state_dev, uint64_t substream, void* stream);
int lv_rng_advance(uint64_t* state_dev, uint64_t inc, void* stream);
/* all the noise of one VAE.loss call in one launch: eps (substream 0), dropout_in / dropout_out keep-masks (substreams
 * 1, 2; either may be NULL), then offset += inc (lv_rng_advance queued behind it).  state_dev: uint64[2] = {seed, offset} */
int lv_rng_noise_step(float* eps, long n_eps, uint8_t* mask_in, long n_in, float keep_in, uint8_t* mask_out, long n_out,
                      float keep_out, uint64_t* state_dev, uint64_t inc, void* stream);
int lv_rng_bernoulli_f32(const float* p, float* out, long n, const uint64_t* state_dev, uint64_t substream,
                         void* stream);   /* torch.bernoulli(batch): dynamic binarisation, image.py:287,318 */

/* ---- evaluation statistics on top of the hot path's forward (lv_eval.hip) ----------------------------
 * log q(z|x) of GaussianEncoderBase.eval_inference_dist (modules/encoders/encoder.py:81-109) for z [B][ns][nz] -> out [B][ns];
 * mu == NULL: the standard normal prior of VAE.eval_prior_dist (modules/vae.py:135-145) */
int lv_gauss_logpdf_f32(const float* z, const float* mu, const float* logvar, float* out, int B, int ns, int nz, void* stream);
/* log_sum_exp(value, dim=-1) (modules/utils.py:3-16) over the rows of in [R][C] (ld), plus the constant `add`
 * (VAE.nll_iw, modules/vae.py:127: - log(nsamples)) */
int lv_logsumexp_rows_f32(const float* in, long ld, int R, int C, float add, float* out, void* stream);
/* GaussianEncoderBase.calc_mi (encoder.py:111-145) from the encoder's (mu, logvar) [Bx][nz] and the samples z [Bz][nz]:
 * out_dev[0] = MI estimate, [1] = E log q(z|x), [2] = E log q(z); ws: Bz floats */
int lv_calc_mi_f32(const float* mu, const float* logvar, const float* z, float* ws, float* out_dev, int Bx, int Bz, int nz,
                   void* stream);
/* calc_au (text.py:200-227) accumulators over posterior means mu [B][nz]: acc_dev[k] += sum_b mu[b][k] (mean == NULL) or
 * sum_b (mu[b][k] - mean[k])^2 */
int lv_au_accum_f32(const float* mu, const float* mean, float* acc_dev, int B, int nz, void* stream);

/* ---- model posterior on a latent grid (lv_grid_posterior.hip): VAE.eval_log_model_posterior / calc_model_posterior_mean
 * (modules/vae.py:170-196, 256-273), the synthetic experiment's plots (toy.py:188-231, 391-462, 482-483).
 * lv_dec_cond_ll_f32: log p(x_b | z_{b,s}) of LSTMDecoder.log_probability (dec_lstm.py:66-148, 156-161) in eval mode (no
 * dropout) for x [B][T] and K samples per sentence at z + b*z_stride ([K][nz]; z_stride = 0: one grid shared by every
 * sentence) -> cond_ll [B][K]; weights as the module stores them; ws: lv_dec_cond_ll_f32_ws_floats floats, 16-byte aligned.
 * lv_dec_cond_ll_f32_supported: 1 inside the kernel's envelope (H <= 128, nz <= 64, T >= 2), else 0 (-4 from the call). */
int lv_dec_cond_ll_f32_supported(int V, int ni, int H, int nz, int T);
long lv_dec_cond_ll_f32_ws_floats(int V, int H, int nz, int B, int T);
int lv_dec_cond_ll_f32(const int64_t* x, int B, int T, const float* z, long z_stride, int K, const float* embed,
                       const float* trans, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                       const float* pred, int V, int ni, int H, int nz, float* ws, float* cond_ll, void* stream);
/* the grid normalisation: joint = log N(z; 0, I) + cond_ll, log_post = joint - log_sum_exp_k(joint) (log_post may be NULL),
 * mean [B][nz] = sum_k exp(log_post_k) z_k */
int lv_grid_posterior_f32(const float* cond_ll, const float* z, long z_stride, int B, int K, int nz, float* log_post,
                          float* mean, void* stream);

/* ---- Metropolis-Hastings sampling from the model posterior (lv_mh.hip): VAE.sample_from_posterior (modules/vae.py:218-254).
 * A random-walk chain per (sentence, chain): next = eps * std + cur (two roundings), ratio = log p(next, x) - log p(cur, x),
 * accept = ratio >= 0 || u < exp(ratio) (a NaN ratio rejects), cur / cur_ll selected, never blended.  State in caller-owned
 * buffers: cur [B][C][nz], cur_ll [B][C], accepts [B][C] (int32 acceptance counts); samples [B][nsamples][C][nz]; iteration i
 * (counted from 0 over the whole chain) stores kept sample (i - burn_in) / thin when i >= burn_in and thin divides i - burn_in.
 * ratio_out / accept_out (float / int32, one per chain and iteration) may be NULL.  The kernels hold no generator: eps and u
 * are buffers of standard normal / uniform [0, 1) draws.
 * lv_mh_chain_f32 (vae.py:218-254): the fused route for the eval-mode LSTM decoder inside lv_dec_cond_ll_f32's envelope
 * (lv_mh_chain_f32_supported: the same answer) -- n_iter iterations iter0 .. iter0 + n_iter - 1 in one launch, one workgroup per
 * (sentence, 16 chains); eps [n_iter][B][C][nz], u [n_iter][B][C]; first != 0: score the starting point in cur first (incoming
 * cur_ll / accepts ignored, counts start at 0).  ws: lv_mh_chain_f32_ws_floats floats, 16-byte aligned, filled ONCE per chain by
 * lv_mh_chain_prep_f32 (weights as the module stores them; vae.py:218-254's x and decoder). */
int lv_mh_chain_f32_supported(int V, int ni, int H, int nz, int T);
long lv_mh_chain_f32_ws_floats(int V, int H, int nz, int B, int T);
int lv_mh_chain_prep_f32(const int64_t* x, int B, int T, const float* embed, const float* trans, const float* w_ih,
                         const float* w_hh, const float* b_ih, const float* b_hh, const float* pred, int V, int ni, int H, int nz,
                         float* ws, void* stream);
int lv_mh_chain_f32(const int64_t* x, int B, int T, const float* ws, int V, int H, int nz, int C, float* cur, float* cur_ll,
                    int* accepts, const float* eps, const float* u, int n_iter, int iter0, int burn_in, int thin, int nsamples,
                    float std, int first, float* samples, float* ratio_out, int* accept_out, void* stream);
/* lv_mh_step_f32 (vae.py:218-254, one pass of the loop at 232-251): the propose / accept glue for any decoder, rows = B * C
 * chains, any nz >= 1.  cond_ll [rows] = log p(x|prop) as eval_cond_ll returned it; prop [rows][nz] is replaced by the next
 * iteration's proposals eps_next * std + cur (eps_next NULL: left alone); keep = index of the kept sample this iteration
 * produces or -1.  init != 0 (vae.py:227-228): cond_ll was computed at cur -- cur_ll = log p(cur, x), accepts = 0, first proposals. */
int lv_mh_step_f32(const float* cond_ll, float* prop, float* cur, float* cur_ll, int* accepts, const float* u,
                   const float* eps_next, float std, float* samples, int rows, int C, int nz, int nsamples, int keep, int init,
                   float* ratio_out, int* accept_out, void* stream);

/* ---- annealed importance sampling of log p(x) (lv_ais.hip): VAE.nll_ais (Neal 2001; Wu et al. 2017).  The transitions are
 * the random-walk Metropolis kernel above on the annealed target q0(z)^(1 - beta) p(z, x)^beta; every chain carries a log-weight.
 *   q0      = N(mu0, diag exp(lv0)), mu0 / lv0 [B][nz]; both NULL: the prior N(0, I)
 *   g(z)    = (log p(z) - log q0(z)) + log p(x|z)           float32; with the prior as q0 the pair is skipped, g = log p(x|z)
 *   z_0     ~ q0,  logw = 0 (float64)
 *   for i = 1..N:
 *       logw += (beta_i - beta_{i-1}) * (double) g(cur)      float64 accumulate, beta a float64 array
 *       next  = eps_i * std_i + cur                          rounded product, then rounded sum
 *       ratio = [log q0(next) + (float)beta_i * g(next)] - [log q0(cur) + (float)beta_i * g(cur)]
 *       accept = ratio >= 0 || u_i < expf(ratio)             select, never blend; a NaN ratio rejects
 *   log p^(x) = logsumexp_c logw_c - log C
 * State in caller-owned buffers: cur [B][C][nz], g_cur / lq_cur [B][C] (g(cur), log q0(cur)), logw [B][C] float64, accepts
 * [B][C] int32.  ratio_out / accept_out / logw_out (float / int32 / float64, one per chain and iteration; logw_out: the running
 * log-weight after the iteration's increment) may be NULL.  eps and u are buffers of standard normal / uniform [0, 1) draws.
 * lv_ais_chain_f32: the fused route, envelope lv_ais_chain_f32_supported (that of lv_mh_chain_f32); ws is lv_mh_chain_prep_f32's
 * workspace, unchanged.  n_iter iterations in one launch: eps [n_iter][B][C][nz], u [n_iter][B][C], std_it [n_iter], beta
 * [n_iter + 1] = the temperature before this launch's first iteration, then one per iteration.  first != 0: score the starting
 * point in cur first (incoming g_cur / lq_cur / logw / accepts ignored; logw and the counts start at 0). */
int lv_ais_chain_f32_supported(int V, int ni, int H, int nz, int T);
int lv_ais_chain_f32(const int64_t* x, int B, int T, const float* ws, int V, int H, int nz, int C, float* cur, float* g_cur,
                     float* lq_cur, double* logw, int* accepts, const float* eps, const float* u, const double* beta,
                     const float* std_it, const float* mu0, const float* lv0, int n_iter, int first, float* ratio_out,
                     int* accept_out, double* logw_out, void* stream);
/* lv_ais_step_f32: the glue for any decoder, rows = B * C chains, any nz >= 1, one launch per iteration.  cond_ll [rows] =
 * log p(x|prop) as eval_cond_ll returned it; the launch decides iteration i at temperature beta (= beta_i), selects, counts and
 * writes ratio_out / accept_out [rows]; then, where eps_next is given, it applies iteration i + 1's increment
 * logw += dbeta_next * (double) g(cur) (dbeta_next = beta_{i+1} - beta_i, formed in float64 by the caller), writes it to
 * logw_out_next [rows] and replaces prop by eps_next * std_next + cur.  init != 0: cond_ll was computed at cur = z_0 -- g_cur,
 * lq_cur, logw = 0, accepts = 0, then iteration 1's increment and proposals as above (u, beta unread). */
int lv_ais_step_f32(const float* cond_ll, float* prop, float* cur, float* g_cur, float* lq_cur, double* logw, int* accepts,
                    const float* u, double beta, const float* eps_next, float std_next, double dbeta_next, const float* mu0,
                    const float* lv0, int rows, int C, int nz, int init, float* ratio_out, int* accept_out,
                    double* logw_out_next, void* stream);

/* ---- Hamiltonian transitions for the chains above (lv_hmc.hip): VAE.nll_ais(transition="hmc"),
 * VAE.sample_from_posterior(transition="hmc").  The contract, with the float32 evaluation order of every expression, is at the
 * top of lv_hmc.hip; q0, g, the accept rule, the float64 beta and logw are those of lv_ais.hip.  With rec(z) = -log p(x|z) and
 * d(z) = d rec / d z from one decoder forward + backward to z on all rows = B * C chains (row b * C + c):
 *   grad U_beta(z)_j = a_j + (float)beta * ((z_j - a_j) + d_j),  a_j = (z_j - mu0_j) * expf(-lv0_j)   (prior: z_j + beta * d_j)
 *   for i = 1..N:  logw += (beta_i - beta_{i-1}) * (double) g(cur);  p <- mom_i;  K0 = 0.5 |p|^2
 *                  p <- p - (eps / 2) grad U(cur)     (from the cached d(cur));   L times: z <- z + eps p, score z, kick (the
 *                  last kick a half one);  dH = [log q0(z) + beta_i g(z)] - [log q0(cur) + beta_i g(cur)] + K0 - 0.5 |p|^2
 *                  accept = dH >= 0 || u_i < expf(dH);  select;  eps <- min(max(eps * (accepted ? up : down), eps_min), eps_max)
 * lv_hmc_leap_f32 is one launch after every decoder pass.  rec [rows], dz [parts][rows][nz] (lv_dec_tail_dz_f32's partial
 * sums; parts = 1: a plain gradient).  In flight: pos [rows][nz] (the decoder's z input), mom [rows][nz], k0 [rows].  State: cur
 * [rows][nz], g_cur / lq_cur / rec_cur [rows], d_cur [rows][nz], logw [rows] float64, accepts [rows] int32, eps [rows].
 *   mode 0 (init): the pass scored z_0 = pos -- store the state, logw = 0, accepts = 0, then open transition 1;
 *   mode 1 (mid):  full kick at beta, drift, write mom / pos (needs L >= 2);
 *   mode 2 (last): half kick at beta, dH, the decision with u [rows], select, count, adapt, then open the next transition.
 * Opening (mom_next [rows][nz] given): logw += dbeta_next * (double) g(cur) -> logw_out_next, p <- mom_next, K0 -> k0, half kick
 * at beta_next from d_cur, drift -> pos.  mom_next NULL: no transition follows, only the state is written.  beta, beta_next and
 * dbeta_next = beta_next - beta are formed in float64 by the caller.  dh_out / flag_out [rows] (mode 2), logw_out_next [rows],
 * keep_out [rows][nz] (the selected cur; modes 0 and 2) may be NULL.  Nothing is written when an argument is refused. */
int lv_hmc_leap_f32(const float* rec, const float* dz, int parts, float* pos, float* mom, float* k0, float* cur, float* g_cur,
                    float* lq_cur, float* rec_cur, float* d_cur, double* logw, int* accepts, float* eps, const float* u,
                    const float* mom_next, double beta, double beta_next, double dbeta_next, const float* mu0, const float* lv0,
                    int rows, int C, int nz, int L, int mode, float up, float down, float eps_min, float eps_max, float* dh_out,
                    int* flag_out, double* logw_out_next, float* keep_out, void* stream);

/* ---- generation helpers (lv_eval.hip; SURVEY.md 8f row 4: modules/decoders/dec_lstm.py:163-367) -------------------------
 * torch.argmax(logits, dim=1) (greedy_decode, dec_lstm.py:304): lowest index among equal maxima */
int lv_argmax_rows_f32(const float* in, long ld, int R, int C, int64_t* idx, void* stream);
/* F.log_softmax(logits, -1) + the live hypotheses' running log-probabilities addrow[r] (beam_search_decode, dec_lstm.py:214-218) */
int lv_log_softmax_rows_f32(const float* in, long ld, int R, int C, const float* addrow, float* out, long ldo, void* stream);
/* categorical draw from softmax(logits[r]) by inverse CDF with the uniform u[r] (sample_decode's torch.multinomial,
 * dec_lstm.py:351-352).  With w[c] = exp(logits[r][c] - max_c logits[r]) and s = sum_c w[c]: idx[r] = the first column with
 * w[c] > 0 whose inclusive running sum reaches u[r]*s.  If rounding leaves the running sum short, idx[r] is the last column
 * with positive weight; C - 1 is returned only if no column has positive weight.  A column of probability zero is never drawn. */
int lv_sample_rows_f32(const float* in, long ld, int R, int C, const float* u, int64_t* idx, void* stream);
/* the same draw from a tempered, truncated distribution (no counterpart in the reference, whose sample_decode draws from the full
 * softmax, dec_lstm.py:351-352).  y = in * inv_temp (one f32 multiply); order: larger y first, lower column among equals; Kk = the
 * first min(top_k, C) columns (top_k == 0: all); w = exp(y - max y); K = the shortest prefix of Kk whose weight reaches
 * top_p * sum_Kk w (top_p == 1: Kk; never empty).  idx[r] = the first column of K, in COLUMN order, with w > 0 whose inclusive
 * running sum over K reaches u[r] * sum_K w; the last positive-weight column of K if rounding leaves the sum short; C - 1 only if
 * no column has positive weight.  Optional outputs (NULL: not written): lp = (x[idx] - max x) - log sum_all exp(x - max x), the
 * model's log-probability at temperature 1; lq = (y[idx] - max y) - log sum_K w, the log-probability under the distribution drawn
 * from; kept = |K|, tau = min y over K, ntie = columns of K equal to tau: K is {y > tau} plus the first ntie columns with y == tau.
 * Rows 16-byte aligned (LV_ERR_ALIGN); inv_temp finite and > 0, top_k >= 0, 0 < top_p <= 1 (LV_ERR_SHAPE).  The result is a
 * function of the inputs alone: repeated launches give the same bits. */
int lv_sample_filtered_rows_f32(const float* in, long ld, int R, int C, const float* u, float inv_temp, int top_k, float top_p,
                                int64_t* idx, float* lp, float* lq, int* kept, float* tau, int* ntie, void* stream);

/* ---- Omniglot path: ResNetEncoderV2 (modules/encoders/enc_resnet_v2.py:27-126) and PixelCNNDecoderV2
 * (modules/decoders/dec_pixelcnn_v2.py:12-195).  Activations NHWC ([N*H*W][C]); a convolution = lv_im2col_f32 +
 * lv_gemm_* against weights packed [Cout][taps][Cin]; 1x1 convolutions are plain GEMMs.  `ntaps` = length of the
 * raster-order tap PREFIX that is materialised / used: kh*kw for an ordinary conv, (kh/2)*kw + kw/2 + 1 for a type-B
 * masked conv (dec_pixelcnn_v2.py:17-20) -- the masked taps are skipped, not multiplied by zero. */
int lv_im2col_f32(const float* x, float* col, long ldcol, int N, int H, int W, int C, int Ho, int Wo,
                  int kh, int kw, int pad, int stride, int ntaps, void* stream);
int lv_col2im_f32(const float* dcol, long ldcol, float* dx, int N, int H, int W, int C, int Ho, int Wo,
                  int kh, int kw, int pad, int stride, int ntaps, int accumulate, void* stream);
int lv_conv_pack_w_f32(const float* w /*[Cout][Cin][KK]*/, float* wg /*[Cout][KK][Cin]*/, int Cout, int Cin, int KK, void* stream);
int lv_conv_unpack_dw_f32(const float* dwg, float* dw, int Cout, int Cin, int KK, int accumulate, void* stream);
int lv_mul_inplace_f32(float* w, const float* m, long n, void* stream);   /* MaskedConv2d.forward: weight.data.mul_(mask) */
/* Direct (implicit-GEMM) 32 -> 32 convolutions on 28 x 28 maps: the masked k x k convolutions of PixelCNNBlock
 * (dec_pixelcnn_v2.py:12-62), no im2col buffer; masked taps are skipped in forward / data gradient (the type-B taps are a raster
 * prefix), the weight gradient covers all k*k taps (lv_conv_direct.hip).  in / out NHWC [N][28][28][32]; k odd <= 7. */
long lv_conv32_wpack_floats(int ntaps);
int lv_conv32_pack_f32(const float* w /*[32][32][k*k]*/, float* wp, int k, int ntaps, int transpose, void* stream);
int lv_conv32_f32(const float* in, const float* wp, float* out, int N, int k, int ntaps, int mirror, int accumulate, void* stream);
int lv_conv32_wgrad_slabs(int N, int k);
long lv_conv32_wgrad_ws_floats(int N, int k);
int lv_conv32_wgrad_f32(const float* x, const float* dy, float* dw /*[32][32][k*k]*/, float* ws, int N, int k, int accumulate,
                        void* stream);
/* Pointwise (1 x 1) convolutions between 32 / 64 channels (PixelCNNBlock's bottleneck and expansion convolutions,
 * dec_pixelcnn_v2.py:41-43,49-51): out [P][Cout] (=|+=) in [P][Cin] . W^T, W [Cout][Cin]; w_transposed = 1: W given as
 * [Cin][Cout] (the data gradient of the convolution that owns it); the weight gradient sums dy^T x over all P pixels. */
int lv_conv1x1_f32(const float* in, const float* w, float* out, long P, int Cin, int Cout, int w_transposed, int accumulate,
                   void* stream);
long lv_conv1x1_wgrad_ws_floats(int Cin, int Cout);
/* Split-bf16 forms of lv_conv32_f32 / lv_conv32_bnstat_f32 (round 4): every operand as hi + lo with hi = bf16(x), lo = bf16(x - hi),
 * products on the bf16 matrix pipe with f32 accumulation.  terms = 3: hi*hi' + hi*lo' + lo*hi' (results agree with the exact-f32 form
 * to ~1e-5 relative per product term before summation); terms = 1: plain bf16 operands.  wp16: lv_conv32_pack_b16's image (a buffer of
 * lv_conv32_wpack_floats(ntaps) floats).  bn_partial: NULL, or the BatchNorm stage-1 partials as lv_conv32_bnstat_f32 (forward only). */
int lv_conv32_pack_b16(const float* w, void* wp16, int k, int ntaps, int transpose, void* stream);
int lv_conv32_b16(const float* in, const void* wp16, float* out, float* bn_partial, int N, int k, int ntaps, int mirror, int accumulate,
                  int terms, void* stream);
/* Stage 1 of a BatchNorm BACKWARD in the epilogue of the data-gradient convolution that produces its incoming gradient (round 4;
 * dec_pixelcnn_v2.py:44-62: conv -> BatchNorm -> ELU chains, backward): the data gradient g = dL/d(BN output) leaves the kernel as
 * dv = g * ELU'(y) and every workgroup writes the per-channel (sum dv, sum dv * xhat), xhat = (x - mean) * invstd, of what it stored to
 * partial [blocks][2][C] (blocks = lv_conv32_blocks(N) / lv_conv1x1_blocks(P)); lv_bn_bwd_apply_partials_f32 then finishes the
 * BatchNorm (dx, dgamma, dbeta) with no reduction launch.  y = the BatchNorm's saved output, x = its input.  lv_conv32_bnbwd: terms = 0
 * (exact f32, wp from lv_conv32_pack_f32(transpose = 1)), 1 / 3 (split-bf16, lv_conv32_pack_b16). */
int lv_conv32_bnbwd(const float* in, const void* wp, float* dv, float* partial, int N, int k, int ntaps, const float* y, const float* x,
                    const float* mean, const float* invstd, int act_elu, int terms, void* stream);
int lv_conv1x1_bnbwd_f32(const float* in, const float* w, float* dv, float* partial, long P, int Cin, int Cout, const float* y,
                         const float* x, const float* mean, const float* invstd, int act_elu, void* stream);
int lv_bn_bwd_apply_partials_f32(const float* x, const float* dv, const float* partial, int nblk, const float* mean, const float* invstd,
                                 const float* gamma, float* dx, float* dgamma, float* dbeta, int accumulate_param_grads, long P, int C,
                                 void* stream);
/* ... and of lv_conv32_wgrad_f32 (same scratch and partial layout: lv_wgrad_reduce_batched serves both). */
int lv_conv32_wgrad_b16(const float* x, const float* dy, float* dw, float* ws, int N, int k, int accumulate, int terms, void* stream);
/* All weight-gradient reductions of a backward pass in one launch: lv_conv32_wgrad_f32 / lv_conv1x1_wgrad_f32 called with
 * dw = NULL leave their partial blocks in ws (lv_conv32_wgrad_parts / lv_conv1x1_wgrad_parts of them), and
 * lv_wgrad_reduce_batched sums every layer's partials into its gradient.  desc (HOST memory): 4 int64 per layer =
 * {ws pointer, dw pointer, outputs | parts << 32, k*k (32 -> 32 convolution) or 0 (pointwise)}. */
int lv_conv32_wgrad_parts(int N, int k);
int lv_conv1x1_wgrad_parts(long P);
int lv_wgrad_reduce_batched(const long long* desc, int ndesc, void* stream);
/* PixelCNN ancestral sampling one pixel at a time (dec_pixelcnn_v2.py:201-232; lv_pixelcnn_sample.hip): every layer of
 * PixelCNNDecoderV2.forward at ONE position (i, j) for all B images, from the cached input maps of the masked convolutions at the
 * earlier positions -- bit-equal to the eval-mode full forward (same fma chains in the same order as lv_gemm_f32 /
 * lv_conv1x1_f32 / lv_conv32_f32 / lv_bn_eval_f32).  net: HOST array of lv_pixelcnn_net_words() 64-bit words (device pointers,
 * int64 / double fields of the network table; the per-block tables of lv_pixelcnn_block_words() words each live in device
 * memory); image_engine.PixelCNNSampler builds both.  lv_conv32_tap_split(N): the summation form lv_conv32_f32 uses at batch N. */
int lv_pixelcnn_net_words(void);
int lv_pixelcnn_block_words(void);
int lv_pixelcnn_pixel_step_f32(const long long* net, int B, int i, int j, void* stream);
int lv_conv32_tap_split(int N);
/* Forward convolutions that also leave the stage-1 partials (per-workgroup per-channel sum and sum of squares of their
 * outputs, [blocks][2][Cout]) of the nn.BatchNorm2d that follows them in PixelCNNBlock (dec_pixelcnn_v2.py:41-52), consumed
 * by lv_bn_fwd_partials_f32: the normalisation's statistics pass over the activation is saved. */
int lv_conv32_blocks(int N);
int lv_conv32_bnstat_f32(const float* in, const float* wp, float* out, float* bn_partial, int N, int k, int ntaps, void* stream);
long lv_conv1x1_blocks(long P);
int lv_conv1x1_bnstat_f32(const float* in, const float* w, float* out, float* bn_partial, long P, int Cin, int Cout, void* stream);
int lv_bn_fwd_partials_f32(const float* x, const float* gamma, const float* beta, const float* res, int act_elu, float* y,
                           float* mean, float* invstd, float* run_mean, float* run_var, float eps, float momentum,
                           const float* partial, int nblk, long P, int C, void* stream);
int lv_conv1x1_wgrad_f32(const float* x, const float* dy, float* dw, float* ws, long P, int Cin, int Cout, int accumulate,
                         void* stream);
/* nn.BatchNorm2d in train mode (batch statistics, running stats momentum update with unbiased variance) fused with the
 * residual add and nn.ELU that follow it in ResNetBlock / PixelCNNBlock; backward with ELU' from the saved output */
int lv_bn_workspace_floats(int C);
/* the same module in eval mode (running statistics; image.py:96-187 evaluation passes, dec_pixelcnn_v2.py:201-232 sampling):
 * y = act((x - run_mean) / sqrt(run_var + eps) * gamma + beta (+ res)); mean_out / invstd_out (may be NULL) = what was applied */
int lv_bn_eval_f32(const float* x, const float* gamma, const float* beta, const float* run_mean, const float* run_var, float eps,
                   const float* res, int act_elu, float* y, float* mean_out, float* invstd_out, long P, int C, void* stream);
/* backward of lv_bn_eval_f32 (the statistics are constants: no batch-sum term): g = dy (+ dy2 + dy3 + dy4, NULL or given in order),
 * dv = g * elu'(y) (also the residual input's gradient), dx = dv * gamma * invstd, dbeta = sum_p dv, dgamma = sum_p dv * xhat
 * (= or +=); mean / invstd as lv_bn_eval_f32 wrote them */
int lv_bn_eval_bwd_f32(const float* x, const float* dy, const float* dy2, const float* dy3, const float* dy4, const float* y,
                       const float* mean, const float* invstd, const float* gamma, int act_elu, float* dv, float* dx,
                       float* dgamma, float* dbeta, int accumulate_param_grads, long P, int C, void* stream);
int lv_bn_fwd_f32(const float* x, const float* gamma, const float* beta, const float* res, int act_elu,
                  float* y, float* mean, float* invstd, float* run_mean, float* run_var,
                  float eps, float momentum, float* ws, long P, int C, void* stream);
int lv_bn_bwd_f32(const float* x, const float* dy, const float* y, const float* mean, const float* invstd,
                  const float* gamma, int act_elu, float* dv, float* dx, float* dgamma, float* dbeta,
                  int accumulate_param_grads, float* ws /* lv_bn_workspace_floats(C) + 2C */, long P, int C, void* stream);
/* The same backward with the incoming gradient given as TWO summands, dy + dy2 (dy2 may be NULL): an activation with two
 * consumers (every residual-block output of dec_pixelcnn_v2.py:33-62) receives two gradient tensors, and adding them while the
 * reduction pass reads them saves the separate accumulation launch (3 passes over the tensor) for one more read. */
int lv_bn_bwd2_f32(const float* x, const float* dy, const float* dy2, const float* y, const float* mean, const float* invstd,
                   const float* gamma, int act_elu, float* dv, float* dx, float* dgamma, float* dbeta,
                   int accumulate_param_grads, float* ws, long P, int C, void* stream);
/* ... and as up to FOUR summands dy + dy2 + dy3 + dy4 (given in order, the unused ones NULL; added left to right): the outputs of
 * the PixelCNN's main blocks feed a residual add, a direct connection and the next block (dec_pixelcnn_v2.py:88-110). */
int lv_bn_bwd4_f32(const float* x, const float* dy, const float* dy2, const float* dy3, const float* dy4, const float* y,
                   const float* mean, const float* invstd, const float* gamma, int act_elu, float* dv, float* dx, float* dgamma,
                   float* dbeta, int accumulate_param_grads, float* ws, long P, int C, void* stream);
/* nn.Sigmoid + the BCE of PixelCNNDecoderV2.reconstruct_error (dec_pixelcnn_v2.py:190-195, eps = 1e-12) */
int lv_sigmoid_bce_fwd_f32(const float* logit, const float* x, float* rec, int B, int npix, float eps, void* stream);
int lv_sigmoid_bce_bwd_f32(const float* logit, const float* x, const float* drec, float* dlogit, int B, int npix,
                           float eps, void* stream);
/* torch.cat([img, z_transform(z).view(B, fm, 28, 28)], dim) as one NHWC tensor (dec_pixelcnn_v2.py:178-186) */
int lv_dec_input_fwd_f32(const float* x, const float* zt, float* in5, int B, int npix, int fm, void* stream);
int lv_dec_input_bwd_f32(const float* din5, float* dzt, int B, int npix, int fm, void* stream);
/* Multi-sample training (image.py --nsamples; VAE.loss(x, kl_weight, nsamples = ns), dec_pixelcnn_v2.py:178-190): the decoder runs on
 * Bd = B * ns images in row order bd = b * ns + s, and decoder row bd takes its image channel and its BCE target from image bd / ns of
 * x [B][npix] -- no expanded copy of x.  logit [Bd * npix], rec / drec [Bd], zt [Bd][fm * npix], in5 [Bd * npix][1 + fm].  The results
 * have the bits of the entries above run on x.repeat_interleave(ns) (ns = 1: their bits).  The input layer's backward is
 * lv_dec_input_bwd_f32 with B := Bd. */
int lv_sigmoid_bce_ns_fwd_f32(const float* logit, const float* x, float* rec, int B, int ns, int npix, float eps, void* stream);
int lv_sigmoid_bce_ns_bwd_f32(const float* logit, const float* x, const float* drec, float* dlogit, int B, int ns, int npix, float eps,
                              void* stream);
int lv_dec_input_ns_fwd_f32(const float* x, const float* zt, float* in5, int B, int ns, int npix, int fm, void* stream);
/* BatchNorm from the producing convolution's stage-1 partial rows at ANY row count (lv_bn_fwd_partials_f32 and
 * lv_bn_bwd_apply_partials_f32 re-read all rows in every workgroup and stop at 1024 of them): the rows [nblk][2][C] -- a buffer of
 * lv_bn_partial_floats(nblk, C) floats -- are reduced once, in f64 and a fixed order, by a launch of their own, and the apply pass
 * reads the finished 2 * C floats.  Forward: lv_bn_finish_fwd_f32 (mean, invstd, running statistics with momentum and the unbiased
 * variance; run_mean / run_var both NULL or both given), then lv_bn_fwd_stats_f32.  Backward: lv_bn_finish_bwd_f32 (sums [2][C] =
 * this layer's (sum dv, sum dv * xhat); dbeta / dgamma = or +=), then lv_bn_bwd_stats_f32.  C: a power of two in [16, 256]. */
long lv_bn_partial_floats(long nblk, int C);
int lv_bn_finish_fwd_f32(const float* partial, int nblk, long P, int C, float eps, float momentum, float* mean, float* invstd,
                         float* run_mean, float* run_var, void* stream);
int lv_bn_fwd_stats_f32(const float* x, const float* gamma, const float* beta, const float* res, int act_elu, float* y,
                        const float* mean, const float* invstd, long P, int C, void* stream);
int lv_bn_finish_bwd_f32(const float* partial, int nblk, int C, float* sums, float* dgamma, float* dbeta, int accumulate_param_grads,
                         void* stream);
int lv_bn_bwd_stats_f32(const float* x, const float* dv, const float* sums, const float* mean, const float* invstd, const float* gamma,
                        float* dx, long P, int C, void* stream);

/* Batched, device-resident beam search for the LSTM decoder (lv_beam.hip; dec_lstm.py:163-268 for B sentences at once).  State
 * lives in caller-owned buffers laid out [B][K] (K slots per sentence): tok int64, score f32 (-inf = dead slot), h / c as two
 * [B][K][H] halves (the cell reads one and writes the other; lv_beam_advance_f32 gathers back), meta int32 [B][4] = {n_done, active,
 * steps taken, reserved}, the completed list done_score f32 [B][K] / done_ref int32 [B][K][2] = (step, rank) in completion order,
 * trace int32 [Tmax][B][K][3] = (parent slot, word, destination slot or -1) in rank order, margin f32 [B] (smallest gap between the
 * last accepted and the first rejected candidate so far) and counter int32 [1] (sentences still active).  Candidates are ordered by
 * score descending, then flat index slot * V + word ascending.  Envelope: K <= 16, K * V < 2^31, B * K <= 8192
 * (lv_beam_supported; LV_ERR_UNSUPPORTED outside).  An inactive sentence is left untouched by select and advance. */
int lv_beam_supported(int B, int K, int V);
long lv_beam_ws_floats(int B, int K, int V);
int lv_beam_init_f32(const float* h0, const float* c0, float* h, float* c, int64_t* tok, float* score, int* meta,
                     float* done_score, float* margin, int* counter, int B, int K, int H, int V, int start_tok, void* stream);
/* logits [B * K][ld] -> pick_score / pick_flat [B][K + 1]: the best K - n_done candidates (logit - lse) + score[slot] in rank order,
 * then the runner-up; flat = -1 where there is none.  part: lv_beam_ws_floats(B, K, V) floats. */
int lv_beam_select_f32(const float* logits, long ld, const float* score, const int* meta, float* part, float* pick_score,
                       int* pick_flat, float* margin, int B, int K, int V, void* stream);
/* step t (0-based, < Tmax) of dec_lstm.py:232-246 from those picks; (h_src, c_src) -> (h_dst, c_dst) must be different halves */
int lv_beam_advance_f32(const float* pick_score, const int* pick_flat, const float* h_src, const float* c_src, float* h_dst,
                        float* c_dst, int64_t* tok, float* score, int* meta, float* done_score, int* done_ref, int* trace,
                        int* counter, int t, int Tmax, int B, int K, int H, int V, int end_tok, void* stream);
/* winner = first maximum over completed (completion order) then live slots (slot order): ids int64 [B][Tmax + 1] (<s> in front),
 * len int32 [B], win_score f32 [B] */
int lv_beam_backtrace(const float* score, const int* meta, const float* done_score, const int* done_ref, const int* trace,
                      int64_t* ids, int* len, float* win_score, int B, int K, int Tmax, int start_tok, void* stream);

/* Device-resident greedy / sample decoding for the LSTM decoder (lv_rollout.hip; dec_lstm.py:270-367 for n sentences at once).
 * State of n rows in caller-owned buffers: tok int64 [n] (next input word), alive int32 [n], ids int64 [n][Tmax] (emitted words),
 * len int32 [n], score f32 [n] (running log-probability), margin f32 [n] (greedy: smallest top-1 minus top-2 logit gap so far),
 * counter int32 [1] (rows still alive), h / c as two [n][H] halves (the cell reads one and writes the other).
 * init: tok = start_tok, alive = 1, len = 0, score = 0, margin = +inf, counter = n, (h0, c0) copied into (h, c). */
int lv_rollout_init_f32(const float* h0, const float* c0, float* h, float* c, int64_t* tok, int* alive, int* len, float* score,
                        float* margin, int* counter, int n, int H, int V, int start_tok, void* stream);
/* step t (0-based, < Tmax) in one launch.  The pick from logits [n][ld]: u == NULL -> argmax, bit-equal to lv_argmax_rows_f32 (rows
 * 16-byte aligned, LV_ERR_ALIGN otherwise); else the inverse-CDF draw with u [n], bit-equal to lv_sample_rows_f32 (margin may then
 * be NULL).  A live row: ids[r][t] = tok[r] = pick, len += 1, score += (x[pick] - M) - log S, margin = min(margin, top1 - top2)
 * (greedy), alive = (pick != end_tok), counter drops by one per row that ended.  A dead row keeps ids / len / score / margin / tok.
 * Every row's state moves (h_src, c_src) -> (h_dst, c_dst) (different halves).  counter == 0 on entry: nothing is changed. */
int lv_rollout_pick_f32(const float* logits, long ld, const float* u, const float* h_src, const float* c_src, float* h_dst,
                        float* c_dst, int64_t* tok, int* alive, int64_t* ids, int* len, float* score, float* margin,
                        int* counter, int t, int Tmax, int n, int H, int V, int end_tok, void* stream);
/* the same step with the draw of lv_sample_filtered_rows_f32, bit-equal to it (u [n] mandatory, rows 16-byte aligned): score +=
 * lp, qscore f32 [n] += lq for a live row; the bookkeeping, the counter gate and the dead-row rules of lv_rollout_pick_f32 (a dead
 * row keeps qscore as well).  There is no margin. */
int lv_rollout_pick_filtered_f32(const float* logits, long ld, const float* u, float inv_temp, int top_k, float top_p,
                                 const float* h_src, const float* c_src, float* h_dst, float* c_dst, int64_t* tok, int* alive,
                                 int64_t* ids, int* len, float* score, float* qscore, int* counter, int t, int Tmax, int n, int H,
                                 int V, int end_tok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LVAE_H */
