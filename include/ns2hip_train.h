/* libns2hip: the training pass -- the backward of the denoiser, of the conditioning encoders, of the DurationPitchPredictor and of the
 * Aligner, and the RVQ cross-entropy term.  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  The
 * conventions, the status codes, ns2_linear_args, ns2_attn_args and the definition of a ragged batch with its computed extent are those
 * of ns2hip.h, which this header includes.
 *
 * Ragged batches in training: output rows and gradient rows at or beyond a length are exact zeros, so what follows them in the pass (the
 * weight-gradient GEMMs, the bias and FiLM sums) needs no lengths. */
#ifndef NS2HIP_TRAIN_H
#define NS2HIP_TRAIN_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ training: the backward pass
 * What `loss.backward()` runs for the denoiser (NS2:1635 `pred = self.model(...)` under autograd, NS2:1637-1666 the loss,
 * NS2:1886 `accelerator.backward`).  Two training arithmetics, selected per call by `precision`:
 *   3 = bf16 hi / lo planes, three bf16 MFMA products per contraction (the fp32 exponent range: no loss scaling);
 *   4 = "mixed": FMT_H8 lines, one IEEE-half product + both correction terms on the fp8 MFMA (2 MFMA units instead of 3).  IEEE half
 *       stops at 65504 and loses precision below 6e-5, so the caller scales the loss (a power of two; every gradient is linear in
 *       it) -- the reference trains under accelerate's fp16 mixed precision the same way (NS2:1710-1711, 1723-1726).  Values that
 *       leave the half range are counted (ns2_saturation_count, ns2_saturation_peek): an overflowed step is detected, not silently clamped.
 *       The attention products stay bf16 x3 at both precisions (q / k / v / dO planes are bf16 hi / lo: ns2_linear with out_precision = 3).
 * The contractions reuse the forward GEMM family:
 *   dgrad  dX = dY W   : ns2_linear (fp32 output) on a SECOND pack of the weight -- ns2_weight_pack of W^T ([in, out, taps] with the taps
 *                        flipped), conv_taps as in the forward, pad_left = 0 (the gradient of a causal conv looks ahead);
 *   wgrad  dW = dY^T X : ns2_wgrad on TRANSPOSED planes (contraction over the tokens), split over fixed slots + fixed-order sum.
 * Every reduction of this section is slot based and summed in a fixed order: gradients are deterministic, no atomics. */

/* re-pack a weight IN PLACE from new fp32 values (same shape / flags as the ns2_weight_pack call that made it): stream-ordered,
 * no allocation, no synchronisation -- the per-step refresh of an optimizer's weights */
int ns2_weight_update(ns2_weight* w, const float* w_src, const float* extra1x1, void* stream);

/* Every pack of a training pass in ONE launch.  A part = a rectangle of a packed weight (rows [row0, row0 + rows), columns per tap
 * [col0, col0 + cols) of a plain ns2_weight_pack weight: no GEGLU permutation, no extra 1x1 block) and where its fp32 values live:
 * element (r, c, tap) at src[r * sr + c * sc + tap * st], strides in elements and possibly negative -- the parameter's own storage
 * serves the forward pack (sr = C T, sc = T, st = 1), the dgrad pack W^T (sr = T, sc = C T) with flipped taps (st = -1 from src + T - 1)
 * and q | kv concatenations (two parts) without any copy.  ns2_weights_repack_build writes the device table (caller-owned memory of
 * ns2_weights_repack_table_bytes(n) bytes; synchronises once), ns2_weights_repack replays it: stream-ordered, no allocation. */
typedef struct {
  ns2_weight* w; const float* src;
  int64_t sr, sc, st;
  int row0, rows, col0, cols;
} ns2_repack_part;
int64_t ns2_weights_repack_table_bytes(int n);
int ns2_weights_repack_build(const ns2_repack_part* parts, int n, void* table_device, int64_t table_bytes, int64_t* total_blocks, void* stream);
int ns2_weights_repack(const void* table_device, int n, int64_t total_blocks, void* stream);
/* after ns2_weights_repack: rebuild the tiled images (ns2_weight_tile_conv3 / _linear / _wavenet) of those weights that have them --
 * one small launch per such weight, stream-ordered, no allocation.  With it packs that carry images may be part of a repack table. */
int ns2_weights_retile(ns2_weight* const* weights, int n, void* stream);

/* fp32 gradient x [M, C] (row stride ldx) -> any of
 *   row planes [M, ld_row] (zero beyond C)                                  -- the A operand of the dgrad GEMM;
 *   transposed planes T[c][m] with ld_t token columns (ld_t a multiple of 32, zero beyond M) and t_rows rows (zero beyond C; a
 *     W operand of ns2_wgrad needs its rows padded to a multiple of 256)    -- the operands of ns2_wgrad;
 *     per_batch != 0: T[b * t_rows + c][n] per utterance of seq_len tokens   -- the transposed operands of ns2_attention_bwd;
 *     shift: T[c][m] = x[m - shift][c] if m - shift lies in the utterance of m (seq_len tokens each), else 0;
 *   colsum_partial [ns2_grad_prep_slices(M, ld_t)][C]: column sums of 64-row tiles (sum the slots with ns2_reduce_slices:
 *     the bias gradient). */
int64_t ns2_grad_prep_slices(int M, int64_t ld_t);
int ns2_grad_prep(const float* x, int64_t ldx, int M, int C, int seq_len, int shift, uint16_t* row_hi, uint16_t* row_lo, int ld_row,
                  uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, float* colsum_partial, int precision, void* stream);
/* the same transposition for an activation that already exists as operand planes (columns [in_col0, in_col0 + C) of [M, ld_in]):
 * tap t of a causal conv (NS2:583-595) contributes x[n - (k - 1 - t) * dilation], i.e. shift = (k - 1 - t) * dilation */
int ns2_planes_transpose(const uint16_t* in_hi, const uint16_t* in_lo, int ld_in, int in_col0, int M, int C, int seq_len, int shift,
                         uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, int precision, void* stream);
/* out[o * inner + j] (+)= sum_s partial[(o * S + s) * inner + j], s in increasing order */
int ns2_reduce_slices(const float* partial, int64_t outer, int S, int64_t inner, float* out, int accumulate, void* stream);
/* weight gradient of nn.Linear / CausalConv1d (NS2:583-595, 1021-1024, 1051-1069): dw[r, k, t] = sum_m dY[m, r] * X_t[m, k].
 * dyt: transposed planes of dY, R rows; xt: transposed planes of the T (shifted) inputs stacked along the rows, tap t at rows
 * [t * Kp, t * Kp + K), allocated (zeros) up to the next multiple of 256 rows; both with ld_t token columns.  dw [R, K, T] fp32
 * (the nn.Conv1d layout; T = 1: nn.Linear).  workspace = ns2_wgrad_workspace_bytes(R, T * Kp, ld_t) bytes of caller scratch. */
int64_t ns2_wgrad_workspace_bytes(int R, int ncols, int64_t ld_t);
int ns2_wgrad(const uint16_t* dyt_hi, const uint16_t* dyt_lo, const uint16_t* xt_hi, const uint16_t* xt_lo, int64_t ld_t, int R, int T,
              int Kp, int K, float* dw, void* workspace, int64_t workspace_bytes, int precision, void* stream);

/* The same gradient from the TOKEN-MAJOR operand planes themselves: dy [M, ld_dy] (the row planes ns2_grad_prep writes for the dgrad
 * GEMM), x [M, ld_x] (the operand planes the forward GEMM read).  Tap t of a causal conv's gradient reads x[m - (T - 1 - t) * dil]
 * inside the utterance of m (seq_len tokens, >= 32, M a multiple of it); T = 1: nn.Linear (dil / seq_len ignored).  The kernel forms
 * its MFMA fragments with gfx950's LDS transpose reads, so neither transposed nor shifted copies of the operands exist in memory.
 * Any shape is computed; ns2_wgrad_rows_preferred says whether this route is the faster one (the 256 x 256 kernel must fill the chip:
 * the dim = 128 model's narrow gradients stay on ns2_wgrad, which picks the 128 x 128 kernel).  workspace = ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32)). */
int ns2_wgrad_rows_preferred(int R, int ncols, int64_t M);
int ns2_wgrad_rows(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x, int64_t M,
                   int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes, int precision,
                   void* stream);
/* ns2_wgrad_rows on a ragged batch of M / seq_len utterances: a 32-token K tile whose tokens are all hidden is
 * neither fetched nor multiplied.  With seq_len % 256 == 0 a tile is hidden iff its first token is, and the causal taps of a visible
 * tile (token m - shift) read visible rows only.  The slice plan, the slots and the order of their sum are those of ns2_wgrad_rows
 * for the same M: a slot's sum only loses terms, and where the hidden rows of dY are zeros (the cotangent of a ragged pass) those
 * terms were exact zeros, so dW has the bits of ns2_wgrad_rows.  The hidden rows of dY and X may hold anything: they are not read.
 * Unlike ns2_wgrad_rows, seq_len is required for T = 1 too (it is the utterance stride of the lengths).  Refused (NS2_ERR_ARG, before
 * any device call) when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0; whatever ns2_wgrad_rows refuses is
 * refused alike.  Workspace: ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32)), as there. */
int ns2_wgrad_rows_lens(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x,
                        int64_t M, int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes,
                        int precision, const int* row_lens, void* stream);

/* WavenetResBlock's FiLM + gate (NS2:629-636) for the unfused training forward: out = tanh(z) * sigmoid(z), z = h * gamma_b + beta_b,
 * film[b] = [gamma (d) | beta (d)]; and its backward: dh = dg g'(z) gamma, partial[(b * slices + s)] = [sum dg g'(z) h | sum dg g'(z)]
 * over the s-th group of tokens of utterance b (ns2_film_gate_slices(seq_len) groups; ns2_reduce_slices gives d film [B, 2 d]) */
int ns2_film_gate_fwd(const float* h, int64_t ldh, const float* film, int film_ld, int seq_len, int64_t M, int d, float* out, int64_t ldo,
                      void* stream);
int ns2_film_gate_slices(int seq_len);
int ns2_film_gate_bwd(const float* dg, int64_t lddg, const float* h, int64_t ldh, const float* film, int film_ld, int B, int seq_len, int d,
                      float* dh, int64_t lddh, float* partial, void* stream);
/* GEGLU (NS2:1004-1007) on the saved pre-activation pre [M, ldp] = [x (f) | gate (f)]: planes of gelu(gate) * x, and the backward */
int ns2_geglu_fwd(const float* pre, int64_t ldp, int64_t M, int f, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
int ns2_geglu_bwd(const float* dh, int64_t lddh, const float* pre, int64_t ldp, int64_t M, int f, float* dpre, int64_t lddp, void* stream);
/* RMSNorm backward (NS2:727-746): dx = (dx_add ? dx_add : 0) + dL/dx (dx may alias dx_add: the residual stream's gradient);
 * cond_partial [B * slices][2 d] -> the adaptive (gamma_c, beta_c) gradients, gamma_partial [B * slices][d] -> the learned gamma's.
 * d: a multiple of 4, at most 2048; the leading dimensions multiples of 4.  A workgroup keeps 12 d floats in dynamic LDS: beyond
 * d = 1365 that is more than 64 KiB (96 KiB at d = 2048), and the launcher raises the kernel's dynamic-LDS limit before it launches. */
int ns2_rmsnorm_bwd_slices(int seq_len);
int ns2_rmsnorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, const float* cond, int cond_ld, int B,
                    int seq_len, int d, const float* dx_add, float* dx, int64_t lddx, float* cond_partial, float* gamma_partial, void* stream);

/* The training forward is ns2_attention_fwd with `lse` set.
 * delta[b, h, q] = sum_d dO[q, 64 h + d] * O[q, 64 h + d] (O from its operand planes, o_precision 3 or 4) */
int ns2_attention_delta(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H, int Nq,
                        float* delta, int o_precision, void* stream);
/* flash-attention backward, head dim 64: dq = scale * dS k, dk = scale * dS^T q, dv = P^T dO with P recomputed from lse and
 * dS = P (dO v^T - delta).  q / k / v / d_out: row-major planes (head h at columns col0 + 64 h) -- the kernels form K^T, Q^T and
 * dO^T themselves (LDS transpose reads of the row-major tiles).  dq == NULL or dk == dv == NULL skips that half (cross-attention to a
 * context that needs no gradient). */
typedef struct {
  const uint16_t* q_hi; const uint16_t* q_lo; int ldq, q_col0;
  const uint16_t* k_hi; const uint16_t* k_lo; int ldk, k_col0;
  const uint16_t* v_hi; const uint16_t* v_lo; int ldv, v_col0;
  const uint16_t* do_hi; const uint16_t* do_lo; int lddo;
  const float* lse; const float* delta;
  float* dq; int lddq, dq_col0;
  float* dk; int lddk, dk_col0;
  float* dv; int lddv, dv_col0;
  int B, H, Nq, Nk; float scale;
  /* gp_q / gp_kv != 0 -- that half of the gradients leaves the kernel as OPERAND PLANES instead of fp32 (the q | k | v projection's
   * dgrad and wgrad GEMMs are their only consumers): planes [rows, gp_ld] of precision gp_precision (3: bf16 hi / lo lines, 4: FMT_H8),
   * dq at columns dq_col0 + 64 h of row b Nq + q, dk / dv at dk_col0 / dv_col0 + 64 h of row b Nk + k (column offsets multiples of 32) */
  uint16_t* gp_hi; uint16_t* gp_lo; int gp_ld, gp_precision, gp_q, gp_kv;
  /* the mask and the dropout of the forward this is the backward of, as in ns2_attn_args (all zero: neither) */
  const uint8_t* key_mask; float dropout_p; const uint32_t* dropout_seed; unsigned dropout_call;
} ns2_attn_bwd_args;
int ns2_attention_bwd(const ns2_attn_bwd_args* args, void* stream);

/* ---- the denoiser's self-attention on a ragged batch, forward and backward.  Self-attention only (Nq == Nk = N, the stride of every
 * address); whole 64-row tiles beyond a length are neither fetched nor multiplied. */
/* ns2_attention_fwd as the training forward (args->lse wanted, precision 3, head_dim 64) of a ragged batch.  Utterance b attends to
 * keys [0, lens[b]) as in ns2_attention_fwd_lens; rows q < lens[b] of o and lse are bit for bit those of ns2_attention_fwd on the
 * utterance alone at Nq = Nk = lens[b].  Rows q >= lens[b]: o is all-zero bits in its format (bf16 hi / lo lines, or FMT_H8 lines with
 * o_precision 4) and lse is +inf, the statistic under which the backward kernels give such a query P = 0.
 * Refused (NS2_ERR_ARG, before any device call) when args or lens is null, args->lse is missing, Nq != Nk, or args->key_mask or
 * args->dropout_p is set.  ns2_attention_fwd_lens stays the inference call and keeps refusing lse. */
int ns2_attention_train_fwd_lens(const ns2_attn_args* args, const int* lens, void* stream);

/* ns2_attention_bwd of that forward.  Rows < lens[b] of dq, dk and dv (fp32, or the operand planes gp_*, both formats) are bit for bit
 * those of ns2_attention_bwd on the utterance alone at Nq = Nk = lens[b]; rows >= lens[b] are all-zero bits.  What q, k, v, dO, lse and
 * delta hold at or beyond a length is not read into any result.  Refused like the forward: args or lens null, lse missing, Nq != Nk,
 * key_mask or dropout_p set. */
int ns2_attention_bwd_lens(const ns2_attn_bwd_args* args, const int* lens, void* stream);

/* ---- head dims 32 and 128: the attention forward with its log-sum-exp, the delta reduction and the flash backward for heads of 32, 64
 * or 128 columns.  The entries above keep their head dim of 64 (ns2_attention_fwd refuses lse at any other).  These take the head
 * dim as an argument: head h lies at columns col0 + head_dim * h of every operand, output and gradient, and `scale` is the
 * caller's (head_dim ** -0.5 for the reference's attention).  With head_dim 64 (or 0) each launches the very kernels of its counterpart:
 * the same bits.  The arithmetic is that of head dim 64 throughout: precision 3 operands (bf16 hi / lo lines, hi*hi + hi*lo + lo*hi), a
 * fixed summation order, no atomics; o and the gradient planes leave in bf16 hi / lo lines or FMT_H8 lines (o_precision / gp_precision).
 * Every refusal of the three is NS2_ERR_ARG and is made before any device call. */
/* the training forward (args->lse required, precision 3) at args->head_dim 32, 64 or 128 (0 = 64); lens NULL, or int32 [B] on the
 * device = ns2_attention_train_fwd_lens's contract (then no key_mask / dropout, Nq == Nk) */
int ns2_attention_train_fwd_hd(const ns2_attn_args* args, const int* lens, void* stream);
/* ns2_attention_delta with heads of head_dim columns */
int ns2_attention_delta_hd(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H, int Nq,
                           int head_dim, float* delta, int o_precision, void* stream);
/* ns2_attention_bwd / ns2_attention_bwd_lens with head h at columns col0 + head_dim * h; scale is the caller's (head_dim ** -0.5) */
int ns2_attention_bwd_hd(const ns2_attn_bwd_args* args, int head_dim, const int* lens, void* stream);

/* ---- training of the conditioning encoders (NS2:228-341, 1073-1115; trained jointly with the denoiser: NS2:1538-1543, 1635) ----
 * Transformer's attention has two things Model's has not, a key-padding mask and dropout on the softmax output: the key_mask and
 * dropout_* fields of ns2_attn_args / ns2_attn_bwd_args.  On ragged text and prompts every attention of the conditioning trains on
 * these same kernels under byte masks formed on the device from the lengths, and rows behind a length are selected to zero by the caller
 * (ns2_zero_rows_lens); the one kernel that mixes rows and has a backward of its own with lengths is ns2_groupnorm_silu_bwd_lens. */
/* debugging / tests: out [B, H, Nq, Nk] bytes, 1 where the kernels above keep P[b, h, q, k] */
int ns2_dropout_keep_mask(const uint32_t* seed, unsigned call, float dropout_p, int B, int H, int Nq, int Nk, uint8_t* out, void* stream);
/* SiLU of the encoders' k = 9 convolutions (NS2:247, 306-311) on the fp32 pre-activation x [M, ldx], C columns, and its backward
 * dx = dy silu'(x).  Leading dimensions multiples of 4, 16-byte aligned pointers. */
int ns2_silu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream);
int ns2_silu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream);
/* gradient of PhonemeEncoder's token embedding (NS2:281-284): dw [rows, d] = sum of dy [M, lddy] rows per id, negative ids counting as
 * pad_id (an ordinary row of the table, as upstream); summed in ascending token order: bit-reproducible */
int ns2_embedding_bwd(const int64_t* ids, int64_t M, int pad_id, const float* dy, int64_t lddy, int rows, int d, float* dw, void* stream);

/* ---- training of the DurationPitchPredictor (NS2:344-527; its duration / pitch L1 terms, NS2:1578-1589) ----
 * The training FORWARD of GroupNorm + SiLU (+ residual) is ns2_groupnorm_silu with an fp32 output: the caller keeps its workspace, which
 * holds the per-chunk (count, mean, M2) slots.  ns2_groupnorm_silu_bwd takes that buffer as `stats` and combines the slots in the same
 * order with the same code, so it normalises with the forward's mean and rstd bit for bit.  With xh = (x - mean) rstd, z = xh w + b,
 * dz = dy silu'(z):  dweight_dbias [2 C] = (sum dz xh | sum dz) over all rows;  dx = rstd (dz w - s1 / N - xh s2 / N), s1 = sum dz w,
 * s2 = sum dz w xh per (utterance, group), N = n C / groups.  (The residual's gradient is dy itself.)  dy [B n, lddy], x and dx [B n, C].
 * Column sums per 32-row chunk go to fixed slots of the workspace and are added in a fixed order: no atomics, bit-reproducible. */
int64_t ns2_groupnorm_silu_bwd_workspace_bytes(int B, int n, int C);
int ns2_groupnorm_silu_bwd(const float* dy, int64_t lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                           const float* bias, float eps, const void* stats, int64_t stats_bytes, float* dx, float* dweight_dbias,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* ns2_groupnorm_silu_bwd with a row count per utterance.
 *   row_lens  int32 [B] in device memory, read by the kernels alone and clamped into [1, n].
 *   stats     the workspace ns2_groupnorm_silu_lens filled with its fp32 output (out_f32): the training forward of a ragged batch is
 *             that entry; the backward recombines its slots, so it normalises with the forward's mean and rstd, bit for bit.
 * The per-(utterance, group) sums s1, s2 and the count N = len_b * C / groups run over rows [0, len_b) only.  Rows of x and dy at or
 * beyond a length are NOT READ: NaN there reaches nothing.  Rows of dx at or beyond a length are written as all-zero bits.
 * dweight | dbias sum the rows [0, len_b) of every utterance.
 * Same fixed slots and the same fixed combination order as ns2_groupnorm_silu_bwd: a chunk of rows wholly behind a length contributes a
 * slot of zeros, the boundary chunk its rows before the length -- no atomics, bit-reproducible.  The rows of dx before a length are bit
 * for bit those of ns2_groupnorm_silu_bwd on the utterance alone at n = len_b (whose forward is ns2_groupnorm_silu alone).
 * row_lens == NULL: the launches of ns2_groupnorm_silu_bwd.  The arguments are checked before any device call (NS2_ERR_ARG).
 * Sizes: stats_bytes >= ns2_groupnorm_workspace_bytes(B, n, C, groups), workspace_bytes >= ns2_groupnorm_silu_bwd_workspace_bytes(B, n, C):
 * the size functions of the entries without lengths. */
int ns2_groupnorm_silu_bwd_lens(const float* dy, int64_t lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                                const float* bias, float eps, const void* stats, int64_t stats_bytes, const int* row_lens, float* dx,
                                float* dweight_dbias, void* workspace, int64_t workspace_bytes, void* stream);
/* backward of out = relu(h . w + b) (ns2_row_dot with relu): g = dout where out > 0 else 0;  dh [M, lddh] = g w;  dw_db [K + 1] =
 * (sum_m g h[m, :] | sum_m g), from per-64-row slots added in a fixed order.  K, ldh, lddh multiples of 4. */
int64_t ns2_row_dot_relu_bwd_workspace_bytes(int64_t M, int K);
int ns2_row_dot_relu_bwd(const float* dout, const float* out, const float* h, int64_t ldh, const float* w, int64_t M, int K, float* dh,
                         int64_t lddh, float* dw_db, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training of the Aligner (aligner.py; the only route that hands it a gradient is the forward-sum / bin loss of NS2:1587-1602) ----
 * Exact arithmetic, fixed summation orders, no atomics: two runs give the same bits.  Lengths are int32 [B] on the device, clamped to
 * [0, size]; nothing here reads device data on the host.  Limits: n <= 1024, T <= 8192, C <= 256. */
/* ReLU between AlignerNet's convolutions (aligner.py:30-51) on the kept fp32 pre-activation x [M, ldx], C columns, and its backward
 * dx = dy where x > 0.  Leading dimensions multiples of 4, 16-byte aligned pointers (as ns2_silu_fwd / ns2_silu_bwd). */
int ns2_relu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream);
int ns2_relu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream);
/* backward of ns2_align_attn (aligner.py:72-90: cdist, masked fill, softmax).  queries [B * T, C], keys [B * n, C], aln_log
 * [B, 1, T, n] and aln_soft [B, n, T] as ns2_align_attn wrote them, g_log [B, 1, T, n] and g_soft [B, n, T] the gradients of the two
 * outputs (either may be null).  With G = g_log + soft (g_soft - sum_i soft g_soft) on the live cells (i < text_lens[b]) and
 * w = G / dist, w = 0 where the cell is masked or dist == 0 (torch.cdist's convention: never NaN or inf):
 *   dq [B * T, C]: dq_t = sum_i w (q_t - k_i), phonemes in ascending order;
 *   dk [B * n, C]: dk_i = sum_t w (k_i - q_t), per slice of 256 frames in ascending order, the slices through the fixed-order
 *   slice reducer (ns2_reduce_slices' kernel).  The DIRECT form is summed (rowsum(w) q - w K cancels where q ~ k).
 * workspace = ns2_align_attn_bwd_workspace_bytes bytes: w [B, T, n] fp32 + ceil(T / 256) slots of [B, n, C] fp32; 16-byte aligned. */
int64_t ns2_align_attn_bwd_workspace_bytes(int B, int T, int n, int C);
int ns2_align_attn_bwd(const float* queries, const float* keys, const float* aln_log, const float* aln_soft, const float* g_log,
                       const float* g_soft, const int* text_lens, int B, int T, int n, int C, float* dq, float* dk, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* ForwardSumLoss and BinLoss (aligner.py:132-167, 169-183) on aln_log [B, 1, T, n]; each loss is requested by a non-null output
 * pointer (a device scalar), both share the row statistics.
 * Forward-sum: per frame t < mel_lens[b] the log-softmax over [blank_logprob | aln_log[t, 0 .. L - 1]], L = text_lens[b] (columns
 * > L of the n + 1 wide row are excluded); CTC with blank 0, targets 1 .. L, S = 2 L + 1 states, every skip between labels allowed
 * (they are distinct); zero_infinity (an infeasible utterance gives loss 0, gradient 0); fs_loss = mean_b(nll_b / max(L_b, 1)).
 * One workgroup per utterance runs the alpha recursion over the frames, the states spread over its lanes, and keeps alpha
 * [B, T, 2 n + 1] in the workspace.  Arithmetic: fp64 on probabilities scaled per frame by a power of two (the exponent of the frame
 * before's maximum: exact, and the sum of the exponents gives nll) -- an fp32 log-space recursion leaves the gradient 300 .. 10000 x 2^-24
 * of its largest element off (so does torch's fp32 ctc_loss); emissions below e^-700 count as e^-700.
 * Bin: bin_loss = sum(hard log_softmax(aln_log over the columns <= L)) / B, hard [B, n, T] the 0/1 path (column L is kept, as upstream:
 * it holds the aligner's -FLT_MAX).
 * ns2_align_losses_bwd (same aln_log, hard, lengths, blank_logprob and the workspace the forward filled): d_log [B, 1, T, n] =
 * g_fs (softmax - occupancy) / (max(L, 1) B) on the live cells of the frames t < mel_len (beta recursion, the occupancies of a frame
 * normalised to sum 1 over its states; the blank column's share is dropped) + g_bin (hard - softmax sum_i hard) / B on the columns <= L; exactly 0 elsewhere.  g_fs, g_bin: device scalars, the
 * gradients of the two losses (null = that loss takes no part).
 * workspace = ns2_align_losses_workspace_bytes bytes: 4 floats per frame, B doubles, 2 B T (2 n + 1) floats (alpha, and the backward's
 * alpha + beta: the forward's part is only read, so a backward may be repeated). */
int64_t ns2_align_losses_workspace_bytes(int B, int T, int n);
int ns2_align_losses_fwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, int B, int T, int n,
                         float blank_logprob, float* fs_loss, float* bin_loss, void* workspace, int64_t workspace_bytes, void* stream);
int ns2_align_losses_bwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, const float* g_fs,
                         const float* g_bin, int B, int T, int n, float blank_logprob, float* d_log, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* RVQ cross-entropy of the training loss (NS2:1668-1684, `codec.rq(x_start, codes)`; csrc/rvq_ce.hip), everything fp32.  For the M rows of
 * x [M, D] and per quantizer q: dist_c = |r_q - E_q[c]|, row_loss[m][q] = log sum_c exp(-dist_c) + dist_target with target =
 * indices[m][q]; r_{q+1} = r_q - (the code nearest to r_q); loss[0] = sum_q mean_m row_loss[m][q], summed in a fixed order.
 * Optional outputs (null = not wanted): quantized_out [M, D] = 0 + E_0[nearest_0] + E_1[nearest_1] + ... in fp32, in stage order;
 * grad [M, D] = d loss / d x (the nearest codes are constants: sum_q d row_loss_q / d r_q, divided by M) -- null skips the second
 * sweep over the codebooks that forms it.  No atomics: loss and grad are bit-reproducible, and the loss does not depend on whether grad is asked for.
 * Defined edge behaviour: an index outside [0, C) (-1 included) makes that row's losses, hence loss[0], and its row of grad NaN -- no
 * error code, no host read; a residual that equals a code (dist = 0) gives the well-defined loss and that code contributes 0 to grad;
 * near-ties of the nearest code are decided by the fp32 scores (ns2_rvq_encode re-decides them in fp64, this one does not).
 * cb_norm: what ns2_rvq_prepare filled.  workspace: ns2_rvq_ce_workspace_bytes(M, Q, quantized_out != null) bytes (0 without
 * quantized_out).  NS2_ERR_ARG for D != 128 or C % 64 != 0, as ns2_rvq_encode. */
int64_t ns2_rvq_ce_workspace_bytes(int M, int Q, int want_quantized);
int ns2_rvq_ce(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss, float* loss,
               float* quantized_out, float* grad, int M, int Q, int C, int D, void* workspace, int64_t workspace_bytes, void* stream);
/* ns2_rvq_ce of a ragged batch of B utterances padded to n frames: x [B n, D], indices [B n, Q], row_loss [B n, Q],
 * quantized_out and grad [B n, D] (each may be null), row_lens [B] clamped into [1, n].  With len_b = row_lens[b]:
 *   loss[0]       = (1 / B) sum_b (1 / len_b) sum_{t < len_b} sum_q row_loss[b, t, q]      (the mean over utterances of each one's own loss)
 *   grad[b, t, :] = (1 / (B len_b)) sum_q dL/dr_q                                          for t < len_b
 * The loss is summed in a fixed order without atomics (bit-reproducible) and does not depend on whether grad is asked for.  Rows
 * t < len_b of row_loss (and of quantized_out) are bit for bit those of ns2_rvq_ce on the utterance alone.  Rows t >= len_b of row_loss,
 * quantized_out and grad are exact zeros; x and indices are not read there, so an index of -1 or garbage behind a length makes nothing
 * NaN, while an index outside [0, C) BEFORE a length keeps the loud NaN of ns2_rvq_ce.  A workgroup whose 128 rows all lie behind
 * their lengths loads no codebook tile.  workspace: ns2_rvq_ce_workspace_bytes(B * n, Q, quantized_out != null) bytes. */
int ns2_rvq_ce_lens(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss, float* loss,
                    float* quantized_out, float* grad, int B, int n, const int* row_lens, int Q, int C, int D, void* workspace,
                    int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NS2HIP_TRAIN_H */
