/* Ragged batches in libns2hip: skipping the hidden row tiles of a sampling batch in every product.  Part of the C ABI: listed in
 * _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  Status codes, ns2_last_error, ns2_linear_args, ns2_attn_args, ns2_weight, ns2_model and ns2_model_config
 * are those of ns2hip.h, which this header includes.
 *
 * ns2hip_ragged.h made a ragged batch correct: the lengths go to the self-attention, every other kernel computes every row.  Here the
 * lengths go to every product.  For a batch [B, N] with N % 256 == 0 and device lengths lens (int32 [B], clamped by the kernels into
 * [1, N]) the COMPUTED EXTENT of utterance i is
 *
 *     H_i = min(N, 256 * ceil(lens_i / 256))
 *
 * and row r of utterance i is HIDDEN when r >= H_i.  One granule of 256 rows for every kernel, whatever its own tile height (128 and
 * 256 rows in the GEMM family, 128 and 256 query rows in the attention kernels): producers and consumers agree on which rows exist.
 * A workgroup whose whole row tile is hidden returns before its first load; rows in [lens_i, H_i) share a tile with real frames and
 * are computed exactly as without skipping.  No bit of a row before H_i changes: the convolutions are causal, the self-attention
 * stops at the key counts, everything else is row-local, so a visible row never reads a hidden one.
 *
 * What a hidden tile leaves behind: an fp32 output WITHOUT a residual gets exact zeros (the residual stream's first write and
 * to_pred's output are read row by row by code that does not skip); every other output -- operand planes, V^T, an fp32 output that
 * accumulates into a residual -- keeps what it held.
 *
 * Lengths are read by the kernels alone, never on the host: a launch captured into a HIP graph follows values rewritten between
 * replays.  The split-K route (batches of one to four utterances) takes no lengths. */
#ifndef NS2HIP_RAGGED_SKIP_H
#define NS2HIP_RAGGED_SKIP_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_linear on a ragged batch of args->M / seq_len utterances of seq_len rows each: row tiles at or behind an utterance's computed
 * extent are skipped (out_f32 without resid: zeros there; every other output untouched).  Refused (NS2_ERR_ARG, before any device
 * call) when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0, or when args->seq_len is set and differs.
 * Whatever ns2_linear refuses is refused alike.  A product that splits K (ns2_debug_force_gemm 0 / 4 on a small batch) computes
 * every row. */
int ns2_linear_lens(const ns2_linear_args* args, const int* row_lens, int seq_len, void* stream);

/* ns2_wavenet_block on a ragged batch (M / seq_len utterances): the same refusals as ns2_linear_lens on row_lens, seq_len and M.
 * Hidden row tiles of out_hi / out_lo keep what they held. */
int ns2_wavenet_block_lens(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                           int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                           uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, const int* row_lens, void* stream);

/* ns2_attention_fwd_lens (key_lens != NULL) / ns2_attention_fwd (key_lens == NULL: the cross attention to the resampled prompt has
 * query lengths alone) with per-utterance frame counts on the query side: a query workgroup whose rows all lie at or behind
 * H_b = min(Nq, 256 ceil(query_lens[b] / 256)) returns before its first load, and its rows of o keep what they held.  Key handling
 * is unchanged.  Refused (NS2_ERR_ARG, before any device call) when args or query_lens is null, args->Nq % 256 != 0, or
 * args->key_mask, args->lse or args->dropout_p is set. */
int ns2_attention_fwd_skip(const ns2_attn_args* args, const int* key_lens, const int* query_lens, void* stream);

/* ns2_model_forward_lens with skipping.  frame_lens == NULL is an argument error (ns2_model_forward_lens is the call that allows it).
 * The skipping step runs when the SKIP RULE holds: N % 256 == 0 and no product of the described step is planned on the split-K
 * route; otherwise exactly the launches of ns2_model_forward_lens are issued.  In a skipping step every product and both attention
 * kernels skip hidden row tiles; rows of out at or behind H_i are exact zeros, rows before it have the bits ns2_model_forward_lens
 * gives.  Two utterance chains and a captured step work as there. */
int ns2_model_forward_lens_skip(ns2_model* m, const float* x, const float* times, const float* cond_row, const int* frame_lens,
                                const void* cond_state, int n_cond, float* out, int B, int N, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* Test hooks.  ns2_debug_skip_rule: the skip rule for a configuration, without a device (pure host arithmetic over the described
 * launches, like ns2_debug_chain_rule): *skips = 1 when a forward of B x N frames would run the skipping step.
 * ns2_debug_skip_last: 1 when the last forward of the process -- through any of the model's forward entries -- ran the skipping step,
 * else 0 (a plain ns2_model_forward resets it).
 * ns2_debug_gemm_route_launches: products that ns2_linear / ns2_wavenet_block / the model's steps have sent down a route so far, route =
 * 0 split-K, 1 the 128 x 128 kernel, 2 the 256 x 256 kernel, 3 the FF conv kernel, 4 the lean linear kernel, 5 the lean Wavenet kernel
 * (-1 for any other value): kernels of different routes may give the same bits, so the routing tests read the counter around a call. */
int ns2_debug_skip_rule(const ns2_model_config* cfg, int B, int N, int* skips);
int ns2_debug_skip_last(void);
int64_t ns2_debug_gemm_route_launches(int route);

#ifdef __cplusplus
}
#endif
#endif
