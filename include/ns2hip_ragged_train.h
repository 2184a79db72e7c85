/* Ragged batches in the TRAINING pass of libns2hip: per-utterance lengths in the denoiser's self-attention, forward and backward.
 * Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  Status codes, ns2_last_error, ns2_attn_args and ns2_attn_bwd_args are those of
 * ns2hip.h, which this header includes.
 *
 * The definition is that of ns2hip_ragged.h, carried through the gradient: with lengths lens[i] in [1, N], utterance i contributes to
 * every output and to every gradient exactly what it contributes when run ALONE at lens[i] rows.  Whatever the operands hold at or
 * beyond lens[i] -- NaN included -- never reaches a value or a gradient before it.  Output rows and gradient rows at or beyond a
 * length are exact zeros, so what follows them in the pass (the weight-gradient GEMMs, the bias and FiLM sums) needs no lengths.
 *
 * Lengths are int32 [B] in DEVICE memory and are read by the kernels alone, never on the host: a launch captured into a HIP graph
 * follows values rewritten between replays.  A kernel clamps a value outside [1, N] into that range.  Self-attention only
 * (Nq == Nk = N, the stride of every address); whole 64-row tiles beyond a length are neither fetched nor multiplied. */
#ifndef NS2HIP_RAGGED_TRAIN_H
#define NS2HIP_RAGGED_TRAIN_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
