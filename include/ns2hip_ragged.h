/* Ragged batches in libns2hip: per-utterance lengths in the attention kernels.  Part of the C ABI: listed in _lib.HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).  Status codes, ns2_last_error, ns2_attn_args and ns2_model are those of ns2hip.h, which this header includes.
 *
 * The definition: utterance i of a ragged batch equals utterance i run alone at its own length.  In Model the self-attention is the
 * one thing through which a frame sees later frames (the convolutions are causal; norms, FiLM and the cross-attention to the
 * resampled prompt work per frame), so the lengths go to the self-attention kernels and to nothing else.
 *
 * Lengths are int32 [B] in DEVICE memory and are read by the kernels alone, never on the host: a launch captured into a HIP graph
 * follows values rewritten between replays.  A kernel clamps a value outside [1, N] into that range (no read out of bounds, no
 * empty softmax).  Keys at or beyond an utterance's length are treated as keys at or beyond Nk: score -inf, K rows and V^T columns
 * read as zeros -- what lies there may be anything, NaN included.  Query rows at or beyond the length are computed like any other
 * row, attending to the keys before it: every output is finite and defined. */
#ifndef NS2HIP_RAGGED_H
#define NS2HIP_RAGGED_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_attention_fwd with per-utterance key counts: utterance b attends to keys [0, key_lens[b]).  args->Nk stays the stride of k and
 * of the V^T rows.  Refused (NS2_ERR_ARG, before any device call) when args or key_lens is null or when args->key_mask, args->lse
 * or args->dropout_p is set: key counts belong to the plain inference forward.  Precisions 2 / 4 at head_dim 64 with Nq % 256 == 0
 * and Nk % 64 == 0 run attn_fast_kernel and skip whole key tiles beyond a length; every other shape runs attn_kernel. */
int ns2_attention_fwd_lens(const ns2_attn_args* args, const int* key_lens, void* stream);

/* ns2_model_forward (times != NULL) / ns2_model_forward_row (cond_row != NULL) with per-utterance frame counts: exactly one of
 * times / cond_row.  frame_lens == NULL: the same launches as those two entries. */
int ns2_model_forward_lens(ns2_model* m, const float* x, const float* times, const float* cond_row, const int* frame_lens,
                           const void* cond_state, int n_cond, float* out, int B, int N, void* workspace, int64_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
