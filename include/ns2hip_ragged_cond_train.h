/* Ragged text and prompts in the TRAINING pass of libns2hip: per-utterance lengths through the conditioning (SpeechPromptEncoder,
 * PhonemeEncoder, DurationPitchPredictor, the conditioning of Model).  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).
 * Status codes and ns2_last_error are those of ns2hip.h.
 *
 * The definition is that of ns2hip_ragged_front.h: utterance i of a padded batch is utterance i run alone with its text cut to
 * text_lens[i] and its prompt cut to prompt_lens[i] -- here for the gradients too.  The attention kernels are unchanged: every attention
 * of the conditioning trains on the existing key-mask / dropout kernels under byte masks formed on the device from the lengths, and rows
 * behind a length are selected to zero by the caller (ns2_zero_rows_lens).  The one kernel that mixes rows, has a backward and took no
 * lengths is GroupNorm + SiLU; its forward with lengths is ns2_groupnorm_silu_lens (ns2hip_ragged_front.h), its backward is below.
 *
 * Lengths are int32 [B] in DEVICE memory, read by the kernels alone, never on the host, and clamped into [1, n]: a launch captured into
 * a HIP graph follows values rewritten between replays. */
#ifndef NS2HIP_RAGGED_COND_TRAIN_H
#define NS2HIP_RAGGED_COND_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_groupnorm_silu_bwd (ns2hip.h) with a row count per utterance.
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

#ifdef __cplusplus
}
#endif
#endif
