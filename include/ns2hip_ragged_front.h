/* Ragged prompts and text in libns2hip: per-utterance lengths through the front-end (SpeechPromptEncoder, DurationPitchPredictor, the
 * conditioning of Model).  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  Status codes, ns2_last_error
 * and ns2_model are those of ns2hip.h, which this header includes.
 *
 * The definition is that of ns2hip_ragged.h: utterance i of a ragged batch equals utterance i run alone, here with its text cut to
 * text_lens[i] and its prompt cut to prompt_lens[i].  The GEMM and attention kernels are unchanged: a row never sees another row in a
 * GEMM, the attention kernels already take key counts / key masks, and what mixes rows apart from them -- the "same" convolutions, the
 * GroupNorm statistics, the mean over the prompt -- is handled by the entries below, each a launch of its own.
 *
 * Lengths are int32 [B] in DEVICE memory, read by the kernels alone, never on the host, and clamped into [1, n].  What lies at or
 * beyond a length may hold anything, NaN included, and does not reach what lies before it.  Every entry checks its arguments before
 * any device call (NS2_ERR_ARG). */
#ifndef NS2HIP_RAGGED_FRONT_H
#define NS2HIP_RAGGED_FRONT_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_groupnorm_silu with a row count per utterance.  The statistics of (b, group) are taken over rows [0, row_lens[b]) in the same
 * fixed slots (a chunk wholly behind the length counts 0 values, the boundary chunk the rows before the length): bit-equal to the
 * utterance alone at n = row_lens[b].  Rows at or beyond the length are not read, nor is their residual; they are written as zeros, in
 * fp32 and in the planes.  row_lens == NULL: the launches of ns2_groupnorm_silu.  Workspace: ns2_groupnorm_workspace_bytes. */
int ns2_groupnorm_silu_lens(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                            const float* resid, const int* row_lens, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo,
                            int precision, void* workspace, int64_t workspace_bytes, void* stream);

/* Zero-fill rows [lens[b], n) of every utterance of a row-major [B * n, row_bytes] buffer with 16-byte stores: row_bytes % 16 == 0, buf
 * 16-byte aligned.  All-zero bits are 0.0 in fp32 and in every operand-plane format (pass the physical bytes of a plane row). */
int ns2_zero_rows_lens(void* buf, int64_t row_bytes, int B, int n, const int* lens, void* stream);

/* out[b, :] = mean of in[b, 0 .. lens[b], :] over fp32 rows in [B, n, d] -> [B, d], summed in ascending row order. */
int ns2_mean_rows_lens(const float* in, int B, int n, int d, const int* lens, float* out, void* stream);

/* ns2_model_prepare_cond with a prompt row count per utterance: to_prompt_cond takes the mean over rows [0, prompt_lens[b]), and the
 * perceiver resampler attends to keys [0, Lm + prompt_lens[b]) of cat(latents, prompt) (ns2_attention_fwd_lens's path; the key counts
 * are made on the device).  Prompt rows at or beyond a length may hold NaN.  The drop branch (null substitutes) ignores the lengths.
 * prompt_lens == NULL: the launches of ns2_model_prepare_cond.  Same workspace and cond_state sizes. */
int ns2_model_prepare_cond_lens(ns2_model* m, const float* prompt, int n_prompt, const int* prompt_lens, const float* cond, int n_cond,
                                int drop, int B, int N, void* cond_state, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
