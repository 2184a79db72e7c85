/* libns2hip: the conditioning front-end -- the DurationPitchPredictor, the Aligner and the row kernels of ragged prompts and text.
 * Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  The conventions, the status codes and the definition
 * of a ragged batch are those of ns2hip.h, which this header includes. */
#ifndef NS2HIP_FRONTEND_H
#define NS2HIP_FRONTEND_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ DurationPitchPredictor and text-conditioned sampling
 * (NS2:344-527, 87-104, 164-175, 1449-1455, 1476-1483).  The trunk's convolutions are ns2_linear calls (conv_taps = k,
 * pad_left = k / 2), its RMSNorm and attention ns2_rmsnorm and ns2_attention_fwd; these are the pieces around them.
 * ns2_groupnorm_silu: nn.GroupNorm(groups, C) + SiLU (Block, NS2:346-369) over token-major fp32 rows x [B * n, C], statistics
 * per (utterance, group) over n x C / groups values, eps as given; resid (may be null) [B * n, C] is added after the SiLU (the
 * second Block of a ResnetBlock, NS2:394-398).  Outputs: out_f32 [B * n, C] and / or operand planes (out_hi, out_lo, ldo = C)
 * in the format of `precision`.  C / groups must be a multiple of 4 (and C of 32 for planes); fp32 buffers 16-byte aligned.
 * workspace = ns2_groupnorm_workspace_bytes(B, n, C, groups) bytes of caller-owned scratch: per-chunk (count, mean, M2)
 * partials in fixed slots, combined in a fixed order -- the result is bit-reproducible. */
int64_t ns2_groupnorm_workspace_bytes(int B, int n, int C, int groups);
int ns2_groupnorm_silu(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                       const float* resid, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* ns2_groupnorm_silu with a row count per utterance.  The statistics of (b, group) are taken over rows [0, row_lens[b]) in the same
 * fixed slots (a chunk wholly behind the length counts 0 values, the boundary chunk the rows before the length): bit-equal to the
 * utterance alone at n = row_lens[b].  Rows at or beyond the length are not read, nor is their residual; they are written as zeros, in
 * fp32 and in the planes.  row_lens == NULL: the launches of ns2_groupnorm_silu.  Workspace: ns2_groupnorm_workspace_bytes. */
int ns2_groupnorm_silu_lens(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                            const float* resid, const int* row_lens, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo,
                            int precision, void* workspace, int64_t workspace_bytes, void* stream);
/* totals[b] = sum_i int(duration[b, i]) (generate_mask_from_repeats, NS2:87-92; negative durations count as 0 frames):
 * the caller reads max(totals) = n_frames for ns2_length_regulate */
int ns2_length_regulate_totals(const float* duration, int B, int n_ph, int* totals, void* stream);
/* the length regulator of NaturalSpeech2.sample (NS2:1478-1483): frame f < n_frames of utterance b takes the phoneme whose
 * [exclusive, inclusive) prefix of int(duration[b]) holds f (none past the utterance's total: zeros), and
 * out[b, :, f] = enc[b, ph, :] + pitch_table[f0_to_coarse(pitch[b, ph]), :]   (NS2:164-175, 1449-1455)
 * duration / pitch [B, n_ph], enc [B, n_ph, D], pitch_table [>= 256, D], out [B, D, n_frames]; mel_min / mel_max = the fp32
 * constants 1127 log(1 + f0_min / 700) / 1127 log(1 + f0_max / 700) of f0_to_coarse.  n_ph <= 8192. */
int ns2_length_regulate(const float* duration, const float* pitch, const float* enc, const float* pitch_table, int B, int n_ph,
                        int D, int n_frames, float mel_min, float mel_max, float* out, void* stream);
/* out[m] = act(x[m, :K] . w + bias[0]), act = ReLU when relu != 0 (to_pred: Linear(dim, 1) + ReLU, NS2:467-471); bias may be
 * null; K and ldx multiples of 4, x and w 16-byte aligned */
int ns2_row_dot(const float* x, int ldx, int M, int K, const float* w, const float* bias, int relu, float* out, void* stream);

/* ---- Aligner (aligner.py) and the text-conditioned training pass (NS2:1524-1602).  Lengths are int32 [B] on the device,
 * clamped to [0, size] as create_mask (utils.py:28-33) would; nothing here reads device data on the host. */
/* planes [M, ldo] <- ReLU(x [M, N]) in the operand format of `precision`, columns N .. ldo - 1 zero (AlignerNet's ReLUs between
 * its convolutions, aligner.py:30-51); N % 4 == 0, ldo % 32 == 0 */
int ns2_relu_split(const float* x, int M, int N, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
/* AlignerNet attention (aligner.py:72-90): queries [B * T, C], keys [B * n, C] fp32 token-major; aln_log [B, 1, T, n] =
 * the Euclidean distance summed in fp32 (no negation, no temperature), -FLT_MAX at phonemes >= text_lens[b]; aln_soft
 * [B, n, T] = softmax over phonemes, transposed (a fully masked row is uniform).  n <= 1024, C <= 256 */
int ns2_align_attn(const float* queries, const float* keys, const int* text_lens, int B, int T, int n, int C, float* aln_log,
                   float* aln_soft, void* stream);
/* maximum_path (aligner.py:97-130) of value [B, t_x, t_y] fp32 under the prefix masks text_lens x mel_lens: path [B, t_x, t_y]
 * 0/1 fp32, bit for bit the reference's (ties stay, direction 1 outside the mask, backtrack from row text_len - 1), and
 * durations [B, t_x] int32 = its row sums.  t_x <= 1024, t_y <= 8192; workspace = ns2_maximum_path_workspace_bytes bytes
 * (the per-column path rows, plus the direction bits when t_x_pad * t_y / 8 bytes exceed 128 KiB of LDS) */
int64_t ns2_maximum_path_workspace_bytes(int B, int t_x, int t_y);
int ns2_maximum_path(const float* value, const int* text_lens, const int* mel_lens, int B, int t_x, int t_y, float* path,
                     int* durations, void* workspace, int64_t workspace_bytes, void* stream);
/* average_over_durations (utils.py:4-26): pitch [B, T] (the reference's [B, 1, T]), durations [B, n] int32 -> out [B, n] = mean
 * of the non-zero frames of each phoneme from fp32 prefix sums, 0 where none.  T, n <= 8192 */
int ns2_average_over_durations(const float* pitch, const int* durations, int B, int T, int n, float* out, void* stream);
/* backward of expand_encodings with durations (NS2:1449-1455, the forward is ns2_length_regulate): d_cond [B, D, n_frames],
 * duration / pitch [B, n] fp32 -> d_enc [B, n, D] = sum of d_cond over each phoneme's frames, d_table [n_bins, D] (null: skip)
 * = sum over (b, i) in ascending order of the rows of d_enc whose f0_to_coarse(pitch) is the bin.  No atomics: bit-reproducible.
 * workspace = ns2_expand_backward_workspace_bytes(B, n) bytes */
int64_t ns2_expand_backward_workspace_bytes(int B, int n);
int ns2_expand_backward(const float* d_cond, const float* duration, const float* pitch, int B, int n, int D, int n_frames, int n_bins,
                        float mel_min, float mel_max, float* d_enc, float* d_table, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ---- ragged prompts and text (SpeechPromptEncoder, DurationPitchPredictor, the conditioning of Model)
 * Utterance i of a ragged batch equals utterance i run alone, here with its text cut to
 * text_lens[i] and its prompt cut to prompt_lens[i].  The GEMM and attention kernels are unchanged: a row never sees another row in a
 * GEMM, the attention kernels already take key counts / key masks, and what mixes rows apart from them -- the "same" convolutions, the
 * GroupNorm statistics, the mean over the prompt -- is handled by ns2_groupnorm_silu_lens, the two entries below and
 * ns2_model_prepare_cond_lens (ns2hip.h), each a launch of its own.  What lies at or beyond a length does not reach what lies before it. */
/* Zero-fill rows [lens[b], n) of every utterance of a row-major [B * n, row_bytes] buffer with 16-byte stores: row_bytes % 16 == 0, buf
 * 16-byte aligned.  All-zero bits are 0.0 in fp32 and in every operand-plane format (pass the physical bytes of a plane row). */
int ns2_zero_rows_lens(void* buf, int64_t row_bytes, int B, int n, const int* lens, void* stream);

/* out[b, :] = mean of in[b, 0 .. lens[b], :] over fp32 rows in [B, n, d] -> [B, d], summed in ascending row order. */
int ns2_mean_rows_lens(const float* in, int B, int n, int d, const int* lens, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NS2HIP_FRONTEND_H */
