/* Ragged RAW AUDIO in the training pass of libns2hip: per-utterance sample counts in the mel spectrogram and the pitch extractor, and
 * per-utterance frame counts in the RVQ cross-entropy term.  Part of the C ABI: listed in _lib.HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).  Status codes and ns2_last_error are those of ns2hip.h.
 *
 * The definition is that of ns2hip_ragged.h and ns2hip_ragged_train.h: what utterance i yields in the padded batch is what it yields
 * ALONE, cut to its length.  Whatever lies at or behind a length -- NaN included -- reaches no value and no gradient before it, and what
 * is returned at or behind a length is an exact 0.
 *
 * Lengths are int32 [B] in DEVICE memory and are read by the kernels alone, never on the host: a launch captured into a HIP graph
 * follows values rewritten between replays.  A kernel clamps a value outside its range into it (the host cannot check it without a
 * read).  Every entry checks its other arguments before any device call (NS2_ERR_ARG) and refuses a null length pointer: the entries
 * without lengths stay the calls without lengths. */
#ifndef NS2HIP_RAGGED_AUDIO_H
#define NS2HIP_RAGGED_AUDIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_audio_to_mel (ns2hip.h) of a ragged batch: audio [B, L], sample_lens [B], out [B, n_mels, T], T = 1 + L / hop_length.  A length is
 * clamped into [n_fft / 2 + 1, L] (one reflection must stay in range).  With T_b = 1 + sample_lens[b] / hop_length, frames t < T_b are
 * bit for bit those of ns2_audio_to_mel on the utterance alone at L = sample_lens[b]: the reflection of torch.stft(center=True) is taken
 * about the utterance's own last sample.  Frames t >= T_b are exact 0.0f -- padding, not the -100 dB of silent audio -- and a block
 * whose frames all lie there reads no sample and runs no FFT.  Samples at or behind a length are never read into a result. */
int ns2_audio_to_mel_lens(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window, const float* twiddle,
                          const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db, float* out,
                          const int* sample_lens, void* stream);

/* ns2_pitch_yin (ns2hip_pitch.h) of a ragged batch: frame i of utterance b reads zeros outside [0, sample_lens[b]).  A length is clamped
 * into [1, L].  Frames t < T_b (as above) are bit for bit those of ns2_pitch_yin on the utterance alone; frames t >= T_b are exact 0
 * (unvoiced), and their blocks return early. */
int ns2_pitch_yin_lens(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max, float threshold,
                       float* f0, const int* sample_lens, void* stream);

/* ns2_rvq_ce (ns2hip.h) of a ragged batch of B utterances padded to n frames: x [B n, D], indices [B n, Q], row_loss [B n, Q],
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
#endif
