/* libns2hip: raw audio and the codec -- the mel spectrogram, the pitch extractor, the sample-rate converter, the pieces of EnCodec's
 * SEANet and LSTM, and its RVQ.  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  The conventions, the
 * status codes and the definition of a ragged batch are those of ns2hip.h, which this header includes.  The *_lens entries here refuse a
 * null length pointer: the entries without lengths stay the calls without lengths. */
#ifndef NS2HIP_AUDIO_H
#define NS2HIP_AUDIO_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- AudioToMel (audio_to_mel.py, NS2:181-224): audio [B, L] fp32 -> out [B, n_mels, T], T = 1 + L / hop_length.  The frames
 * are those of torch.stft(center=True, pad_mode="reflect", onesided=True), power |X|^2, mel = fb^T power summed in ascending
 * bins, and with log_db 10 log10(max(mel, 1e-10)).  Tables (host-built, fp64 rounded to fp32): window [n_fft] (Hann zero-padded
 * centred), twiddle [n_fft] complex (cos, sin)(-2 pi k / n_fft); the filterbank compactly as fb_meta [3][n_mels] int32 = first
 * bin, number of bins, offset into fb_w [n_w], with first + number <= n_bins (the bins read) <= n_fft / 2 + 1.  n_fft a power of
 * two in [256, 2048], 1 <= hop_length <= n_fft, n_mels <= 256, L > n_fft / 2.  No atomics: bit-reproducible per utterance. */
int ns2_audio_to_mel(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window, const float* twiddle,
                     const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db, float* out, void* stream);
/* ns2_audio_to_mel of a ragged batch: audio [B, L], sample_lens [B], out [B, n_mels, T], T = 1 + L / hop_length.  A length is
 * clamped into [n_fft / 2 + 1, L] (one reflection must stay in range).  With T_b = 1 + sample_lens[b] / hop_length, frames t < T_b are
 * bit for bit those of ns2_audio_to_mel on the utterance alone at L = sample_lens[b]: the reflection of torch.stft(center=True) is taken
 * about the utterance's own last sample.  Frames t >= T_b are exact 0.0f -- padding, not the -100 dB of silent audio -- and a block
 * whose frames all lie there reads no sample and runs no FFT.  Samples at or behind a length are never read into a result. */
int ns2_audio_to_mel_lens(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window, const float* twiddle,
                          const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db, float* out,
                          const int* sample_lens, void* stream);

/* YIN (de Cheveigne & Kawahara, JASA 2002, steps 1-5): audio [B, L] fp32 -> f0 [B, T] fp32 in Hz, 0 where unvoiced,
 * T = 1 + L / hop_length (the frames of ns2_audio_to_mel).  With W = 2 tau_max and S = 3 tau_max, frame i reads the S samples from
 * s_i = i hop_length - S / 2, zero outside [0, L):
 *   d(tau)  = sum_{j = 0}^{W - 1} (x[s_i + j] - x[s_i + j + tau])^2,  tau = 1 .. tau_max   (the direct form, not the autocorrelation)
 *   c(tau)  = sum_{k = 1}^{tau} d(k)
 *   d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1
 *   tau     = the first of tau_min .. tau_max with d'(tau) < threshold (none: f0 = 0), advanced while tau < tau_max and
 *             d'(tau + 1) < d'(tau)
 *   den     = d'(tau - 1) - 2 d'(tau) + d'(tau + 1);  delta = clamp(0.5 (d'(tau - 1) - d'(tau + 1)) / den, -1, 1) if
 *             tau + 1 <= tau_max and den > 0, else 0
 *   f0      = sample_rate / (tau + delta)
 * Callers derive tau_min = floor(sample_rate / f0_ceil) and tau_max = ceil(sample_rate / f0_floor).  The first and last frames
 * of an utterance see the zero padding and come out unvoiced, as does audio shorter than about one span.
 * 2 <= tau_min < tau_max <= 1024, hop_length >= 1, L >= 1, 1 <= B <= 65535.  One launch, fp32, no atomics, sums in a fixed
 * order: bit-reproducible, and a row does not depend on the rest of the batch. */
int ns2_pitch_yin(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max, float threshold,
                  float* f0, void* stream);
/* ns2_pitch_yin of a ragged batch: frame i of utterance b reads zeros outside [0, sample_lens[b]).  A length is clamped
 * into [1, L].  Frames t < T_b (T_b as in ns2_audio_to_mel_lens) are bit for bit those of ns2_pitch_yin on the utterance alone;
 * frames t >= T_b are exact 0 (unvoiced), and their blocks return early. */
int ns2_pitch_yin_lens(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max, float threshold,
                       float* f0, const int* sample_lens, void* stream);

/* Polyphase rational resampling by up / down (the rates divided by their gcd): audio [B, L] fp32 -> out [B, L_out] fp32,
 * L_out = ceil(up L / down).  With T = 2 width + down taps per phase,
 *   out[b, f up + p] = sum_{i = 0}^{T - 1} k[p][i] x[b, f down + i - width],   x = 0 outside [0, L),   p in [0, up),
 * stored for f up + p < L_out only.  `taps` is the table TRANSPOSED, [T][up] fp32 in device memory: taps[i up + p] = k[p][i], so that
 * lanes with neighbouring p read neighbouring addresses.  The callers' table is the windowed sinc of resample.py (built in fp64,
 * rounded once); the kernel takes any.  Each output is one fp32 fma chain in ascending i: no atomics, an order that depends on
 * neither the shape nor the batch, so results are bit-reproducible and a row does not depend on the rest of the batch.
 * audio, taps and out are 4-byte aligned; rows start wherever that puts them (16-byte loads where the addresses allow, the same bits
 * either way).  Offsets are 64-bit: B L_out may exceed 2^31.
 * 1 <= up, down <= 640, width >= 0, T <= 1024, L >= 1, 1 <= B <= 65535.  Positive up, down beyond that: NS2_UNAVAILABLE, nothing is
 * launched (ns2_resample_frames_per_block answers 0 for them). */
int ns2_resample(const float* audio, int B, int64_t L, int up, int down, int width, const float* taps, float* out, int64_t L_out,
                 void* stream);

/* ns2_resample of a ragged batch: lens [B] int32 sample counts in device memory, read by the kernel alone and clamped there to [0, L].
 * Utterance b reads zeros at and behind lens[b] (a select: what lies there, NaN included, reaches nothing), so outputs
 * q < ceil(up lens[b] / down) are bit for bit those of ns2_resample on the utterance cut to its length; from there on exact 0 is
 * stored. */
int ns2_resample_lens(const float* audio, int B, int64_t L, int up, int down, int width, const float* taps, float* out, int64_t L_out,
                      const int* lens, void* stream);

/* Host arithmetic, no device: the output frames f (of `up` samples, from `down` input samples each) that one workgroup owns; block j
 * starts at input sample j F down and output sample j F up.  0: the shape is not taken. */
int ns2_resample_frames_per_block(int up, int down, int width);

/* ------------------------------------------------------------------ EnCodec SEANet encoder / decoder pieces (HFENC:81-347)
 * The convolutions themselves are ns2_linear calls on channel-last rows (strided / transposed convolutions as 2-tap
 * convolutions over rows regrouped by the stride); these are the pieces around them.
 * ns2_seanet_prep: fp32 x [B, in_prefix + T, C] (row stride ldx, the first in_prefix rows of every utterance skipped;
 *   + optional add [B, T, C]) -> optional ELU (HFENC:285-347) -> operand
 *   planes [B, prefix + T, ldo] whose `prefix` leading rows per utterance hold the mirrored samples (row -j = row j): EnCodec's
 *   reflect padding of causal convolutions (HFENC:142-175).  im2col_k > 0 (C must be 1, prefix 0): output column j of row n is
 *   x_reflect[n - (k - 1) + j], the k taps of the first convolution as a K = k Linear.
 * ns2_seanet_unpad: dst[b][t][:] = src[b][prefix + t][:]  (drop the prefix rows of a convolution output)
 * ns2_lstm_layer: one nn.LSTM layer (HFENC:253-266; gate order i, f, g, o).  xproj [B*T, 4H] = x W_ih^T + b_ih (a GEMM, row
 *   b*T + t), w_hh [4H, H], b_hh [4H]; state = ns2_lstm_state_floats(B, H) floats of caller scratch (at least 3*B*H: with less
 *   than the full amount the recurrence runs as one launch per step instead of one persistent launch per layer);
 *   out[b*T + t, :H] = h_t (+ resid row). */
int ns2_seanet_prep(const float* x, int ldx, int in_prefix, const float* add, int ldadd, int B, int64_t T, int C, int elu, int prefix,
                    int im2col_k, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
/* ns2_seanet_prep2: one pass over fp32 x [B, in_prefix + T, C] for the two operands EnCodec's residual block (HFENC:268-301) needs
 *   of it -- ELU(x) and x -- each (either may be NULL) into the column window [col0, col0 + cols) of a plane buffer of row stride
 *   ld (logical columns; col0 a multiple of 32, cols >= C a multiple of 4, zero filled past C), rows laid out as ns2_seanet_prep
 *   does (`prefix` mirrored rows per utterance).  Lets x and the hidden activation share one operand, so that
 *   conv2(elu(h)) + shortcut(x) is ONE GEMM over the concatenated K. */
int ns2_seanet_prep2(const float* x, int ldx, int in_prefix, int B, int64_t T, int C, int prefix, uint16_t* elu_hi, uint16_t* elu_lo,
                     int elu_ld, int elu_col0, int elu_cols, uint16_t* raw_hi, uint16_t* raw_lo, int raw_ld, int raw_col0, int raw_cols,
                     int precision, void* stream);
/* ns2_seanet_conv_narrow: the two ends of the SEANet stacks as what they are -- the encoder's first convolution (ci = 1 -> co
 *   channels, HFENC:304-327) and the decoder's last (ci -> co = 1, HFENC:330-358): causal, reflect padded (HFENC:142-175), k = 7,
 *   fp32 on the vector ALUs in one pass over the wide side.  x fp32 [B, in_prefix + T, ci] (row stride ldx), optional ELU on the
 *   input, w [co, ci, k] as nn.Conv1d holds it, out fp32 [B * T, co] (row stride ldo).  Returns NS2_UNAVAILABLE (nothing launched)
 *   for any other shape: the caller takes the GEMM path. */
int ns2_seanet_conv_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int ci, int co, int k, int elu, const float* w,
                           const float* bias, float* out, int64_t ldo, void* stream);
/* ns2_seanet_resblock_narrow: EnCodec's residual block (HFENC:268-301) y = shortcut(x) + conv2(elu(conv1(elu(x)))) -- conv1 k = 3
 *   causal, dilation 1, reflect padded, C -> C / 2; conv2 and the shortcut 1 x 1 -- in ONE fp32 pass on the vector ALUs for the narrow
 *   end of the SEANet stacks (C = 32: the blocks that run at the full sample rate), instead of two operand-plane passes + two GEMMs.
 *   x fp32 [B, in_prefix + T, C] (row stride ldx) -> out fp32 [B * T, C] (row stride ldo).  Weights pre-arranged in consumption order:
 *   w1p [3][C][C / 2] = conv1.weight[h][c][t] at (t, c, h); w2p [C / 2][C] = conv2.weight[c][h] at (h, c); wsp [C][C] =
 *   shortcut.weight[o][c] at (c, o); b1 = conv1.bias; b2s = conv2.bias + shortcut.bias.  Returns NS2_UNAVAILABLE (nothing launched)
 *   for any other shape: the caller takes the GEMM path. */
int ns2_seanet_resblock_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int C, const float* w1p, const float* b1,
                               const float* w2p, const float* wsp, const float* b2s, float* out, int64_t ldo, void* stream);
int ns2_seanet_unpad(const float* src, int64_t ld_src, int prefix, float* dst, int64_t ld_dst, int B, int64_t T, int C, void* stream);
int64_t ns2_lstm_state_floats(int B, int H);
int ns2_lstm_layer(const float* xproj, int64_t ld_x, const float* w_hh, const float* b_hh, float* state, int64_t state_floats,
                   const float* resid, int64_t ld_r, float* out, int64_t ld_o, int B, int64_t T, int H, void* stream);

/* ns2_lstm2: BOTH layers of EnCodec's 2-layer nn.LSTM (HFENC:253-266, H = 512) in one launch, layer 2 running one frame behind
 *   layer 1 on its own workgroups and layer 1 forming layer 2's input projections (no GEMM between the layers).  xproj1 [B*T, 4H] =
 *   x W_ih1^T + b_ih1; w_hh1 / w_ih2 / w_hh2 [4H, H]; b_* [4H]; state = ns2_lstm2_state_floats() floats of caller scratch;
 *   out[b*T + t, :H] = h2_t (+ resid row).  Returns NS2_UNAVAILABLE -- nothing launched -- when the device cannot hold all the
 *   workgroups at once, B > 32, or NS2_LSTM_FUSED=0 / NS2_LSTM_PERSISTENT=0: call ns2_lstm_layer per layer instead. */
int64_t ns2_lstm2_state_floats(void);
int ns2_lstm2(const float* xproj1, int64_t ld_x, const float* w_hh1, const float* b_hh1, const float* w_ih2, const float* b_ih2,
              const float* w_hh2, const float* b_hh2, float* state, int64_t state_floats, const float* resid, int64_t ld_r, float* out,
              int64_t ld_o, int B, int64_t T, void* stream);

/* The one-launch LSTM recurrences synchronise their workgroups frame by frame through tagged values in global memory, which needs
 * every workgroup resident.  The launchers take that path only when the occupancy query says the device can hold them; should a
 * wait still time out (CU masking, a device saturated by other processes) the kernel gives up -- its output is then incomplete --
 * and counts the launch here instead of trapping.  Synchronises; call it after a codec run.  NS2_LSTM_PERSISTENT=0 forces the
 * per-step kernel. */
int ns2_lstm_abort_count(int reset, int64_t* count);
/* test hook: set that counter, as if n launches had given up (exercises the caller's fallback from the one-launch recurrences) */
int ns2_debug_lstm_inject_abort(int n);

/* EnCodec RVQ (HFENC:364-369, 424-447; reference call sites NS2:1445, NS2:1611, NS2:1496).
 * cb_norm: [Q, C] scratch filled by ns2_rvq_prepare (once per codebook set). codes: [M, Q] int64; emb/residual [M, D] or null */
int ns2_rvq_prepare(const float* codebooks, float* cb_norm, int Q, int C, int D, void* stream);
int ns2_rvq_encode(const float* x, const float* codebooks, const float* cb_norm, int64_t* codes, float* emb,
                   float* residual, int* near_tie_count, int M, int Q, int C, int D, float tie_eps, void* stream);
int ns2_rvq_decode(const int64_t* codes, const float* codebooks, float* emb, int M, int Q, int C, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NS2HIP_AUDIO_H */
