/* The pitch extractor of libns2hip (csrc/pitch.hip, pitch.py).  Part of the C ABI: listed in _lib.HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).  Status codes and ns2_last_error are those of ns2hip.h. */
#ifndef NS2HIP_PITCH_H
#define NS2HIP_PITCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
