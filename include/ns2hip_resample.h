/* The sample-rate converter of libns2hip (csrc/resample.hip, resample.py).  Part of the C ABI: listed in _lib.EXTRA_HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).  Status codes and ns2_last_error are those of ns2hip.h. */
#ifndef NS2HIP_RESAMPLE_H
#define NS2HIP_RESAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
