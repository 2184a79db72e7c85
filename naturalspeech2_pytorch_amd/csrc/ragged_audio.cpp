// extern "C" surface of include/ns2hip_ragged_audio.h: per-utterance lengths in the pitch extractor (pitch.hip) and in the RVQ
// cross-entropy term (rvq_ce.hip).  ns2_audio_to_mel_lens sits next to ns2_audio_to_mel in audio_to_mel.hip, which owns the checks and the
// LDS sizing both share.  The lengths are device memory: nothing here reads them.
#include <hip/hip_runtime.h>

#include "../../include/ns2hip_ragged_audio.h"
#include "ns2_host.h"

using namespace ns2;

extern "C" int ns2_pitch_yin_lens(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max,
                                  float threshold, float* f0, const int* sample_lens, void* stream) {
  ARGCHK(audio && f0, "ns2_pitch_yin_lens: null pointer");
  ARGCHK(sample_lens, "ns2_pitch_yin_lens: sample_lens is null (ns2_pitch_yin is the call without lengths)");
  ARGCHK(B >= 1 && B <= 65535, "ns2_pitch_yin_lens: B must be in [1, 65535]");
  ARGCHK(L >= 1, "ns2_pitch_yin_lens: L must be at least 1");
  ARGCHK(sample_rate >= 1 && hop_length >= 1, "ns2_pitch_yin_lens: sample_rate and hop_length must be at least 1");
  ARGCHK(tau_min >= 2 && tau_min < tau_max && tau_max <= PITCH_TAU_MAX, "ns2_pitch_yin_lens: the lags must satisfy 2 <= tau_min < tau_max <= 1024");
  ARGCHK(threshold == threshold, "ns2_pitch_yin_lens: threshold is NaN");
  const int64_t T = 1 + L / hop_length;
  ARGCHK(T <= 0x7fffffffLL, "ns2_pitch_yin_lens: too many frames");
  HIPRET(launch_pitch_yin(audio, B, (long)L, (long)T, sample_rate, hop_length, tau_min, tau_max, threshold, f0, (hipStream_t)stream, sample_lens));
  return NS2_OK;
}

extern "C" int ns2_rvq_ce_lens(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss,
                               float* loss, float* quantized_out, float* grad, int B, int n, const int* row_lens, int Q, int C, int D,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(x && codebooks && cb_norm && indices && row_loss && loss, "ns2_rvq_ce_lens: null pointer");
  ARGCHK(row_lens, "ns2_rvq_ce_lens: row_lens is null (ns2_rvq_ce is the call without lengths)");
  ARGCHK(B > 0 && n > 0 && Q > 0 && C > 0, "ns2_rvq_ce_lens: B, n, Q and C must be positive");
  ARGCHK((int64_t)B * n <= 0x7fffffffLL, "ns2_rvq_ce_lens: B * n must fit an int");
  ARGCHK(D == 128 && C % 64 == 0, "ns2_rvq_ce_lens: needs codebook_dim 128 and codebook_size % 64 == 0 (EnCodec: 128 / 1024)");
  const int M = B * n;
  ARGCHK(!quantized_out || (workspace && workspace_bytes >= ns2_rvq_ce_workspace_bytes(M, Q, 1)),
         "ns2_rvq_ce_lens: quantized_out needs a workspace (ns2_rvq_ce_workspace_bytes)");
  RvqCeLensArgs a;
  a.x = x; a.codebooks = codebooks; a.cb_norm = cb_norm; a.targets = indices; a.row_loss = row_loss; a.loss = loss;
  a.nearest = quantized_out ? (int64_t*)workspace : nullptr; a.quantized_out = quantized_out; a.grad = grad;
  a.M = M; a.Q = Q; a.C = C; a.D = D;
  a.row_lens = row_lens; a.B = B; a.n = n;
  HIPRET(launch_rvq_ce_lens(a, (hipStream_t)stream));
  return NS2_OK;
}
