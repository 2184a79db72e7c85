// The sample-rate converter (resample.py; include/ns2hip_audio.h states the formula): polyphase rational resampling by up / down in
// one launch.  out[f up + p] = sum_i k[p][i] x[f down + i - w], i = 0 .. T - 1, T = 2 w + down, one fp32 fma chain per output in
// ascending i.  fp32 throughout, no atomics, no sum whose order depends on the shape or the batch.
//
// One block owns F = RS_R G consecutive output frames f of one utterance (G chosen by the host: resample_groups).
//   - staging: the F down + 2 w input samples the frames read go to LDS, zero outside the utterance.  The LDS image starts `shift`
//     (0 .. 3) samples before the span so that slot 0 is a 16-byte aligned global address whatever the row's own alignment: a group of
//     four slots inside the utterance is one 16-byte load, a group that straddles an end is four guarded 4-byte loads -- the same
//     values either way;
//   - a lane owns one (g, p) and the RS_R frames g, g + G, g + 2 G, g + 3 G at that phase: per tap one global read of the transposed
//     table taps[i up + p] (neighbouring lanes, neighbouring p: coalesced; the table, up to 103 KB at 160 / 147, lives in L2), RS_R LDS
//     reads (a wave's lanes share g or step by `down`) and RS_R fmas.  The frames of a lane are G apart, not adjacent, so that the
//     stores of one r run over consecutive lanes: out[r G up + item].
// An output depends on its own T samples alone, so an utterance's row is bit-identical alone or in any batch.
// LENS (ns2_resample_lens): utterance b ends at lens[b], clamped into [0, L]: the staging reads nothing from there on (zeros: a
// select, not a product), outputs from ceil(up lens[b] / down) on are stored as 0, and a block that holds only such outputs returns
// after storing them.  The instantiation without LENS has none of it.
// This translation unit converts nothing to half: it includes no ns2_common.h and owns no range counter.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ns2_host.h"

namespace ns2 {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_R = 4;                  // frames per lane
constexpr int RS_MAX_RATE = 640;         // up, down
constexpr int RS_MAX_TAPS = 1024;        // T
constexpr int RS_MAX_ITEMS = 2048;       // (g, p) pairs per block: at most 8 per lane
constexpr int RS_LDS_SOFT = 32 * 1024;   // what the choice of G keeps to (five blocks a CU); one group always fits: 4 (4 * 640 + 1024 + 6)

// bytes of the LDS image of F frames: shift (<= 3) + (F - 1) down + T slots, in whole groups of four
inline long rs_lds_bytes(int F, int down, int T) { return 4L * ((3 + (long)(F - 1) * down + T + 3) & ~3L); }

// G, the frame groups per block (F = RS_R G): of those whose image fits RS_LDS_SOFT and whose G up items stay within RS_MAX_ITEMS, the
// one that fills the lanes best (G up / (256 ceil(G up / 256))), the largest of equals.  0: the shape is not taken.
int resample_groups(int up, int down, int width) {
  if (up < 1 || down < 1 || width < 0 || up > RS_MAX_RATE || down > RS_MAX_RATE) return 0;
  const long T = 2L * width + down;
  if (T > RS_MAX_TAPS) return 0;
  int G = 1;
  long best_n = 0, best_d = 1;
  for (int g = 1; g == 1 || ((long)g * up <= RS_MAX_ITEMS && rs_lds_bytes(RS_R * g, down, (int)T) <= RS_LDS_SOFT); ++g) {
    const long n = (long)g * up, d = (n + RS_THREADS - 1) / RS_THREADS * RS_THREADS;
    if (n * best_d >= best_n * d) { G = g; best_n = n; best_d = d; }
  }
  return G;
}

// grid (ceil(ceil(L_out / up) / F), B), RS_THREADS threads, dynamic LDS rs_lds_bytes(F, down, T)
template <bool LENS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ audio, long L, int up, int down, int w, int T,
                                                              int G, const float* __restrict__ taps, float* __restrict__ out, long L_out,
                                                              const int* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) float rs_sm[];
  const int t = threadIdx.x;
  const long b = blockIdx.y;
  const int F = RS_R * G;
  const long f0 = (long)blockIdx.x * F;
  const long q0 = f0 * up;                                          // the block's first output
  const long nq = min((long)F * up, L_out - q0);                   // outputs this block stores (>= 1 by the grid)
  long Le = L, nc = nq;                                             // where the utterance ends; the first nc outputs are computed
  if constexpr (LENS) {
    Le = min(max((long)lens[b], 0L), L);
    nc = min(max((Le * up + down - 1) / down - q0, 0L), nq);
  }
  float* o = out + b * L_out + q0;
  if constexpr (LENS) {
    if (nc == 0) {                                                  // block-uniform, before any barrier
      for (long j = t; j < nq; j += RS_THREADS) o[j] = 0.f;
      return;
    }
  }
  const float* x = audio + b * L;
  const long s0 = f0 * down - w;                                    // the first sample the block reads (may be negative)
  const int shift = (int)(((long)(reinterpret_cast<uintptr_t>(x) >> 2) + s0) & 3);
  const long g0 = s0 - shift;                                       // the sample of slot 0: x + g0 is 16-byte aligned
  const int ngrp = (shift + (F - 1) * down + T + 3) >> 2;
  for (int v = t; v < ngrp; v += RS_THREADS) {
    const long src = g0 + 4L * v;
    float4 u;
    if (src >= 0 && src + 4 <= Le) {
      u = *reinterpret_cast<const float4*>(x + src);
    } else {
      u.x = (src >= 0 && src < Le) ? x[src] : 0.f;
      u.y = (src + 1 >= 0 && src + 1 < Le) ? x[src + 1] : 0.f;
      u.z = (src + 2 >= 0 && src + 2 < Le) ? x[src + 2] : 0.f;
      u.w = (src + 3 >= 0 && src + 3 < Le) ? x[src + 3] : 0.f;
    }
    reinterpret_cast<float4*>(rs_sm)[v] = u;
  }
  __syncthreads();

  const float* xs = rs_sm + shift;
  const int items = G * up, gstep = G * down;
  for (int it = t; it < items; it += RS_THREADS) {
    const int g = it / up, p = it - g * up;
    const float* kp = taps + p;
    const float* xf = xs + g * down;
    float acc[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int i = 0; i < T; ++i) {
      const float k = kp[i * up];
#pragma unroll
      for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(k, xf[r * gstep + i], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {                                // frame r G + g, phase p: output r items + it of the block
      const long j = (long)r * items + it;
      if (j < nc) o[j] = acc[r];
      else if (LENS && j < nq) o[j] = 0.f;
    }
  }
}

int resample_entry(const char* name, const float* audio, int B, int64_t L, int up, int down, int width, const float* taps, float* out,
                   int64_t L_out, const int* lens, bool with_lens, void* stream) {
  ARGCHK(audio && taps && out, "ns2_resample: null pointer");
  ARGCHK(!with_lens || lens, "ns2_resample_lens: lens is null (ns2_resample is the call without lengths)");
  ARGCHK(((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(taps) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
         "ns2_resample: audio, taps and out must be 4-byte aligned");
  ARGCHK(B >= 1 && B <= 65535, "ns2_resample: B must be in [1, 65535]");
  ARGCHK(L >= 1, "ns2_resample: L must be at least 1");
  ARGCHK(up >= 1 && down >= 1 && width >= 0, "ns2_resample: up and down must be at least 1, width at least 0");
  ARGCHK(L <= INT64_MAX / RS_MAX_RATE / 2, "ns2_resample: L is too large");
  const int G = resample_groups(up, down, width);
  if (G == 0) {
    set_error("%s: takes up, down <= %d and 2 width + down <= %d taps, got %d / %d, width %d", name, RS_MAX_RATE, RS_MAX_TAPS, up, down, width);
    return NS2_UNAVAILABLE;
  }
  ARGCHK(L_out == (L * up + down - 1) / down, "ns2_resample: L_out must be ceil(up L / down)");
  const int T = 2 * width + down, F = RS_R * G;
  const int64_t nblk = ((L_out + up - 1) / up + F - 1) / F;
  ARGCHK(nblk <= 0x7fffffffLL, "ns2_resample: too many frames");
  const dim3 grid((unsigned)nblk, (unsigned)B);
  const size_t lds = (size_t)rs_lds_bytes(F, down, T);
  hipStream_t s = (hipStream_t)stream;
  if (with_lens)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), lds, s, audio, (long)L, up, down, width, T, G, taps, out, (long)L_out, lens);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), lds, s, audio, (long)L, up, down, width, T, G, taps, out, (long)L_out, lens);
  HIPRET(hipGetLastError());
  return NS2_OK;
}

}  // namespace
}  // namespace ns2

using namespace ns2;

extern "C" int ns2_resample(const float* audio, int B, int64_t L, int up, int down, int width, const float* taps, float* out, int64_t L_out,
                            void* stream) {
  return resample_entry("ns2_resample", audio, B, L, up, down, width, taps, out, L_out, nullptr, false, stream);
}

extern "C" int ns2_resample_lens(const float* audio, int B, int64_t L, int up, int down, int width, const float* taps, float* out,
                                 int64_t L_out, const int* lens, void* stream) {
  return resample_entry("ns2_resample_lens", audio, B, L, up, down, width, taps, out, L_out, lens, true, stream);
}

extern "C" int ns2_resample_frames_per_block(int up, int down, int width) { return RS_R * resample_groups(up, down, width); }
