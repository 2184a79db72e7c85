// The YIN pitch estimator (pitch.py; de Cheveigne & Kawahara, JASA 2002, steps 1-5; include/ns2hip_audio.h states the formula) in
// one launch: framing, the difference function, its cumulative-mean normalisation, the threshold search, the descent to the local
// minimum and the parabolic interpolation.  fp32 throughout, no atomics, every sum in a fixed order.
//
// One block owns F consecutive frames of one utterance (F <= 8, chosen by the host so that the lanes of the difference function
// are full: 3 at the defaults).  Each frame's span of S = 3 tau_max samples is staged in LDS, zero outside the utterance, at a
// 16-byte aligned row of its own (frames overlap by S - hop samples, but a shared span would put frame f at f * hop floats, which
// is aligned only when hop % 4 == 0; the re-reads come from L2).
//   - difference function: a lane owns the PY_R = 4 lags 4g .. 4g + 3 of one frame and walks j four at a time.  Per step it reads
//     x[j .. j + 3] (one 16-byte read, the same address for every lane of the frame: a broadcast) and x[j + 4g .. j + 4g + 7]
//     (two aligned 16-byte reads, consecutive lanes at consecutive 16 bytes: conflict-free), and does 16 subtract + fma (the
//     compiler packs them in pairs).  A lag's sum is kept as four partial sums over j = q mod 4, each in ascending j, folded as
//     (p0 + p1) + (p2 + p3).  Lag 0 is computed like any other (it is 0) so that the lags of a lane start at a multiple of four.
//     Eight lags per lane read less per subtract-fma pair but fill the lanes worse (43 lanes a frame against 85): measured
//     1.77 ms against 1.64 ms at 32 x 327 680 samples (PY_R = 8; profiles/pitch_lags_per_lane_ab.txt);
//   - the rest is one wave per frame, 64 lags at a time: an inclusive Kogge-Stone scan by __shfl_up with the total of the chunks
//     before it carried in (a fixed shape), d'(tau) back into the lag's LDS slot, then two ascending ballot searches -- the
//     first lag below the threshold, and from there the first lag whose successor is not lower.
// A frame's value depends on its own samples alone, so an utterance's row is bit-identical alone or in any batch.
// LENS (ns2_pitch_yin_lens, include/ns2hip_audio.h): utterance b ends at its own sample_lens[b], clamped into [1, L]: the
// staging reads zeros from there on, frames from T_b = 1 + len / hop on are stored as 0 (unvoiced), and a block that holds only such
// frames returns after storing them.  The instantiation without LENS is the kernel as it was.
// This translation unit converts nothing to half: it includes no ns2_common.h and owns no range counter.
#include <hip/hip_runtime.h>

#include "ns2_host.h"

namespace ns2 {
namespace {

constexpr int PY_THREADS = 256;
constexpr int PY_R = 4;               // lags per lane of the difference function (a multiple of 4 that divides 64)
constexpr int PY_FRAMES_MAX = 8;
constexpr int PY_LDS_MAX = 64 * 1024;

// LDS image: smp [F][SP] | dd [F][DP].  SP: the span plus what the lags past tau_max of the last lane over-read (zeros);
// DP: the lags 0 .. tau_max rounded up to whole 64-lag chunks
inline int py_sp(int tau_max) { return (3 * tau_max + PY_R + 3) & ~3; }
inline int py_dp(int tau_max) { return (tau_max + 1 + 63) / 64 * 64; }
inline int py_groups(int tau_max) { return (tau_max + PY_R) / PY_R; }  // lanes per frame: lags 0 .. tau_max, PY_R each

// grid (ceil(T / F), B), PY_THREADS threads, dynamic LDS 4 F (SP + DP) bytes
template <bool LENS>
__global__ __launch_bounds__(PY_THREADS) void pitch_yin_kernel(const float* __restrict__ audio, long L, long T, int hop, int F, int G,
                                                               int SP, int DP, int tau_min, int tau_max, float fs, float thr,
                                                               float* __restrict__ f0, const int* __restrict__ sample_lens) {
  extern __shared__ float4 py_sm[];
  float* smp = reinterpret_cast<float*>(py_sm);
  float* dd = smp + F * SP;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long b = blockIdx.y;
  const long fr0 = (long)blockIdx.x * F;
  const int nfo = (int)min((long)F, T - fr0);                     // frames this block stores
  int nf = nfo;                                                   // ... of which it computes the first nf; the rest are 0
  long Le = L;                                                    // where the utterance ends
  if constexpr (LENS) {
    Le = min(max((long)sample_lens[b], 1L), L);
    nf = (int)min(max(1 + Le / hop - fr0, 0L), (long)nfo);
    if (nf == 0) {                                                // block-uniform, before any barrier
      if (t < nfo) f0[b * T + fr0 + t] = 0.f;
      return;
    }
  }
  const int S = 3 * tau_max, W = 2 * tau_max, W4 = W & ~3;
  const float* x = audio + b * L;

  for (int i = t; i < nf * SP; i += PY_THREADS) {
    const int f = i / SP, idx = i - f * SP;
    const long src = (fr0 + f) * hop - S / 2 + idx;
    smp[i] = (idx < S && src >= 0 && src < Le) ? x[src] : 0.f;
  }
  __syncthreads();

  // d(tau) = sum_j (x[j] - x[j + tau])^2, j = 0 .. W - 1
  for (int it = t; it < nf * G; it += PY_THREADS) {
    const int f = it / G, g = it - f * G;
    const float* xs = smp + f * SP;
    const float* xl = xs + PY_R * g;
    float acc[PY_R][4];
#pragma unroll
    for (int r = 0; r < PY_R; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
#pragma unroll 2
    for (int j = 0; j < W4; j += 4) {
      const float4 a4 = *reinterpret_cast<const float4*>(xs + j);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w};
      float w[PY_R + 4];
#pragma unroll
      for (int i = 0; i < PY_R + 4; i += 4) {
        const float4 u = *reinterpret_cast<const float4*>(xl + j + i);
        w[i] = u.x; w[i + 1] = u.y; w[i + 2] = u.z; w[i + 3] = u.w;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < PY_R; ++r) {
          const float e = a[q] - w[q + r];
          acc[r][q] = fmaf(e, e, acc[r][q]);
        }
    }
    if (W4 < W) {                                                 // W = 2 tau_max is even: two samples remain
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float a = xs[W4 + q];
#pragma unroll
        for (int r = 0; r < PY_R; ++r) {
          const float e = a - xl[W4 + q + r];
          acc[r][q] = fmaf(e, e, acc[r][q]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < PY_R; r += 4) {
      float4 d;
      d.x = (acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3]);
      d.y = (acc[r + 1][0] + acc[r + 1][1]) + (acc[r + 1][2] + acc[r + 1][3]);
      d.z = (acc[r + 2][0] + acc[r + 2][1]) + (acc[r + 2][2] + acc[r + 2][3]);
      d.w = (acc[r + 3][0] + acc[r + 3][1]) + (acc[r + 3][2] + acc[r + 3][3]);
      *reinterpret_cast<float4*>(dd + f * DP + PY_R * g + r) = d;
    }
  }
  __syncthreads();

  const int NC = DP / 64;
  for (int fb = 0; fb < F; fb += PY_THREADS / 64) {               // block-uniform trips: the barrier below is reached by every wave
    const int f = fb + wave;
    const bool active = f < nf;
    float* dp = dd + (active ? f : 0) * DP;
    if (active) {                                                 // c(tau) = sum_{k <= tau} d(k);  d'(tau) = d tau / c, 1 where c = 0
      float carry = 0.f;
      for (int k = 0; k < NC; ++k) {
        const int tau = 64 * k + lane;
        const float d = (tau >= 1 && tau <= tau_max) ? dp[tau] : 0.f;
        float s = d;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float up = __shfl_up(s, o, 64);
          if (lane >= o) s += up;
        }
        const float c = carry + s;
        carry = __shfl(c, 63, 64);
        if (tau <= tau_max) dp[tau] = c > 0.f ? d * (float)tau / c : 1.f;
      }
    }
    __syncthreads();
    if (active) {
      int first = -1;                                             // the first lag in [tau_min, tau_max] with d' < thr
      for (int k = tau_min >> 6; k < NC && first < 0; ++k) {
        const int tau = 64 * k + lane;
        const bool p = tau >= tau_min && tau <= tau_max && dp[min(tau, tau_max)] < thr;
        const unsigned long long m = __ballot(p);
        if (m) first = 64 * k + __ffsll((long long)m) - 1;
      }
      float out = 0.f;
      if (first >= 0) {
        int stop = -1;                                            // from there, the first lag whose successor is not lower
        for (int k = first >> 6; k < NC && stop < 0; ++k) {
          const int tau = 64 * k + lane;
          const bool p = tau >= first && (tau >= tau_max || !(dp[min(tau + 1, tau_max)] < dp[min(tau, tau_max)]));
          const unsigned long long m = __ballot(p);
          if (m) stop = 64 * k + __ffsll((long long)m) - 1;
        }
        stop = min(max(stop, first), tau_max);                    // (always found: the lane of tau_max votes)
        const float y0 = dp[stop - 1], y1 = dp[stop];
        float delta = 0.f;
        if (stop + 1 <= tau_max) {
          const float y2 = dp[stop + 1];
          const float den = y0 - 2.f * y1 + y2;
          if (den > 0.f) delta = fminf(fmaxf(0.5f * (y0 - y2) / den, -1.f), 1.f);
        }
        out = fs / ((float)stop + delta);
      }
      if (lane == 0) f0[b * T + fr0 + f] = out;
    }
    if constexpr (LENS) {
      if (!active && f < nfo && lane == 0) f0[b * T + fr0 + f] = 0.f;
    }
  }
}

}  // namespace

// sample_lens null: the call without lengths
hipError_t launch_pitch_yin(const float* audio, int B, long L, long T, int sample_rate, int hop, int tau_min, int tau_max, float threshold,
                            float* f0, hipStream_t s, const int* sample_lens) {
  const int G = py_groups(tau_max), SP = py_sp(tau_max), DP = py_dp(tau_max);
  const size_t per_frame = 4 * (size_t)(SP + DP);
  int F = 1;
  long best_n = 0, best_d = 1;                                    // lane use of the difference function: F G / (256 ceil(F G / 256))
  for (int f = 1; f <= PY_FRAMES_MAX && f * per_frame <= (size_t)PY_LDS_MAX; ++f) {
    const long n = (long)f * G, d = (n + PY_THREADS - 1) / PY_THREADS * PY_THREADS;
    if (n * best_d > best_n * d) { F = f; best_n = n; best_d = d; }
  }
  const dim3 grid((unsigned)((T + F - 1) / F), (unsigned)B);
  if (sample_lens)
    hipLaunchKernelGGL(pitch_yin_kernel<true>, grid, dim3(PY_THREADS), F * per_frame, s, audio, L, T, hop, F, G, SP, DP, tau_min, tau_max,
                       (float)sample_rate, threshold, f0, sample_lens);
  else
    hipLaunchKernelGGL(pitch_yin_kernel<false>, grid, dim3(PY_THREADS), F * per_frame, s, audio, L, T, hop, F, G, SP, DP, tau_min, tau_max,
                       (float)sample_rate, threshold, f0, sample_lens);
  return hipGetLastError();
}

}  // namespace ns2
