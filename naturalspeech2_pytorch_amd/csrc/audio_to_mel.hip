// AudioToMel (audio_to_mel.py; the reference's AudioToMel, NS2:181-224) in one pass over the audio: reflect-padded framing,
// the Hann window, a real n_fft-point FFT, power, the triangular mel projection and (optionally) the dB log, per frame.
//
// One block owns `fpb` consecutive frames of one utterance.  It stages their sample span into LDS once, with the reflect
// padding of torch.stft(center=True) applied by index mapping, so every sample is read from HBM once rather than n_fft / hop
// times.  The frames then go through the FFT FB = 2048 / N at a time (N = n_fft / 2), 8 complex points per thread:
//   - the real FFT is an N-point complex FFT of z[m] = x[2m] + i x[2m+1] plus the split post-pass
//     X[k] = (Z[k] + conj Z[N-k]) / 2 - i w^k (Z[k] - conj Z[N-k]) / 2;
//   - the complex FFT is a self-sorting (Stockham) decimation in time: radix-4 stages, one radix-2 stage last when log2 N is
//     odd, each butterfly in registers, one LDS exchange per stage (rows padded by one float2 per 32 against the power-of-two
//     strides).  The first stage reads the windowed samples straight from the staged span;
//   - twiddles and the window are tables the host computed in fp64 and rounded to fp32 (no device sin / cos);
//   - power |X|^2 goes to LDS; each mel row sums its compact filter (first bin, weights) in ascending bin order, then
//     10 log10(max(mel, 1e-10)), the log10 taken in fp64 and rounded to fp32;
//   - results are staged as [mel][frame] in LDS so that each store writes a contiguous run of frames of one mel row.
// No atomics: a frame's values depend on its samples alone, so an utterance's output is bit-identical whatever batch it is in.
//
// LENS (ns2_audio_to_mel_lens, include/ns2hip_audio.h): utterance b ends at its own sample_lens[b], clamped into
// [n_fft / 2 + 1, L].  The reflection is taken about ITS last sample -- the one index map at the staging of smp -- so frames
// t < T_b = 1 + len / hop are those of the utterance alone; frames from T_b on are stored as 0.0f, and a block that holds only such
// frames stages nothing and runs no FFT.  The instantiation without LENS is the kernel as it was.
#include <hip/hip_runtime.h>

#include <climits>

#include "ns2_common.h"
#include "ns2_host.h"

namespace ns2 {

constexpr int AM_THREADS = 256;
constexpr int AM_POINTS = 2048;      // complex points in flight per block: 8 per thread
constexpr int AM_FPB = 32;           // frames per block, halved while the LDS image exceeds AM_LDS_SOFT
constexpr int AM_LDS_SOFT = 80 * 1024;
constexpr int AM_LDS_MAX = 160 * 1024;

NS2_DEVINL int am_pad(int a) { return a + (a >> 5); }           // one float2 of padding per 32

NS2_DEVINL float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

NS2_DEVINL void dft4(float2* v) {                                 // forward 4-point DFT, e^{-2 pi i / 4} = -i
  const float2 s02 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), d02 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
  const float2 s13 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), d13 = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
  v[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
  v[2] = make_float2(s02.x - s13.x, s02.y - s13.y);
  v[1] = make_float2(d02.x + d13.y, d02.y - d13.x);              // d02 - i d13
  v[3] = make_float2(d02.x - d13.y, d02.y + d13.x);              // d02 + i d13
}

// host and device agree on this LDS image (floats unless noted):
//   tw [n_fft] float2 | buf [FB][NP] float2 | win [n_fft] | pw [FB][n_bins] | os [n_mels][fpb + 1] | w [n_w] | meta [3 n_mels] int
//   | smp [(fpb - 1) hop + n_fft]
inline size_t am_lds_bytes(int N, int fpb, int hop, int n_mels, int n_bins, int n_w) {
  const int nfft = 2 * N, fb = AM_POINTS / N, np = N + N / 32;
  return 8 * (size_t)nfft + 8 * (size_t)fb * np + 4 * (size_t)nfft + 4 * (size_t)fb * n_bins + 4 * (size_t)n_mels * (fpb + 1) +
         4 * (size_t)n_w + 12 * (size_t)n_mels + 4 * ((size_t)(fpb - 1) * hop + nfft);
}

// grid (ceil(T / fpb), B), AM_THREADS threads, dynamic LDS am_lds_bytes
template <int N, bool LENS>
__global__ __launch_bounds__(AM_THREADS) void audio_to_mel_kernel(const float* __restrict__ audio, long L, long T, int hop, int fpb,
                                                                  const float* __restrict__ window, const float2* __restrict__ twiddle,
                                                                  const int* __restrict__ fb_meta, const float* __restrict__ fb_w,
                                                                  int n_w, int n_mels, int n_bins, int log_db, float* __restrict__ out,
                                                                  const int* __restrict__ sample_lens) {
  constexpr int NFFT = 2 * N, FB = AM_POINTS / N, NP = N + N / 32, Q = N / 4;
  extern __shared__ float2 am_sm[];
  float2* tw = am_sm;
  float2* buf = tw + NFFT;
  float* win = reinterpret_cast<float*>(buf + FB * NP);
  float* pw = win + NFFT;
  float* os = pw + FB * n_bins;
  float* wts = os + n_mels * (fpb + 1);
  int* meta = reinterpret_cast<int*>(wts + n_w);                // start [n_mels] | len [n_mels] | offset into w [n_mels]
  float* smp = reinterpret_cast<float*>(meta + 3 * n_mels);

  const int t = threadIdx.x;
  const long b = blockIdx.y;
  const long f0 = (long)blockIdx.x * fpb;
  const int nfo = (int)min((long)fpb, T - f0);                  // frames this block stores
  int nf = nfo;                                                 // ... of which it computes the first nf; the rest are 0
  long Le = L;                                                  // where the utterance ends: the reflection's mirror
  if constexpr (LENS) {
    Le = min(max((long)sample_lens[b], (long)N + 1), L);
    nf = (int)min(max(1 + Le / hop - f0, 0L), (long)nfo);
    if (nf == 0) {                                              // block-uniform: nothing staged, no FFT, no barrier passed
      for (int i = t; i < n_mels * fpb; i += AM_THREADS) {
        const int m = i / fpb, f = i % fpb;
        if (f < nfo) out[(b * n_mels + m) * T + f0 + f] = 0.f;
      }
      return;
    }
  }
  const float* x = audio + b * L;
  for (int i = t; i < NFFT; i += AM_THREADS) {
    tw[i] = twiddle[i];
    win[i] = window[i];
  }
  for (int i = t; i < n_w; i += AM_THREADS) wts[i] = fb_w[i];
  for (int i = t; i < 3 * n_mels; i += AM_THREADS) meta[i] = fb_meta[i];
  const int span = (fpb - 1) * hop + NFFT, valid = (nf - 1) * hop + NFFT;
  const long s0 = f0 * hop - N;                                 // sample index of smp[0] (center=True pads n_fft / 2)
  for (int i = t; i < span; i += AM_THREADS) {
    float v = 0.f;
    if (i < valid) {
      long s = s0 + i;
      s = s < 0 ? -s : (s >= Le ? 2 * (Le - 1) - s : s);      // reflect; Le > n_fft / 2 keeps one reflection in range
      v = x[s];
    }
    smp[i] = v;
  }
  __syncthreads();

  for (int fb0 = 0; fb0 < nf; fb0 += FB) {
    float2 v[2][4];
    // radix-4 stage at Ns = 1 (unit twiddles), straight from the windowed samples
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int g = t + q * AM_THREADS, f = g / Q, j = g % Q;
      const float* s = smp + (fb0 + f) * hop;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 2 * (j + r * Q);
        v[q][r] = make_float2(win[m] * s[m], win[m + 1] * s[m + 1]);
      }
      dft4(v[q]);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int g = t + q * AM_THREADS, f = g / Q, j = g % Q;
#pragma unroll
      for (int r = 0; r < 4; ++r) buf[f * NP + am_pad(4 * j + r)] = v[q][r];
    }
    __syncthreads();
#pragma unroll
    for (int Ns = 4; Ns * 4 <= N; Ns *= 4) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int g = t + q * AM_THREADS, f = g / Q, j = g % Q, k = j % Ns;
        v[q][0] = buf[f * NP + am_pad(j)];
#pragma unroll
        for (int r = 1; r < 4; ++r) v[q][r] = cmul(buf[f * NP + am_pad(j + r * Q)], tw[2 * r * k * (N / (4 * Ns))]);
        dft4(v[q]);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int g = t + q * AM_THREADS, f = g / Q, j = g % Q, k = j % Ns, d = (j / Ns) * Ns * 4 + k;
#pragma unroll
        for (int r = 0; r < 4; ++r) buf[f * NP + am_pad(d + r * Ns)] = v[q][r];
      }
      __syncthreads();
    }
    if constexpr ((N & 0x55555555) == 0) {                      // log2 N odd: a radix-2 stage at Ns = N / 2
      float2 a[4], c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int g = t + q * AM_THREADS, f = g / (N / 2), j = g % (N / 2);
        a[q] = buf[f * NP + am_pad(j)];
        c[q] = cmul(buf[f * NP + am_pad(j + N / 2)], tw[2 * j]);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int g = t + q * AM_THREADS, f = g / (N / 2), j = g % (N / 2);
        buf[f * NP + am_pad(j)] = make_float2(a[q].x + c[q].x, a[q].y + c[q].y);
        buf[f * NP + am_pad(j + N / 2)] = make_float2(a[q].x - c[q].x, a[q].y - c[q].y);
      }
      __syncthreads();
    }
    // split post-pass and power, bins [0, n_bins)
    for (int i = t; i < FB * n_bins; i += AM_THREADS) {
      const int f = i / n_bins, k = i % n_bins;
      const float2* Z = buf + f * NP;
      float p;
      if (k == 0 || k == N) {
        const float2 z0 = Z[0];
        const float re = k == 0 ? z0.x + z0.y : z0.x - z0.y;
        p = re * re;
      } else {
        const float2 a = Z[am_pad(k)], c = Z[am_pad(N - k)];
        const float2 e = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));     // (Z[k] + conj Z[N-k]) / 2
        const float2 o = make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x));    // -i (Z[k] - conj Z[N-k]) / 2
        const float2 wo = cmul(tw[k], o);
        const float xr = e.x + wo.x, xi = e.y + wo.y;
        p = xr * xr + xi * xi;
      }
      pw[f * n_bins + k] = p;
    }
    __syncthreads();
    // mel rows, ascending bins; then dB
    const int nfb = min(FB, nf - fb0);
    for (int i = t; i < nfb * n_mels; i += AM_THREADS) {
      const int f = i / n_mels, m = i % n_mels;
      const float* p = pw + f * n_bins + meta[m];
      const float* w = wts + meta[2 * n_mels + m];
      const int len = meta[n_mels + m];
      float acc = 0.f;
      for (int e = 0; e < len; ++e) acc = fmaf(w[e], p[e], acc);
      // clamp(min=1e-10) keeps a NaN, as torch.clamp does.  log10 in fp64 rounded to fp32: the device log10f is 1 ulp off at the
      // floor (log10f(1e-10f) != -10), and silence must come out at the composite's -100.0 exactly
      if (log_db) acc = 10.f * (float)log10((double)(acc < 1e-10f ? 1e-10f : acc));
      os[m * (fpb + 1) + fb0 + f] = acc;
    }
    // the next sub-batch writes buf only after its first barrier; pw is rewritten after two more
  }
  __syncthreads();
  for (int i = t; i < n_mels * fpb; i += AM_THREADS) {
    const int m = i / fpb, f = i % fpb;
    if constexpr (LENS) {
      if (f < nfo) out[(b * n_mels + m) * T + f0 + f] = f < nf ? os[m * (fpb + 1) + f] : 0.f;
    } else {
      if (f < nf) out[(b * n_mels + m) * T + f0 + f] = os[m * (fpb + 1) + f];
    }
  }
}

#define AM_HIPRET(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return NS2_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
#define AM_ARGCHK(cond, msg)           \
  do {                                 \
    if (!(cond)) {                     \
      set_error("%s: %s", who, msg);   \
      return NS2_ERR_ARG;              \
    }                                  \
  } while (0)

template <int N, bool LENS>
static int launch_audio_to_mel(const float* audio, int B, int64_t L, int64_t T, int hop, int fpb, size_t lds, const float* window,
                               const float* twiddle, const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins,
                               int log_db, float* out, const int* sample_lens, hipStream_t s) {
  static DynLdsAttr attr;
  AM_HIPRET(attr.ensure(reinterpret_cast<const void*>(&audio_to_mel_kernel<N, LENS>), (int)lds));
  const dim3 grid((unsigned)((T + fpb - 1) / fpb), (unsigned)B);
  hipLaunchKernelGGL((audio_to_mel_kernel<N, LENS>), grid, dim3(AM_THREADS), lds, s, audio, (long)L, (long)T, hop, fpb, window,
                     reinterpret_cast<const float2*>(twiddle), fb_meta, fb_w, n_w, n_mels, n_bins, log_db, out, sample_lens);
  AM_HIPRET(hipGetLastError());
  return NS2_OK;
}

// the argument checks and the launch of both entries; `who` names the entry in the messages
template <bool LENS>
static int audio_to_mel_entry(const char* who, const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window,
                              const float* twiddle, const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db,
                              float* out, const int* sample_lens, void* stream) {
  AM_ARGCHK(audio && window && twiddle && fb_meta && fb_w && out && B > 0 && B <= 65535, "bad arguments");
  if (LENS) AM_ARGCHK(sample_lens, "sample_lens is null (ns2_audio_to_mel is the call without lengths)");
  AM_ARGCHK(n_fft >= 256 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, "n_fft must be a power of two in [256, 2048]");
  AM_ARGCHK(hop_length >= 1 && hop_length <= n_fft, "hop_length must be in [1, n_fft]");
  AM_ARGCHK(n_mels >= 1 && n_mels <= 256, "n_mels must be in [1, 256]");
  const int N = n_fft / 2;
  AM_ARGCHK(n_bins >= 1 && n_bins <= N + 1 && n_w >= 0 && n_w <= 2 * (N + 1), "bad filterbank table sizes");
  AM_ARGCHK(L > N, "reflect padding needs more than n_fft / 2 samples");
  const int64_t T = 1 + L / hop_length;
  int fpb = AM_FPB;
  const int fb = AM_POINTS / N;
  while (fpb > fb && am_lds_bytes(N, fpb, hop_length, n_mels, n_bins, n_w) > (size_t)AM_LDS_SOFT) fpb /= 2;
  const size_t lds = am_lds_bytes(N, fpb, hop_length, n_mels, n_bins, n_w);
  AM_ARGCHK(lds <= (size_t)AM_LDS_MAX, "configuration exceeds the LDS");
  AM_ARGCHK((T + fpb - 1) / fpb <= INT_MAX, "too many frames");
  const hipStream_t s = (hipStream_t)stream;
  switch (N) {
    case 128: return launch_audio_to_mel<128, LENS>(audio, B, L, T, hop_length, fpb, lds, window, twiddle, fb_meta, fb_w, n_w, n_mels, n_bins, log_db, out, sample_lens, s);
    case 256: return launch_audio_to_mel<256, LENS>(audio, B, L, T, hop_length, fpb, lds, window, twiddle, fb_meta, fb_w, n_w, n_mels, n_bins, log_db, out, sample_lens, s);
    case 512: return launch_audio_to_mel<512, LENS>(audio, B, L, T, hop_length, fpb, lds, window, twiddle, fb_meta, fb_w, n_w, n_mels, n_bins, log_db, out, sample_lens, s);
    default: return launch_audio_to_mel<1024, LENS>(audio, B, L, T, hop_length, fpb, lds, window, twiddle, fb_meta, fb_w, n_w, n_mels, n_bins, log_db, out, sample_lens, s);
  }
}

}  // namespace ns2

using namespace ns2;

extern "C" int ns2_audio_to_mel(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window, const float* twiddle,
                                const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db, float* out,
                                void* stream) {
  return audio_to_mel_entry<false>("ns2_audio_to_mel", audio, B, L, n_fft, hop_length, window, twiddle, fb_meta, fb_w, n_w, n_mels, n_bins,
                                   log_db, out, nullptr, stream);
}

// ... of a ragged batch
extern "C" int ns2_audio_to_mel_lens(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window,
                                     const float* twiddle, const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins,
                                     int log_db, float* out, const int* sample_lens, void* stream) {
  return audio_to_mel_entry<true>("ns2_audio_to_mel_lens", audio, B, L, n_fft, hop_length, window, twiddle, fb_meta, fb_w, n_w, n_mels,
                                  n_bins, log_db, out, sample_lens, stream);
}
