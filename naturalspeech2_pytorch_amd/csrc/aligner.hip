// The Aligner's pieces of the text-conditioned training pass (NS2:1524-1602, aligner.py, utils.py:4-33) that the GEMM
// kernels do not cover:
//   - ReLU + split: the activations between the Aligner's convolutions (AlignerNet, aligner.py:17-60) as operand planes,
//     padding columns zeroed (80 and 160 channels are not multiples of 32);
//   - the attention of AlignerNet.forward (aligner.py:62-90): plain Euclidean distances summed in fp32 on the vector ALUs,
//     masked phonemes filled with -FLT_MAX, softmax over phonemes, written as aln_log [B, 1, T, n] and transposed as
//     aln_soft [B, n, T];
//   - the monotonic alignment search maximum_path (aligner.py:97-130): one wave per utterance walks the mel frames in order
//     with the DP column in registers (R rows per lane, v[i-1] across lanes by a DPP wave shift), packs the direction bits
//     into LDS (or a caller-provided scratch when they do not fit), backtracks from LDS, and a second kernel writes the 0/1
//     path and its row sums;
//   - average_over_durations (utils.py:4-26) from fp32 prefix sums;
//   - the backward of expand_encodings (NS2:1449-1455): d enc[b, i] = sum of d cond over phoneme i's frames and
//     d pitch_emb.weight[bin] summed over (b, i) in a fixed order -- no atomics, bit-reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "ns2_common.h"
#include "ns2_host.h"

namespace ns2 {

// ---------------------------------------------------------------- ReLU + split
__global__ __launch_bounds__(256) void relu_split_kernel(const float* x, int M, int N, bf16_t* out_hi, bf16_t* out_lo, int ldo,
                                                         int fmt) {
  const bool il = fmt_il(fmt, out_lo);
  const long quads = (long)M * (ldo / 4);
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long row = q / (ldo / 4);
    const int c = (int)(q % (ldo / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < N) v = *reinterpret_cast<const float4*>(x + row * N + c);      // N % 4 == 0: a quad is all in or all padding
    store_cols4(out_hi + row * pld(ldo, il), c, fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f), fmt, il);
  }
}

// ---------------------------------------------------------------- distances + mask + softmax (aligner.py:62-90)
constexpr int AA_TQ = 16;                 // mel frames per block
constexpr int AA_TK = 64;                 // phonemes per key tile

NS2_DEVINL float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (ceil(T / AA_TQ), B), 256 threads; dynamic LDS: q [AA_TQ][C] | k [AA_TK][C + 1] | row [AA_TQ][n]
__global__ __launch_bounds__(256) void align_attn_kernel(const float* q, const float* k, const int* text_lens, int T, int n, int C,
                                                         float* aln_log, float* aln_soft) {
  extern __shared__ float sm[];
  float* qs = sm;
  float* ks = qs + AA_TQ * C;
  float* rows = ks + AA_TK * (C + 1);
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, t = threadIdx.x;
  const int tl = min(max(text_lens[b], 0), n);
  const int nq = min(AA_TQ, T - t0);
  for (int i = t; i < AA_TQ * C; i += 256) {
    const int f = i / C, c = i % C;
    qs[i] = f < nq ? q[((long)b * T + t0 + f) * C + c] : 0.f;
  }
  const int kk = t & 63, fq = (t >> 6) * 4;
  for (int k0 = 0; k0 < n; k0 += AA_TK) {
    __syncthreads();
    for (int i = t; i < AA_TK * C; i += 256) {
      const int j = i / C, c = i % C;
      ks[j * (C + 1) + c] = k0 + j < n ? k[((long)b * n + k0 + j) * C + c] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
      const float kc = ks[kk * (C + 1) + c];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = qs[(fq + e) * C + c] - kc;
        acc[e] += d * d;
      }
    }
    if (k0 + kk < n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rows[(fq + e) * n + k0 + kk] = k0 + kk < tl ? sqrtf(acc[e]) : -FLT_MAX;
    }
  }
  __syncthreads();
  const int w = t >> 6, lane = t & 63;
  for (int f = w; f < nq; f += 4) {                   // one wave per frame: masked log row, then softmax in place
    float* r = rows + f * n;
    float m = -FLT_MAX;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, r[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += expf(r[i] - m);
    s = wave_sum(s);
    float* lr = aln_log + ((long)b * T + t0 + f) * n;
    for (int i = lane; i < n; i += 64) {
      const float x = r[i];
      lr[i] = x;
      r[i] = expf(x - m) / s;
    }
  }
  __syncthreads();
  for (int i = t; i < n * AA_TQ; i += 256) {          // transposed: 16 consecutive frames of one phoneme
    const int ph = i / AA_TQ, f = i % AA_TQ;
    if (f < nq) aln_soft[((long)b * n + ph) * T + t0 + f] = rows[f * n + ph];
  }
}

// ---------------------------------------------------------------- maximum_path (aligner.py:97-130)
// Layout of the direction bits of one utterance: lane l of the search wave owns rows [l R, l R + R); every CPW = 32 / R
// columns it writes one 32-bit word, bit (j % CPW) R + r = direction of row l R + r at column j (1 = stay, 0 = come from
// the row above).  Word (g, l) sits at g * 64 + l: t_x_pad * t_y / 8 bytes per utterance, t_x_pad = 64 R.
constexpr int MP_STAGE = 64;              // groups of words staged into LDS per backtrack block (scratch mode): 16 KiB
constexpr int64_t MP_LDS_BITS_MAX = 128 * 1024;

static inline int mp_rows_per_lane(int t_x) {
  int r = 1;
  while (64 * r < t_x) r <<= 1;
  return r;
}
static inline int64_t mp_bits_bytes(int t_x, int t_y) {
  const int cpw = 32 / mp_rows_per_lane(t_x);
  return (int64_t)((t_y + cpw - 1) / cpw) * 64 * 4;
}

NS2_DEVINL float shift_up1(float x) {       // lane l <- lane l - 1 (DPP wave_shr:1); lane 0 <- -inf
  const int r = __builtin_amdgcn_update_dpp(__float_as_int(-__builtin_inff()), __float_as_int(x), 0x138, 0xF, 0xF, false);
  return (threadIdx.x & 63) == 0 ? -__builtin_inff() : __int_as_float(r);
}

// the reference's backtrack over columns [j_lo, j_hi] reading words from `words` (group g at (g - g0) * 64); lane 0 only.
// Python indexing: a negative row index counts from the end (only reachable with NaN values); below -t_x the reference
// raises IndexError -- here the remaining columns get no path.
template <int R>
NS2_DEVINL void mp_walk(const uint32_t* words, int g0, int j_hi, int j_lo, int& idx, int t_x, int tl, short* ro) {
  constexpr int CPW = 32 / R;
  int key = -1;
  uint32_t word = 0;
  for (int j = j_hi; j >= j_lo; --j) {
    if (idx < -t_x) { ro[j] = -1; continue; }
    const int row = idx < 0 ? idx + t_x : idx;
    int d = 1;                                         // outside the mask the direction is forced to 1
    if (row < tl) {
      ro[j] = (short)row;
      const int kw = (j / CPW - g0) * 64 + row / R;
      if (kw != key) { word = words[kw]; key = kw; }
      d = (word >> ((j % CPW) * R + row % R)) & 1;
    } else {
      ro[j] = -1;
    }
    idx += d - 1;
  }
}

// grid (B), one wave; dynamic LDS: the bits (LDS_BITS) or the staging window.  rowof[b, j] (j < mel_len) <- the path's row
// at column j, -1 where the path is masked out.
template <int R, bool LDS_BITS>
__global__ __launch_bounds__(64) void mp_search_kernel(const float* value, const int* text_lens, const int* mel_lens, int t_x, int t_y,
                                                       uint32_t* gbits, int64_t gbits_words, short* rowof) {
  extern __shared__ uint32_t mp_sm[];
  constexpr int CPW = 32 / R;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int tl = min(max(text_lens[b], 0), t_x), ml = min(max(mel_lens[b], 0), t_y);
  if (tl == 0 || ml == 0) return;                    // no live cell: the write kernel emits zeros without reading rowof
  uint32_t* bits = LDS_BITS ? mp_sm : gbits + (long)b * gbits_words;
  short* ro = rowof + (long)b * t_y;
  const float* vb = value + (long)b * t_x * t_y;
  const int row0 = lane * R;
  const float NEG_INF = -__builtin_inff();

  float v[R], cur[R][4], nxt[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = 0.f;            // v starts as zeros (aligner.py:105)
  // runs of 4 columns per row; cells outside the lengths are never read (they cannot reach the masked output)
  auto load = [&](float (&dst)[R][4], int j0) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int row = row0 + r, j = j0 + c;
        dst[r][c] = (row < tl && j < ml) ? vb[(long)row * t_y + j] : 0.f;
      }
  };
  load(cur, 0);
  uint32_t acc = 0;
  for (int j0 = 0; j0 < ml; j0 += 4) {
    load(nxt, j0 + 4);                                 // prefetch the next run
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + c;
      if (j < ml) {
        const float prev = shift_up1(v[R - 1]);
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
          const float v1 = v[r], v0 = r ? v[r - 1] : prev;
          const bool m = v1 >= v0;                     // a tie stays
          const float vm = m ? v1 : v0;
          if (m || row0 + r >= tl) acc |= 1u << ((j % CPW) * R + r);
          v[r] = row0 + r <= j ? vm + cur[r][c] : NEG_INF;
        }
        if ((j + 1) % CPW == 0 || j == ml - 1) {
          bits[(j / CPW) * 64 + lane] = acc;
          acc = 0;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) cur[r][c] = nxt[r][c];
  }
  __syncthreads();
  int idx = tl - 1;                                  // mask[:, :, 0].sum() - 1 with mel_len > 0
  if (LDS_BITS) {
    if (lane == 0) mp_walk<R>(bits, 0, ml - 1, 0, idx, t_x, tl, ro);
    return;
  }
  // scratch mode: stage MP_STAGE groups at a time (independent loads by every lane), walk them from LDS
  for (int gh = (ml - 1) / CPW; gh >= 0; gh -= MP_STAGE) {
    const int gl = max(0, gh - MP_STAGE + 1);
    for (int g = gl; g <= gh; ++g) mp_sm[(g - gl) * 64 + lane] = bits[(long)g * 64 + lane];
    __syncthreads();
    if (lane == 0) mp_walk<R>(mp_sm, gl, min(ml - 1, (gh + 1) * CPW - 1), gl * CPW, idx, t_x, tl, ro);
    __syncthreads();
  }
}

// grid (ceil(t_x / 4), B), 256 threads: one wave per row writes path[b, i, :] and durations[b, i] = its row sum
__global__ __launch_bounds__(256) void mp_write_kernel(const short* rowof, const int* text_lens, const int* mel_lens, int t_x, int t_y,
                                                       float* path, int* durations) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= t_x) return;
  const int tl = min(max(text_lens[b], 0), t_x), ml = min(max(mel_lens[b], 0), t_y);
  const int jl = (i < tl) ? ml : 0;                  // columns that can hold a 1 in this row
  const short* ro = rowof + (long)b * t_y;
  float* pr = path + ((long)b * t_x + i) * t_y;
  float cnt = 0.f;
  for (int j = lane; j < t_y; j += 64) {
    const bool on = j < jl && ro[j] == i;
    pr[j] = on ? 1.f : 0.f;
    cnt += on ? 1.f : 0.f;
  }
  cnt = wave_sum(cnt);                               // at most 8192: exact
  if (lane == 0) durations[(long)b * t_x + i] = (int)cnt;
}

// ---------------------------------------------------------------- average_over_durations (utils.py:4-26)
constexpr int AV_THREADS = 256;

// grid (B); dynamic LDS: cums[T + 1] fp32 | nz[T + 1] int | ends[n] int.  Prefix sums are accumulated in fp64 and rounded to
// fp32 per frame, as torch's CPU cumsum of fp32 does; integer-valued pitch gives exact prefixes either way.
__global__ __launch_bounds__(AV_THREADS) void avg_dur_kernel(const float* pitch, const int* durs, int T, int n, float* out) {
  extern __shared__ float av_sm[];
  float* cums = av_sm;
  int* nz = reinterpret_cast<int*>(cums + T + 1);
  int* ends = nz + T + 1;
  __shared__ double dpart[AV_THREADS];
  __shared__ int ipart[AV_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* x = pitch + (long)b * T;
  {
    const int per = (T + AV_THREADS - 1) / AV_THREADS;
    const int j0 = min(t * per, T), j1 = min(j0 + per, T);
    double s = 0.0;
    int c = 0;
    for (int j = j0; j < j1; ++j) { s += (double)x[j]; c += x[j] != 0.f; }
    dpart[t] = s;
    ipart[t] = c;
    __syncthreads();
    for (int o = 1; o < AV_THREADS; o <<= 1) {       // Hillis-Steele over the segment sums, fixed order
      const double dv = t >= o ? dpart[t - o] : 0.0;
      const int iv = t >= o ? ipart[t - o] : 0;
      __syncthreads();
      dpart[t] += dv;
      ipart[t] += iv;
      __syncthreads();
    }
    s = dpart[t] - s;
    c = ipart[t] - c;
    if (t == 0) { cums[0] = 0.f; nz[0] = 0; }
    for (int j = j0; j < j1; ++j) {
      s += (double)x[j];
      c += x[j] != 0.f;
      cums[j + 1] = (float)s;
      nz[j + 1] = c;
    }
  }
  __syncthreads();
  {
    const int* d = durs + (long)b * n;
    const int per = (n + AV_THREADS - 1) / AV_THREADS;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += max(d[i], 0);
    ipart[t] = s;
    __syncthreads();
    for (int o = 1; o < AV_THREADS; o <<= 1) {
      const int iv = t >= o ? ipart[t - o] : 0;
      __syncthreads();
      ipart[t] += iv;
      __syncthreads();
    }
    s = ipart[t] - s;
    for (int i = i0; i < i1; ++i) { s += max(d[i], 0); ends[i] = min(s, T); }
  }
  __syncthreads();
  for (int i = t; i < n; i += AV_THREADS) {
    const int e = ends[i], s = i ? ends[i - 1] : 0;
    const float sum = cums[e] - cums[s];
    const float cnt = (float)(nz[e] - nz[s]);
    out[(long)b * n + i] = cnt == 0.f ? cnt : sum / cnt;
  }
}

// ---------------------------------------------------------------- expand_encodings backward (NS2:1449-1455)
// f0_to_coarse (NS2:164-175), the same fp32 operations as the length regulator's (duration_pitch.hip)
NS2_DEVINL int al_f0_coarse(float f0, float mel_min, float mel_max) {
#pragma clang fp contract(off)
  float m = 1127.0f * logf(1.0f + f0 / 700.0f);
  if (m > 0.f) m = (m - mel_min) * 254.0f / (mel_max - mel_min) + 1.0f;
  if (m <= 1.0f) m = 1.0f;
  if (m > 255.0f) m = 255.0f;
  const int c = (int)(m + 0.5f);
  return c < 1 ? 1 : (c > 255 ? 255 : c);
}

// grid (B), 256 threads: starts[b, i] = first frame of phoneme i (int(duration) >= 0 summed, capped at n_frames), starts[b, n]
// = the end of the last one; bins[b, i] = f0_to_coarse(pitch[b, i])
__global__ __launch_bounds__(256) void ex_scan_kernel(const float* dur, const float* pitch, int n, int n_frames, float mel_min,
                                                      float mel_max, int* starts, int* bins) {
  __shared__ int part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* d = dur + (long)b * n;
  const int per = (n + 255) / 256;
  const int i0 = min(t * per, n), i1 = min(i0 + per, n);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += max((int)d[i], 0);
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  s = part[t] - s;
  int* st = starts + (long)b * (n + 1);
  for (int i = i0; i < i1; ++i) {
    st[i] = min(s, n_frames);
    s += max((int)d[i], 0);
    bins[(long)b * n + i] = al_f0_coarse(pitch[(long)b * n + i], mel_min, mel_max);
  }
  if (t == 255) st[n] = min(part[255], n_frames);
}

// grid (n, B), 256 threads over channels: d_enc[b, i, c] = sum over phoneme i's frames f (ascending) of d_cond[b, c, f]
__global__ __launch_bounds__(256) void ex_denc_kernel(const float* d_cond, const int* starts, int n, int D, int n_frames, float* d_enc) {
  const int i = blockIdx.x, b = blockIdx.y;
  const int* st = starts + (long)b * (n + 1);
  const int f0 = st[i], f1 = st[i + 1];
  for (int c = threadIdx.x; c < D; c += 256) {
    const float* g = d_cond + ((long)b * D + c) * n_frames;
    float s = 0.f;
    for (int f = f0; f < f1; ++f) s += g[f];
    d_enc[((long)b * n + i) * D + c] = s;
  }
}

// grid (V, ceil(D / 64)), one wave: d_table[bin, c] = sum over (b, i) in ascending order with bins[b, i] == bin of d_enc[b, i, c]
__global__ __launch_bounds__(64) void ex_dtable_kernel(const float* d_enc, const int* bins, int entries, int D, float* d_table) {
  const int bin = blockIdx.x, c = blockIdx.y * 64 + threadIdx.x;
  float s = 0.f;
  for (int e0 = 0; e0 < entries; e0 += 64) {
    const int e = e0 + threadIdx.x;
    uint64_t m = __ballot(e < entries && bins[e] == bin);
    while (m) {
      const int k = __builtin_ctzll(m);
      m &= m - 1;
      if (c < D) s += d_enc[(long)(e0 + k) * D + c];
    }
  }
  if (c < D) d_table[(long)bin * D + c] = s;
}

}  // namespace ns2

using namespace ns2;

#define AL_HIPRET(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return NS2_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
#define AL_ARGCHK(cond, msg) \
  do {                       \
    if (!(cond)) {           \
      set_error("%s", msg);  \
      return NS2_ERR_ARG;    \
    }                        \
  } while (0)

extern "C" int ns2_relu_split(const float* x, int M, int N, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream) {
  AL_ARGCHK(x && out_hi && M > 0 && N > 0 && N % 4 == 0 && ldo % 32 == 0 && ldo >= N, "ns2_relu_split: bad arguments");
  AL_ARGCHK(precision >= 1 && precision <= 4, "ns2_relu_split: precision must be 1 .. 4");
  AL_ARGCHK(precision != 2 || !out_lo, "ns2_relu_split: precision 2 (fp16) has no lo plane");
  AL_ARGCHK(precision != 3 || out_lo, "ns2_relu_split: precision 3 planes need the lo plane");
  AL_ARGCHK((uintptr_t)x % 16 == 0, "ns2_relu_split: x must be 16-byte aligned");
  const int fmt = precision == 2 ? FMT_F16 : (precision == 4 ? FMT_H8 : FMT_BF16);
  const long quads = (long)M * (ldo / 4);
  const int blocks = (int)std::min<long>((quads + 255) / 256, 4096);
  hipLaunchKernelGGL(relu_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, M, N, reinterpret_cast<bf16_t*>(out_hi),
                     reinterpret_cast<bf16_t*>(out_lo), ldo, fmt);
  AL_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_align_attn(const float* queries, const float* keys, const int* text_lens, int B, int T, int n, int C, float* aln_log,
                              float* aln_soft, void* stream) {
  AL_ARGCHK(queries && keys && text_lens && aln_log && aln_soft && B > 0 && T > 0 && n > 0 && C > 0, "ns2_align_attn: bad arguments");
  AL_ARGCHK(n <= 1024 && C <= 256, "ns2_align_attn: at most 1024 phonemes and 256 channels");
  const size_t lds = sizeof(float) * ((size_t)AA_TQ * C + (size_t)AA_TK * (C + 1) + (size_t)AA_TQ * n);
  static DynLdsAttr attr;
  AL_HIPRET(attr.ensure(reinterpret_cast<const void*>(&align_attn_kernel), (int)lds));
  hipLaunchKernelGGL(align_attn_kernel, dim3((T + AA_TQ - 1) / AA_TQ, B), dim3(256), lds, (hipStream_t)stream, queries, keys,
                     text_lens, T, n, C, aln_log, aln_soft);
  AL_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int64_t ns2_maximum_path_workspace_bytes(int B, int t_x, int t_y) {
  if (B <= 0 || t_x <= 0 || t_y <= 0 || t_x > 1024 || t_y > 8192) return 0;
  const int64_t rowof = ((int64_t)B * t_y * 2 + 255) / 256 * 256;
  const int64_t bits = mp_bits_bytes(t_x, t_y);
  return rowof + (bits <= MP_LDS_BITS_MAX ? 0 : (int64_t)B * bits);
}

template <int R>
static hipError_t mp_launch(bool lds_bits, const float* value, const int* tl, const int* ml, int B, int t_x, int t_y, uint32_t* gbits,
                           int64_t words, short* rowof, hipStream_t s) {
  static DynLdsAttr attr;
  if (lds_bits) {
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&mp_search_kernel<R, true>), (int)(words * 4));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mp_search_kernel<R, true>), dim3(B), dim3(64), (size_t)words * 4, s, value, tl, ml, t_x, t_y, gbits, words, rowof);
  } else {
    hipLaunchKernelGGL((mp_search_kernel<R, false>), dim3(B), dim3(64), (size_t)MP_STAGE * 64 * 4, s, value, tl, ml, t_x, t_y, gbits,
                       words, rowof);
  }
  return hipGetLastError();
}

extern "C" int ns2_maximum_path(const float* value, const int* text_lens, const int* mel_lens, int B, int t_x, int t_y, float* path,
                                int* durations, void* workspace, int64_t workspace_bytes, void* stream) {
  AL_ARGCHK(value && text_lens && mel_lens && path && durations && B > 0 && t_x > 0 && t_y > 0, "ns2_maximum_path: bad arguments");
  AL_ARGCHK(t_x <= 1024 && t_y <= 8192, "ns2_maximum_path: at most 1024 phonemes and 8192 mel frames");
  AL_ARGCHK(workspace && workspace_bytes >= ns2_maximum_path_workspace_bytes(B, t_x, t_y), "ns2_maximum_path: workspace too small");
  const int64_t bits = mp_bits_bytes(t_x, t_y);
  const bool lds_bits = bits <= MP_LDS_BITS_MAX;
  short* rowof = reinterpret_cast<short*>(workspace);
  uint32_t* gbits = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + ((int64_t)B * t_y * 2 + 255) / 256 * 256);
  const int64_t words = bits / 4;
  hipStream_t s = (hipStream_t)stream;
  switch (mp_rows_per_lane(t_x)) {
    case 1: AL_HIPRET(mp_launch<1>(lds_bits, value, text_lens, mel_lens, B, t_x, t_y, gbits, words, rowof, s)); break;
    case 2: AL_HIPRET(mp_launch<2>(lds_bits, value, text_lens, mel_lens, B, t_x, t_y, gbits, words, rowof, s)); break;
    case 4: AL_HIPRET(mp_launch<4>(lds_bits, value, text_lens, mel_lens, B, t_x, t_y, gbits, words, rowof, s)); break;
    case 8: AL_HIPRET(mp_launch<8>(lds_bits, value, text_lens, mel_lens, B, t_x, t_y, gbits, words, rowof, s)); break;
    default: AL_HIPRET(mp_launch<16>(lds_bits, value, text_lens, mel_lens, B, t_x, t_y, gbits, words, rowof, s)); break;
  }
  AL_HIPRET(hipGetLastError());
  hipLaunchKernelGGL(mp_write_kernel, dim3((t_x + 3) / 4, B), dim3(256), 0, s, rowof, text_lens, mel_lens, t_x, t_y, path, durations);
  AL_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_average_over_durations(const float* pitch, const int* durations, int B, int T, int n, float* out, void* stream) {
  AL_ARGCHK(pitch && durations && out && B > 0 && T > 0 && n > 0, "ns2_average_over_durations: bad arguments");
  AL_ARGCHK(T <= 8192 && n <= 8192, "ns2_average_over_durations: at most 8192 frames and 8192 phonemes");
  const size_t lds = (size_t)(T + 1) * 8 + (size_t)n * 4;
  static DynLdsAttr attr;
  AL_HIPRET(attr.ensure(reinterpret_cast<const void*>(&avg_dur_kernel), (int)lds));
  hipLaunchKernelGGL(avg_dur_kernel, dim3(B), dim3(AV_THREADS), lds, (hipStream_t)stream, pitch, durations, T, n, out);
  AL_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int64_t ns2_expand_backward_workspace_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return (int64_t)B * (2 * n + 1) * 4;
}

extern "C" int ns2_expand_backward(const float* d_cond, const float* duration, const float* pitch, int B, int n, int D, int n_frames,
                                   int n_bins, float mel_min, float mel_max, float* d_enc, float* d_table, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  AL_ARGCHK(d_cond && duration && pitch && d_enc && B > 0 && n > 0 && D > 0 && n_frames > 0, "ns2_expand_backward: bad arguments");
  AL_ARGCHK(!d_table || n_bins >= 256, "ns2_expand_backward: the pitch table needs at least 256 rows");
  AL_ARGCHK(workspace && workspace_bytes >= ns2_expand_backward_workspace_bytes(B, n), "ns2_expand_backward: workspace too small");
  int* starts = reinterpret_cast<int*>(workspace);
  int* bins = starts + (int64_t)B * (n + 1);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ex_scan_kernel, dim3(B), dim3(256), 0, s, duration, pitch, n, n_frames, mel_min, mel_max, starts, bins);
  AL_HIPRET(hipGetLastError());
  hipLaunchKernelGGL(ex_denc_kernel, dim3(n, B), dim3(256), 0, s, d_cond, starts, n, D, n_frames, d_enc);
  AL_HIPRET(hipGetLastError());
  if (d_table) {
    hipLaunchKernelGGL(ex_dtable_kernel, dim3(n_bins, (D + 63) / 64), dim3(64), 0, s, d_enc, bins, B * n, D, d_table);
    AL_HIPRET(hipGetLastError());
  }
  return NS2_OK;
}
