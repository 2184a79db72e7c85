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

// ---------------------------------------------------------------- training: backward of the distances + softmax (aligner.py:72-90)
// With G = g_log + soft (g_soft - sum_i soft g_soft) on the live cells (i < text_len) and w = G / dist (0 where masked or dist == 0,
// torch.cdist's convention):  dq_t = sum_i w (q_t - k_i),  dk_i = sum_t w (k_i - q_t) -- the DIRECT form: rowsum(w) q - w K cancels
// where q ~ k.  Three kernels: w [B, T, n] once; dq sums over the phonemes in ascending order; dk sums over fixed slices of
// AB_SLICE frames into slots that the slice reducer (backward.hip) adds in a fixed order.  No atomics: two runs give the same bits.
constexpr int AB_SLICE = 256;             // frames per dk slot

// grid (ceil(T / AA_TQ), B), 256 threads
__global__ __launch_bounds__(256) void align_w_kernel(const float* aln_log, const float* aln_soft, const float* g_log, const float* g_soft,
                                                      const int* text_lens, int T, int n, float* w) {
  __shared__ float part[16][AA_TQ + 1];
  __shared__ float srow[AA_TQ];
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, t = threadIdx.x;
  const int tl = min(max(text_lens[b], 0), n);
  const int nq = min(AA_TQ, T - t0);
  {                                                   // sum_i soft g_soft per frame: 16 phoneme groups, added in group order
    const int f = t & (AA_TQ - 1), pg = t >> 4;
    float s = 0.f;
    if (g_soft && f < nq)
      for (int ph = pg; ph < tl; ph += 16) {
        const long o = ((long)b * n + ph) * T + t0 + f;
        s += aln_soft[o] * g_soft[o];
      }
    part[pg][f] = s;
  }
  __syncthreads();
  if (t < AA_TQ) {
    float s = part[0][t];
#pragma unroll
    for (int g = 1; g < 16; ++g) s += part[g][t];
    srow[t] = s;
  }
  __syncthreads();
  const int wv = t >> 6, lane = t & 63;
  for (int f = wv; f < nq; f += 4) {
    const long row = ((long)b * T + t0 + f) * n;
    const float sr = srow[f];
    for (int i = lane; i < n; i += 64) {
      float r = 0.f;
      if (i < tl) {
        const float d = aln_log[row + i];
        float G = g_log ? g_log[row + i] : 0.f;
        if (g_soft) {
          const long o = ((long)b * n + i) * T + t0 + f;
          G += aln_soft[o] * (g_soft[o] - sr);
        }
        r = d > 0.f ? G / d : 0.f;
      }
      w[row + i] = r;
    }
  }
}

// grid (ceil(T / AA_TQ), B), 256 threads: thread (f = t / 16, c = t % 16 + 16 e) owns dq[t0 + f, c]; dynamic LDS:
// q [AA_TQ][C] | k [AA_TK][C + 1] | w [AA_TQ][AA_TK]
template <int NJ>
__global__ __launch_bounds__(256) void align_dq_kernel(const float* q, const float* k, const float* w, const int* text_lens, int T, int n,
                                                       int C, float* dq) {
  extern __shared__ float sm[];
  float* qs = sm;
  float* ks = qs + AA_TQ * C;
  float* ws = ks + AA_TK * (C + 1);
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, t = threadIdx.x;
  const int tl = min(max(text_lens[b], 0), n);
  const int nq = min(AA_TQ, T - t0);
  for (int i = t; i < AA_TQ * C; i += 256) {
    const int f = i / C, c = i % C;
    qs[i] = f < nq ? q[((long)b * T + t0 + f) * C + c] : 0.f;
  }
  const int f = t >> 4, c0 = t & 15;
  int cc[NJ];
  float acc[NJ];
#pragma unroll
  for (int e = 0; e < NJ; ++e) { cc[e] = min(c0 + 16 * e, C - 1); acc[e] = 0.f; }
  for (int k0 = 0; k0 < tl; k0 += AA_TK) {              // tl is the block's own: every thread runs the same trips
    __syncthreads();
    for (int i = t; i < AA_TK * C; i += 256) {
      const int j = i / C, c = i % C;
      ks[j * (C + 1) + c] = k0 + j < n ? k[((long)b * n + k0 + j) * C + c] : 0.f;
    }
    for (int i = t; i < AA_TQ * AA_TK; i += 256) {
      const int ff = i / AA_TK, j = i % AA_TK;
      ws[i] = (ff < nq && k0 + j < n) ? w[((long)b * T + t0 + ff) * n + k0 + j] : 0.f;
    }
    __syncthreads();
    const int jn = min(AA_TK, tl - k0);
    for (int j = 0; j < jn; ++j) {
      const float wv = ws[f * AA_TK + j];
#pragma unroll
      for (int e = 0; e < NJ; ++e) acc[e] += wv * (qs[f * C + cc[e]] - ks[j * (C + 1) + cc[e]]);
    }
  }
  if (f < nq) {
#pragma unroll
    for (int e = 0; e < NJ; ++e)
      if (c0 + 16 * e < C) dq[((long)b * T + t0 + f) * C + c0 + 16 * e] = acc[e];
  }
}

// grid (ceil(n / 16), slices, B), 256 threads: thread (p = t / 16, c = t % 16 + 16 e) owns slot[slice][i0 + p, c]; dynamic LDS:
// k [16][C] | q [AA_TK][C + 1] | w [AA_TK][16]
template <int NJ>
__global__ __launch_bounds__(256) void align_dk_kernel(const float* q, const float* k, const float* w, const int* text_lens, int T, int n,
                                                       int C, float* partial) {
  extern __shared__ float sm[];
  float* ks = sm;
  float* qs = ks + 16 * C;
  float* ws = qs + AA_TK * (C + 1);
  const int b = blockIdx.z, sl = blockIdx.y, S = gridDim.y, i0 = blockIdx.x * 16, t = threadIdx.x;
  const int tl = min(max(text_lens[b], 0), n);
  const int p = t >> 4, c0 = t & 15;
  float* out = partial + ((long)b * S + sl) * n * C;
  if (i0 >= tl) {                                     // a tile of masked phonemes (the whole block leaves): exact zeros
    if (i0 + p < n)
      for (int c = c0; c < C; c += 16) out[(long)(i0 + p) * C + c] = 0.f;
    return;
  }
  const int ta = sl * AB_SLICE, tb = min(T, ta + AB_SLICE);
  for (int i = t; i < 16 * C; i += 256) {
    const int pp = i / C, c = i % C;
    ks[i] = i0 + pp < n ? k[((long)b * n + i0 + pp) * C + c] : 0.f;
  }
  int cc[NJ];
  float acc[NJ];
#pragma unroll
  for (int e = 0; e < NJ; ++e) { cc[e] = min(c0 + 16 * e, C - 1); acc[e] = 0.f; }
  for (int f0 = ta; f0 < tb; f0 += AA_TK) {
    __syncthreads();
    for (int i = t; i < AA_TK * C; i += 256) {
      const int j = i / C, c = i % C;
      qs[j * (C + 1) + c] = f0 + j < tb ? q[((long)b * T + f0 + j) * C + c] : 0.f;
    }
    for (int i = t; i < AA_TK * 16; i += 256) {
      const int j = i >> 4, pp = i & 15;
      ws[i] = (f0 + j < tb && i0 + pp < n) ? w[((long)b * T + f0 + j) * n + i0 + pp] : 0.f;
    }
    __syncthreads();
    const int jn = min(AA_TK, tb - f0);
    for (int j = 0; j < jn; ++j) {
      const float wv = ws[j * 16 + p];
#pragma unroll
      for (int e = 0; e < NJ; ++e) acc[e] += wv * (ks[p * C + cc[e]] - qs[j * (C + 1) + cc[e]]);
    }
  }
  if (i0 + p < n) {
#pragma unroll
    for (int e = 0; e < NJ; ++e)
      if (c0 + 16 * e < C) out[(long)(i0 + p) * C + c0 + 16 * e] = acc[e];
  }
}

template <int NJ>
static hipError_t align_bwd_launch(const float* q, const float* k, const float* w, const int* tl, int B, int T, int n, int C, float* dq,
                                   float* partial, int S, hipStream_t s) {
  static DynLdsAttr aq, ak;
  const size_t ldq = sizeof(float) * ((size_t)AA_TQ * C + (size_t)AA_TK * (C + 1) + (size_t)AA_TQ * AA_TK);
  const size_t ldk = sizeof(float) * ((size_t)16 * C + (size_t)AA_TK * (C + 1) + (size_t)AA_TK * 16);
  hipError_t e = aq.ensure(reinterpret_cast<const void*>(&align_dq_kernel<NJ>), (int)ldq);
  if (e != hipSuccess) return e;
  e = ak.ensure(reinterpret_cast<const void*>(&align_dk_kernel<NJ>), (int)ldk);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((align_dq_kernel<NJ>), dim3((T + AA_TQ - 1) / AA_TQ, B), dim3(256), ldq, s, q, k, w, tl, T, n, C, dq);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((align_dk_kernel<NJ>), dim3((n + 15) / 16, S, B), dim3(256), ldk, s, q, k, w, tl, T, n, C, partial);
  return hipGetLastError();
}

static inline int64_t ab_w_bytes(int B, int T, int n) { return ((int64_t)B * T * n * 4 + 255) / 256 * 256; }

int64_t align_attn_bwd_workspace_bytes(int B, int T, int n, int C) {
  if (B <= 0 || T <= 0 || n <= 0 || C <= 0) return 0;
  const int S = (T + AB_SLICE - 1) / AB_SLICE;
  return ab_w_bytes(B, T, n) + (int64_t)B * S * n * C * 4;
}

hipError_t launch_align_attn_bwd(const float* q, const float* k, const float* aln_log, const float* aln_soft, const float* g_log,
                                 const float* g_soft, const int* text_lens, int B, int T, int n, int C, float* dq, float* dk,
                                 void* workspace, hipStream_t s) {
  if (B <= 0 || B > 65535 || T <= 0 || T > 8192 || n <= 0 || n > 1024 || C <= 0 || C > 256) return hipErrorInvalidValue;
  float* w = reinterpret_cast<float*>(workspace);
  float* partial = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ab_w_bytes(B, T, n));
  const int S = (T + AB_SLICE - 1) / AB_SLICE;
  hipLaunchKernelGGL(align_w_kernel, dim3((T + AA_TQ - 1) / AA_TQ, B), dim3(256), 0, s, aln_log, aln_soft, g_log, g_soft, text_lens, T, n, w);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int nj = (C + 15) / 16;
  if (nj <= 2) e = align_bwd_launch<2>(q, k, w, text_lens, B, T, n, C, dq, partial, S, s);
  else if (nj <= 3) e = align_bwd_launch<3>(q, k, w, text_lens, B, T, n, C, dq, partial, S, s);
  else if (nj <= 5) e = align_bwd_launch<5>(q, k, w, text_lens, B, T, n, C, dq, partial, S, s);
  else if (nj <= 8) e = align_bwd_launch<8>(q, k, w, text_lens, B, T, n, C, dq, partial, S, s);
  else e = align_bwd_launch<16>(q, k, w, text_lens, B, T, n, C, dq, partial, S, s);
  if (e != hipSuccess) return e;
  return launch_reduce_slices(partial, B, S, (long)n * C, dk, 0, s);
}

// ---------------------------------------------------------------- training: forward-sum (CTC) and bin losses (aligner.py:132-183)
// Forward-sum: per frame t < mel_len the log-softmax over [blank | aln_log[t, 0 .. L - 1]] (L = text_len; the padded row's columns
// > L are excluded), CTC with blank 0 and the targets 1 .. L (distinct labels: a label state may always skip the blank before it),
// S = 2 L + 1 states, zero_infinity, mean over the batch of nll / max(L, 1).  Bin: sum hard log_softmax(aln_log) over the columns
// <= L (column L is kept, as upstream: it holds the aligner's -FLT_MAX), divided by B.
// Workspace: stats [B T][4] fp32 = (-, lse of the bin row, sum_i hard, sum_i hard logp) | lse of the forward-sum row [B T] fp64 | nll [B]
// fp64 | alpha [B][T][2 n + 1] fp64 | e [B][T][2 n + 1] fp64 (the backward's; the forward's part stays as it is, so a backward may be
// repeated).  The recursions run one workgroup per utterance in log space, state s of lane l = l + 256 j, the previous column in LDS
// (two buffers, one barrier per frame); every barrier is unconditional and mel_len is the workgroup's own trip count.
// Arithmetic: the row statistics of the forward-sum rows, the recursions and the occupancies are fp64.  The gradient softmax -
// occupancy cancels (a one-label utterance has both at 1 - 5e-5), and the states that carry mass sit ~10 below the frame's maximum, where
// an fp32 recursion loses 1e-6 per frame: measured on the tests' inputs, fp32 left the gradient 300 .. 10000 x 2^-24 of its largest
// element off, as torch's own fp32 ctc_loss does; fp64 leaves what the fp32 inputs and output allow.
constexpr int AL_STATS = 4;
static inline int64_t al_stats_floats(int B, int T) { return ((int64_t)B * T * AL_STATS + 63) / 64 * 64; }
static inline int64_t al_lse_floats(int B, int T) { return ((int64_t)B * T + 31) / 32 * 64; }      // B T doubles
static inline int64_t al_nll_floats(int B) { return ((int64_t)B + 31) / 32 * 64; }                 // B doubles

int64_t align_losses_workspace_bytes(int B, int T, int n) {
  if (B <= 0 || T <= 0 || n <= 0) return 0;
  return 4 * (al_stats_floats(B, T) + al_lse_floats(B, T) + al_nll_floats(B) + 4 * (int64_t)B * T * (2 * n + 1));
}

NS2_DEVINL double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
NS2_DEVINL double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (ceil(T / AA_TQ), B), 256 threads: one wave per frame, four frames each
__global__ __launch_bounds__(256) void al_rowstat_kernel(const float* aln_log, const float* hard, const int* text_lens, int T, int n,
                                                         float blank, float* stats, double* lse_fs) {
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = min(max(text_lens[b], 0), n), Lb = min(L + 1, n);
  for (int f = wv; f < AA_TQ && t0 + f < T; f += 4) {
    const int t = t0 + f;
    const float* x = aln_log + ((long)b * T + t) * n;
    float m = blank, m2 = -FLT_MAX;
    for (int i = lane; i < Lb; i += 64) {
      const float v = x[i];
      if (i < L) m = fmaxf(m, v);
      m2 = fmaxf(m2, v);
    }
    m = wave_max(m);
    m2 = wave_max(m2);
    double s = 0.0;
    float s2 = 0.f;
    for (int i = lane; i < Lb; i += 64) {
      const float v = x[i];
      if (i < L && lse_fs) s += exp((double)v - (double)m);
      s2 += expf(v - m2);
    }
    s = wave_sum_d(s) + exp((double)blank - (double)m);
    s2 = wave_sum(s2);
    const float ls2 = logf(s2);
    float hs = 0.f, br = 0.f;
    if (hard)
      for (int i = lane; i < Lb; i += 64) {
        const float h = hard[((long)b * n + i) * T + t];
        hs += h;
        br += h * ((x[i] - m2) - ls2);
      }
    hs = wave_sum(hs);
    br = wave_sum(br);
    if (lane == 0) {
      float* st = stats + ((long)b * T + t) * AL_STATS;
      st[0] = 0.f;
      if (lse_fs) lse_fs[(long)b * T + t] = (double)m + log(s);
      st[1] = m2 + ls2;
      st[2] = hs;
      st[3] = br;
    }
  }
}

// The recursions run on SCALED PROBABILITIES, not logs: A_t(s) = (A_{t-1}(s) + A_{t-1}(s - 1) [+ A_{t-1}(s - 2) for a label state]) y_t(s) 2^-k,
// y_t(s) = exp(max(lp_t(s), -700)), k = the binary exponent of the previous frame's maximum (every wave leaves its maximum in LDS before
// that frame's barrier).  A power of two scales exactly, costs one ldexp and keeps the frame's maximum in [0.5, 1) y whatever the length;
// the sums add positive numbers only.  Per state and frame that is one exp off the LDS dependency chain where the log-space form has three
// exps and a log on it (measured: 1.7 us per frame at 3 states per lane in log space).  The clamp at -700 keeps a state of a feasible path
// above the smallest normal double.
NS2_DEVINL double al_emit(float x, double lse) { return exp(fmax((double)x - lse, -700.0)); }

// grid (B), 256 threads: A[b, t, s] for t < mel_len and nll[b] = -(K ln 2 + log(A[S - 1] + A[S - 2])) at the last frame, K = the sum of the
// exponents taken out (an integer: exact)
template <int NSJ>
__global__ __launch_bounds__(256) void al_alpha_kernel(const float* aln_log, const int* text_lens, const int* mel_lens, int T, int n,
                                                       float blank, const double* lse_fs, double* alpha, double* nll) {
  constexpr int SP = 256 * NSJ + 2;
  __shared__ double cs[2 * SP];
  __shared__ double wm[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = min(max(text_lens[b], 0), n), ml = min(max(mel_lens[b], 0), T), S = 2 * L + 1;
  if (tid < 2) { cs[tid] = 0.0; cs[SP + tid] = 0.0; }
  const float* xb = aln_log + (long)b * T * n;
  const double* sb = lse_fs + (long)b * T;
  double* ab = alpha + (long)b * T * (2 * n + 1);
  float xv[NSJ], xn[NSJ];
  double l = 0.0, ln = 0.0;
#pragma unroll
  for (int j = 0; j < NSJ; ++j) xn[j] = 0.f;
  auto loadx = [&](int t, float (&dst)[NSJ], double& lse) {
    lse = sb[t];
#pragma unroll
    for (int j = 0; j < NSJ; ++j) {
      const int s = tid + 256 * j;
      dst[j] = (s < S && (s & 1)) ? xb[(long)t * n + (s >> 1)] : blank;
    }
  };
  if (ml > 0) loadx(0, xv, l);
  long K = 0;
  __syncthreads();
  for (int t = 0; t < ml; ++t) {                       // ml is the workgroup's own: the same trips for every thread
    if (t + 1 < ml) loadx(t + 1, xn, ln);              // the next frame's loads fly during this frame's recursion
    double* cur = cs + ((t & 1) ? SP : 0) + 2;
    const double* prev = cs + ((t & 1) ? 0 : SP) + 2;
    double y[NSJ];
#pragma unroll
    for (int j = 0; j < NSJ; ++j) y[j] = al_emit(xv[j], l);
    int k = 0;
    if (t > 0) {
      const double* w = wm[(t & 1) ^ 1];
      frexp(fmax(fmax(w[0], w[1]), fmax(w[2], w[3])), &k);
      K += k;
    }
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < NSJ; ++j) {
      const int s = tid + 256 * j;
      double a;
      if (t == 0) a = s < 2 ? y[j] : 0.0;
      else a = ldexp((prev[s] + prev[s - 1] + ((s & 1) ? prev[s - 2] : 0.0)) * y[j], -k);
      if (s >= S) a = 0.0;
      cur[s] = a;
      mx = fmax(mx, a);
      if (s < S) ab[(long)t * (2 * n + 1) + s] = a;
    }
    mx = wave_max_d(mx);
    if ((tid & 63) == 0) wm[t & 1][tid >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NSJ; ++j) xv[j] = xn[j];
    l = ln;
  }
  if (tid == 0) {
    double r = L == 0 ? 0.0 : (double)__builtin_inff();  // no frame: feasible only for the empty target
    if (ml > 0) {
      const double* last = cs + (((ml - 1) & 1) ? SP : 0) + 2;
      r = -((double)K * 0.69314718055994530942 + log(last[S - 1] + last[S - 2]));     // last[-1] is the zero pad when S == 1; log(0) = -inf: infeasible
    }
    nll[b] = r;
  }
}

// grid (1), 256 threads: fs_loss = mean_b (nll_b / max(L_b, 1), 0 where infinite), bin_loss = sum of the rows' terms / B; fixed order
__global__ __launch_bounds__(256) void al_finish_kernel(const float* stats, const double* nll, const int* text_lens, int B, int T, int n,
                                                        float* fs_loss, float* bin_loss) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  for (int which = 0; which < 2; ++which) {
    float* out = which ? bin_loss : fs_loss;           // (uniform: the barriers below are reached by every thread or by none)
    if (!out) continue;
    double s = 0.0;
    if (which == 0) {
      for (int b = tid; b < B; b += 256) {
        const double v = nll[b];
        const int L = min(max(text_lens[b], 0), n);
        if (v < (double)__builtin_inff()) s += v / (double)max(L, 1);
      }
    } else {
      for (long r = tid; r < (long)B * T; r += 256) s += (double)stats[r * AL_STATS + 3];
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) *out = (float)(red[0] / (double)B);
    __syncthreads();
  }
}

// grid (ceil(T / AA_TQ), B), 256 threads: d_log <- the bin term g_bin (hard - softmax sum_i hard) / B on the columns <= L, 0 elsewhere
__global__ __launch_bounds__(256) void al_bin_bwd_kernel(const float* aln_log, const float* hard, const int* text_lens, const float* g_bin,
                                                         int B, int T, int n, const float* stats, float* d_log) {
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = min(max(text_lens[b], 0), n), Lb = (g_bin && hard) ? min(L + 1, n) : 0;
  const float sc = Lb ? g_bin[0] / (float)B : 0.f;
  for (int f = wv; f < AA_TQ && t0 + f < T; f += 4) {
    const int t = t0 + f;
    const long row = ((long)b * T + t) * n;
    const float lse = stats[((long)b * T + t) * AL_STATS + 1], hs = stats[((long)b * T + t) * AL_STATS + 2];
    for (int i = lane; i < n; i += 64) {
      float v = 0.f;
      if (i < Lb) v = sc * (hard[((long)b * n + i) * T + t] - expf(aln_log[row + i] - lse) * hs);
      d_log[row + i] = v;
    }
  }
}

// grid (B), 256 threads: the backward recursion over t = mel_len - 1 .. 0 in the same scaling: Bt_t(s) = the probability of the rest of the
// target from state s at frame t, the frame's own emission left out: Bt_t(s) = (W_{t+1}(s) + W_{t+1}(s + 1) [+ W_{t+1}(s + 2)]) 2^-k with
// W_t(s) = y_t(s) Bt_t(s) in LDS.  e[b, t, s] = A_t(s) Bt_t(s), proportional to the occupancy, goes to the workspace's second half.
// Nothing for an infeasible utterance (zero trips for the whole workgroup).
template <int NSJ>
__global__ __launch_bounds__(256) void al_beta_kernel(const float* aln_log, const int* text_lens, const int* mel_lens, int T, int n,
                                                      float blank, const double* lse_fs, const double* alpha, const double* nll, double* e) {
  constexpr int SP = 256 * NSJ + 2;
  __shared__ double cs[2 * SP];
  __shared__ double wm[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = min(max(text_lens[b], 0), n), S = 2 * L + 1;
  const int ml = nll[b] < (double)__builtin_inff() ? min(max(mel_lens[b], 0), T) : 0;
  if (tid < 2) { cs[SP - 2 + tid] = 0.0; cs[2 * SP - 2 + tid] = 0.0; }
  const float* xb = aln_log + (long)b * T * n;
  const double* sb = lse_fs + (long)b * T;
  const double* ab = alpha + (long)b * T * (2 * n + 1);
  double* eb = e + (long)b * T * (2 * n + 1);
  float xv[NSJ], xn[NSJ];
  double av[NSJ], an[NSJ], l = 0.0, ln = 0.0;
#pragma unroll
  for (int j = 0; j < NSJ; ++j) { xn[j] = 0.f; an[j] = 0.0; }
  auto loadx = [&](int t, float (&dst)[NSJ], double (&da)[NSJ], double& lse) {
    lse = sb[t];
#pragma unroll
    for (int j = 0; j < NSJ; ++j) {
      const int s = tid + 256 * j;
      dst[j] = (s < S && (s & 1)) ? xb[(long)t * n + (s >> 1)] : blank;
      da[j] = s < S ? ab[(long)t * (2 * n + 1) + s] : 0.0;
    }
  };
  if (ml > 0) loadx(ml - 1, xv, av, l);
  __syncthreads();
  for (int t = ml - 1; t >= 0; --t) {
    if (t > 0) loadx(t - 1, xn, an, ln);
    double* cur = cs + ((t & 1) ? SP : 0);
    const double* nxt = cs + ((t & 1) ? 0 : SP);
    double y[NSJ];
#pragma unroll
    for (int j = 0; j < NSJ; ++j) y[j] = al_emit(xv[j], l);
    int k = 0;
    if (t < ml - 1) {
      const double* w = wm[(t & 1) ^ 1];
      frexp(fmax(fmax(w[0], w[1]), fmax(w[2], w[3])), &k);
    }
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < NSJ; ++j) {
      const int s = tid + 256 * j;
      double bt;
      if (t == ml - 1) bt = (s == S - 1 || s == S - 2) ? 1.0 : 0.0;
      else bt = ldexp(nxt[s] + nxt[s + 1] + ((s & 1) ? nxt[s + 2] : 0.0), -k);
      if (s >= S) bt = 0.0;
      const double wv = y[j] * bt;
      cur[s] = wv;
      mx = fmax(mx, wv);
      if (s < S) eb[(long)t * (2 * n + 1) + s] = av[j] * bt;
    }
    mx = wave_max_d(mx);
    if ((tid & 63) == 0) wm[t & 1][tid >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NSJ; ++j) { xv[j] = xn[j]; av[j] = an[j]; }
    l = ln;
  }
}

// grid (ceil(T / AA_TQ), B), 256 threads, one wave per frame t < mel_len of a feasible utterance: the occupancies of a frame sum to 1
// over its S states, so occupancy(s) = e[s] / sum_s e[s] -- no scale, no nll enters.  d_log[b, t, i] += (softmax - occupancy of label i)
// scale on the live cells (the blank column's share is dropped), scale = g_fs / (max(L, 1) B).
__global__ __launch_bounds__(256) void al_fs_grad_kernel(const float* aln_log, const int* text_lens, const int* mel_lens, const float* g_fs,
                                                         int B, int T, int n, const double* lse_fs, const double* e, const double* nll,
                                                         float* d_log) {
  const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = min(max(text_lens[b], 0), n), S = 2 * L + 1;
  const int ml = nll[b] < (double)__builtin_inff() ? min(max(mel_lens[b], 0), T) : 0;
  const double scale = (double)g_fs[0] / ((double)max(L, 1) * (double)B);
  for (int f = wv; f < AA_TQ && t0 + f < ml; f += 4) {
    const int t = t0 + f;
    const double* er = e + ((long)b * T + t) * (2 * n + 1);
    double sum = 0.0;
    for (int s = lane; s < S; s += 64) sum += er[s];
    const double inv = 1.0 / wave_sum_d(sum);
    const long row = ((long)b * T + t) * n;
    const double lse = lse_fs[(long)b * T + t];
    for (int i = lane; i < L; i += 64)
      d_log[row + i] += (float)((exp((double)aln_log[row + i] - lse) - er[2 * i + 1] * inv) * scale);
  }
}

static inline int al_nsj(int n) { return (2 * n + 1 + 255) / 256; }

struct AlWs { float* stats; double* lse_fs; double* nll; double* alpha; double* e; };
static inline AlWs al_ws(void* workspace, int B, int T, int n) {
  AlWs w;
  w.stats = reinterpret_cast<float*>(workspace);
  w.lse_fs = reinterpret_cast<double*>(w.stats + al_stats_floats(B, T));
  w.nll = w.lse_fs + al_lse_floats(B, T) / 2;
  w.alpha = w.nll + al_nll_floats(B) / 2;
  w.e = w.alpha + (int64_t)B * T * (2 * n + 1);
  return w;
}

#define AL_BY_NSJ(kernel, nsj, ...)                                                                     \
  do {                                                                                                  \
    if (nsj <= 1) hipLaunchKernelGGL((kernel<1>), dim3(B), dim3(256), 0, s, __VA_ARGS__);               \
    else if (nsj <= 2) hipLaunchKernelGGL((kernel<2>), dim3(B), dim3(256), 0, s, __VA_ARGS__);          \
    else if (nsj <= 3) hipLaunchKernelGGL((kernel<3>), dim3(B), dim3(256), 0, s, __VA_ARGS__);          \
    else if (nsj <= 5) hipLaunchKernelGGL((kernel<5>), dim3(B), dim3(256), 0, s, __VA_ARGS__);          \
    else hipLaunchKernelGGL((kernel<9>), dim3(B), dim3(256), 0, s, __VA_ARGS__);                        \
  } while (0)

hipError_t launch_align_losses_fwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, int B, int T, int n,
                                   float blank, float* fs_loss, float* bin_loss, void* workspace, hipStream_t s) {
  if (B <= 0 || B > 65535 || T <= 0 || T > 8192 || n <= 0 || n > 1024 || (bin_loss && !hard)) return hipErrorInvalidValue;
  const AlWs w = al_ws(workspace, B, T, n);
  hipLaunchKernelGGL(al_rowstat_kernel, dim3((T + AA_TQ - 1) / AA_TQ, B), dim3(256), 0, s, aln_log, bin_loss ? hard : nullptr, text_lens, T,
                     n, blank, w.stats, fs_loss ? w.lse_fs : nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (fs_loss) {
    const int nsj = al_nsj(n);
    AL_BY_NSJ(al_alpha_kernel, nsj, aln_log, text_lens, mel_lens, T, n, blank, w.lse_fs, w.alpha, w.nll);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(al_finish_kernel, dim3(1), dim3(256), 0, s, w.stats, w.nll, text_lens, B, T, n, fs_loss, bin_loss);
  return hipGetLastError();
}

hipError_t launch_align_losses_bwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, const float* g_fs,
                                   const float* g_bin, int B, int T, int n, float blank, float* d_log, void* workspace, hipStream_t s) {
  if (B <= 0 || B > 65535 || T <= 0 || T > 8192 || n <= 0 || n > 1024 || (g_bin && !hard)) return hipErrorInvalidValue;
  const AlWs w = al_ws(workspace, B, T, n);
  const dim3 rows((T + AA_TQ - 1) / AA_TQ, B);
  hipLaunchKernelGGL(al_bin_bwd_kernel, rows, dim3(256), 0, s, aln_log, hard, text_lens, g_bin, B, T, n, w.stats, d_log);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !g_fs) return e;
  const int nsj = al_nsj(n);
  AL_BY_NSJ(al_beta_kernel, nsj, aln_log, text_lens, mel_lens, T, n, blank, w.lse_fs, w.alpha, w.nll, w.e);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(al_fs_grad_kernel, rows, dim3(256), 0, s, aln_log, text_lens, mel_lens, g_fs, B, T, n, w.lse_fs, w.e, w.nll, d_log);
  return hipGetLastError();
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
