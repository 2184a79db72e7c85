// GroupNorm(groups, C) + SiLU (+ residual) over token-major rows [B * n, C] (Block / ResnetBlock, NS2:346-400): the forward kernels,
// shared by duration_pitch.hip (<false>: every utterance has n rows -- ns2_groupnorm_silu and the training backward, which recombines
// the forward's slots) and ragged_front.hip (<true>: a row count per utterance, GnArgs::row_lens -- ns2_groupnorm_silu_lens).
// A statistics pass writes per-chunk partials to fixed slots, then an apply pass combines them in a fixed order (Chan et al.):
// deterministic and bit-reproducible, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "ns2_common.h"
#include "ns2_host.h"

namespace ns2 {

// Statistics of one (utterance, group) are taken over n x cg values (cg = C / groups), relative to a shift K = the group's
// first value in the utterance: for activations with a large common offset (mean 100, std 1) x - K is exact and the
// partials stay small, so neither the mean nor the variance loses digits to cancellation (no E[x^2] - E[x]^2 anywhere).
constexpr int GN_THREADS = 256;
constexpr int GN_PER_THREAD = 16;
constexpr int GN_CHUNK = GN_THREADS * GN_PER_THREAD;     // values per partial slot
constexpr int GN_APPLY_ROWS = 16;

static inline int gn_chunk_rows(int cg) { return cg >= GN_CHUNK ? 1 : GN_CHUNK / cg; }
static inline int gn_chunks(int n, int cg) { return (n + gn_chunk_rows(cg) - 1) / gn_chunk_rows(cg); }

struct Welford { float n, mean, m2; };

// Chan, Golub & LeVeque: merge two (count, mean, M2) summaries; a is the earlier one in the fixed combine order
NS2_DEVINL Welford chan(const Welford& a, const Welford& b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
  return Welford{n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

struct GnArgs {
  const float* x; const float* weight; const float* bias; const float* resid;
  float* out_f; bf16_t* out_hi; bf16_t* out_lo; int ldo; int fmt;
  float4* part; int B, n, C, groups, cg, chunk_rows, nchunks; float eps;
  const int* row_lens = nullptr;          // <true> kernels: rows per utterance, int32 [B] in device memory, clamped into [1, n]
};

// rows of utterance b that count: n, or its own length.  Row 0 is always among them, so K = x[b, 0, g * cg] stays the shift.
template <bool LENS>
NS2_DEVINL int gn_rows(const GnArgs& a, int b) {
  if constexpr (LENS) return min(max(a.row_lens[b], 1), a.n);
  return a.n;
}

// grid (nchunks, groups, B): slot (b, g, chunk) <- (count, mean, M2) of the chunk's values minus K.  <true>: a chunk wholly behind the
// utterance's length writes count 0 (chan() skips it) and the boundary chunk takes the rows before the length, so the slots that
// count are those of the utterance alone at n = its length, bit for bit.
template <bool LENS>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const GnArgs a) {
  const int chunk = blockIdx.x, g = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const float* xb = a.x + (long)b * a.n * a.C + (long)g * a.cg;
  const float K = xb[0];
  const int r0 = chunk * a.chunk_rows;
  const int rows = max(min(a.chunk_rows, gn_rows<LENS>(a, b) - r0), 0);
  const int total = rows * a.cg;
  float v[GN_PER_THREAD];
  int cnt = 0;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < GN_PER_THREAD; ++i) {
    const int idx = t + GN_THREADS * i;
    v[i] = 0.f;
    if (idx < total) {
      const int r = idx / a.cg, c = idx - r * a.cg;
      v[i] = xb[(long)(r0 + r) * a.C + c] - K;
      s += v[i];
      ++cnt;
    }
  }
  Welford w{(float)cnt, 0.f, 0.f};
  if (cnt > 0) {
    w.mean = s / (float)cnt;
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < GN_PER_THREAD; ++i)
      if (t + GN_THREADS * i < total) { const float d = v[i] - w.mean; m2 += d * d; }
    w.m2 = m2;
  }
  // fixed tree inside the wave (lane l takes lane l + o), then the four waves in order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Welford p{__shfl_down(w.n, o, 64), __shfl_down(w.mean, o, 64), __shfl_down(w.m2, o, 64)};
    if ((t & 63) + o < 64 && ((t & 63) & (2 * o - 1)) == 0) w = chan(w, p);
  }
  __shared__ Welford wv[GN_THREADS / 64];
  if ((t & 63) == 0) wv[t >> 6] = w;
  __syncthreads();
  if (t == 0) {
    Welford r = wv[0];
    for (int i = 1; i < GN_THREADS / 64; ++i) r = chan(r, wv[i]);
    a.part[((long)b * a.groups + g) * a.nchunks + chunk] = make_float4(r.n, r.mean, r.m2, 0.f);
  }
}

// (shift, shifted mean, rstd) of group g of utterance b from the statistics slots, combined in slot order.  The ONE place that does it:
// the forward's apply pass and both passes of the backward call it, so the backward normalises with the forward's bits.
NS2_DEVINL void gn_group_stats(const float4* part, const float* x, int b, int g, int groups, int nchunks, int n, int C, int cg, float eps,
                               float& K, float& mean, float& rstd) {
  const float4* p = part + ((long)b * groups + g) * nchunks;
  Welford w{p[0].x, p[0].y, p[0].z};
  for (int i = 1; i < nchunks; ++i) w = chan(w, Welford{p[i].x, p[i].y, p[i].z});
  K = x[(long)b * n * C + (long)g * cg];
  mean = w.mean;
  rstd = 1.0f / sqrtf(w.m2 / w.n + eps);           // biased variance, as nn.GroupNorm
}

// grid (ceil(n / GN_APPLY_ROWS), B): y = silu((x - mean) * rstd * weight + bias) (+ resid), fp32 and / or operand planes.  <true>: a row
// at or beyond the utterance's length is not read (it may hold NaN, and so may its residual) and comes out as zeros, fp32 and planes.
template <bool LENS>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const GnArgs a) {
  const int b = blockIdx.y, t = threadIdx.x;
  extern __shared__ float gs[];           // [groups] shift, [groups] shifted mean, [groups] rstd
  float* sK = gs; float* sM = gs + a.groups; float* sR = gs + 2 * a.groups;
  for (int g = t; g < a.groups; g += GN_THREADS)
    gn_group_stats(a.part, a.x, b, g, a.groups, a.nchunks, a.n, a.C, a.cg, a.eps, sK[g], sM[g], sR[g]);
  __syncthreads();
  const int r0 = blockIdx.x * GN_APPLY_ROWS;
  const int q = a.C >> 2;                          // float4 columns per row
  const bool il = a.out_lo != nullptr || a.fmt == FMT_H8;
  const int len = gn_rows<LENS>(a, b);
  for (int it = t; it < GN_APPLY_ROWS * q; it += GN_THREADS) {
    const int r = r0 + it / q, c = (it % q) * 4;
    if (r >= a.n) break;
    const long row = (long)b * a.n + r;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!LENS || r < len) {
      const int g = c / a.cg;                      // cg % 4 == 0: the four columns share a group
      const float4 xv = *reinterpret_cast<const float4*>(a.x + row * a.C + c);
      const float4 wv = *reinterpret_cast<const float4*>(a.weight + c);
      const float4 bv = *reinterpret_cast<const float4*>(a.bias + c);
      const float K = sK[g], m = sM[g], rs = sR[g];
      o[0] = ((xv.x - K) - m) * rs * wv.x + bv.x; o[1] = ((xv.y - K) - m) * rs * wv.y + bv.y;
      o[2] = ((xv.z - K) - m) * rs * wv.z + bv.z; o[3] = ((xv.w - K) - m) * rs * wv.w + bv.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = siluf(o[e]);
      if (a.resid) {
        const float4 rv = *reinterpret_cast<const float4*>(a.resid + row * a.C + c);
        o[0] += rv.x; o[1] += rv.y; o[2] += rv.z; o[3] += rv.w;
      }
    }
    if (a.out_f) *reinterpret_cast<float4*>(a.out_f + row * a.C + c) = make_float4(o[0], o[1], o[2], o[3]);
    if (a.out_hi) store_cols4(a.out_hi + row * pld(a.ldo, il), c, o[0], o[1], o[2], o[3], a.fmt, il);
  }
}

// What ns2_groupnorm_silu and ns2_groupnorm_silu_lens refuse, before any device call, and the kernels' block of what they accept.
// `who`: the entry's name, the first word of the message.  Returns NS2_OK or NS2_ERR_ARG (the last error is set).
inline int gn_fill_args(const char* who, const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                        const float* resid, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* workspace,
                        int64_t workspace_bytes, GnArgs* out) {
#define GN_ARGCHK(cond, msg)            \
  do {                                  \
    if (!(cond)) {                      \
      set_error("%s: %s", who, msg);    \
      return NS2_ERR_ARG;               \
    }                                   \
  } while (0)
  GN_ARGCHK(x && weight && bias && (out_f32 || out_hi) && B > 0 && n > 0 && groups > 0 && groups <= 1024, "bad arguments");
  GN_ARGCHK(C > 0 && C % groups == 0 && (C / groups) % 4 == 0, "C / groups must be a multiple of 4");
  GN_ARGCHK(precision >= 1 && precision <= 4, "precision must be 1 .. 4");
  GN_ARGCHK(!out_hi || (C % 32 == 0 && ldo == C), "plane output needs C % 32 == 0 and ldo == C");
  GN_ARGCHK(precision != 2 || !out_lo, "precision 2 (fp16) has no lo plane");
  GN_ARGCHK(precision != 3 || !out_hi || out_lo, "precision 3 planes need the lo plane");
  GN_ARGCHK(workspace && workspace_bytes >= (int64_t)B * groups * gn_chunks(n, C / groups) * (int64_t)sizeof(float4), "workspace too small");
  GN_ARGCHK(((uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)resid | (uintptr_t)out_f32 | (uintptr_t)workspace) % 16 == 0,
            "fp32 buffers must be 16-byte aligned");
  GN_ARGCHK(C / groups <= GN_CHUNK, "C / groups must be at most 4096");
#undef GN_ARGCHK
  GnArgs a;
  a.x = x; a.weight = weight; a.bias = bias; a.resid = resid; a.out_f = out_f32;
  a.out_hi = reinterpret_cast<bf16_t*>(out_hi); a.out_lo = reinterpret_cast<bf16_t*>(out_lo); a.ldo = ldo;
  a.fmt = precision == 2 ? FMT_F16 : (precision == 4 ? FMT_H8 : FMT_BF16);
  a.part = reinterpret_cast<float4*>(workspace);
  a.B = B; a.n = n; a.C = C; a.groups = groups; a.cg = C / groups; a.chunk_rows = gn_chunk_rows(a.cg);
  a.nchunks = gn_chunks(n, a.cg); a.eps = eps;
  *out = a;
  return NS2_OK;
}

}  // namespace ns2
