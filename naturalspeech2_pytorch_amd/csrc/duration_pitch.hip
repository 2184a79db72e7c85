// The pieces of the DurationPitchPredictor (NS2:344-527) and of the text-conditioned sampling path (NS2:87-104, 164-175,
// 1449-1455, 1476-1483) that the GEMM kernels do not cover:
//   - GroupNorm(groups, C) + SiLU (+ residual) over token-major rows [B * n, C] (Block / ResnetBlock, NS2:346-400): a
//     statistics pass writing per-chunk partials to fixed slots, then an apply pass that combines them in a fixed order
//     (Chan et al.) -- deterministic and bit-reproducible, no atomics (the kernels: groupnorm_kernel.h, shared with ragged_front.hip);
//   - the length regulator (generate_mask_from_repeats + f0_to_coarse + expand_encodings): a gather plus one fp32 add, which
//     is what the reference's 0/1 mask einsum computes bit for bit;
//   - the to_pred heads (Linear(dim, 1) + ReLU, NS2:467-471) as a row dot product;
//   - for training the predictor (training/duration_pitch_pass.py): the backward of GroupNorm + SiLU, which recombines the forward's own
//     statistics slots (bit-equal mean and rstd) and sums in fixed slots like the forward, and the backward of the heads.
// The convolutions, RMSNorm and attention of the trunk are the existing GEMM / norm / attention kernels.
#include <hip/hip_runtime.h>

#include "ns2_common.h"
#include "ns2_host.h"
#include "groupnorm_kernel.h"

namespace ns2 {

// ---------------------------------------------------------------- GroupNorm + SiLU (NS2:346-369): the forward kernels are groupnorm_kernel.h

// ---------------------------------------------------------------- GroupNorm + SiLU backward (training the predictor)
// With xh = (x - mean) rstd, z = xh w + b, dz = dy silu'(z):   dbias_c = sum dz,  dweight_c = sum dz xh  (over utterances and rows),
// dxh = dz w,  s1 = sum dxh,  s2 = sum dxh xh  (per utterance and group, N = n cg values),  dx = rstd (dxh - s1 / N - xh s2 / N).
// s1 and s2 are the group's sums of w_c times the utterance's column sums of dz and dz xh, so ONE set of per-column partial sums serves the
// parameter gradients and the group sums.  Two passes like the forward: gn_bwd_cols_kernel writes the column sums of a chunk of rows to
// the chunk's own slot; ns2_reduce_slices' kernel adds the slots of an utterance, then the utterances, in a fixed order;
// gn_bwd_apply_kernel forms s1 / N, s2 / N per group (ascending columns) and dx.  No atomics: bit-reproducible.
// Both kernels stream float4s with a row's columns on consecutive lanes.
constexpr int COLS_THREADS = 256;
constexpr int GNB_ROWS = 32;              // rows per column-sum slot
constexpr int RDB_ROWS = 64;              // ... of the head backward

// The threads of a workgroup cover `qt` <= 256 float4 columns; COLS_THREADS / qt rows are in flight at once (row subgroup rsub).  Fold
// the NV accumulators of the row subgroups into subgroup 0 in subgroup order.
template <int NV>
NS2_DEVINL void fold_row_subgroups(float (&acc)[NV], float* lds, int rsub, int rows_par, int t, int qt, bool active) {
#pragma unroll
  for (int e = 0; e < NV; ++e)
    if (active) lds[e * COLS_THREADS + t] = acc[e];
  __syncthreads();
  if (active && rsub == 0)
    for (int j = 1; j < rows_par; ++j)
#pragma unroll
      for (int e = 0; e < NV; ++e) acc[e] += lds[e * COLS_THREADS + j * qt + t];
}

struct GnBwdArgs {
  const float* x; const float* dy; long lddy; const float* weight; const float* bias; const float4* part;
  float* slots;            // [B * rchunks][2][C]: column sums of dz xh | dz over the chunk's rows
  const float* colsum;     // [B][2][C]: the slots of an utterance added up
  float* dx;
  int B, n, C, groups, cg, nchunks, rchunks; float eps;
  const int* row_lens = nullptr;   // <true> kernels: rows per utterance, int32 [B] in device memory, clamped into [1, n]
};

// rows of utterance b that count: n, or its own length (gn_rows of the forward)
template <bool LENS>
NS2_DEVINL int gnb_rows(const GnBwdArgs& a, int b) {
  if constexpr (LENS) return min(max(a.row_lens[b], 1), a.n);
  return a.n;
}

NS2_DEVINL float silu_grad(float z) {
  const float sg = 1.0f / (1.0f + expf(-z));
  return sg * (1.0f + z * (1.0f - sg));
}

// grid (ceil(C / 1024), rchunks, B); dynamic LDS: 3 * groups floats.  <true>: the chunk's rows stop at the utterance's length -- a chunk
// wholly behind it reads nothing and writes a slot of zeros, the boundary chunk sums its rows before the length, so the slots that count
// are those of the utterance alone at n = its length, bit for bit (the reducer adds the zero slots behind them: x + 0 = x).
template <bool LENS>
__global__ __launch_bounds__(COLS_THREADS) void gn_bwd_cols_kernel(const GnBwdArgs a) {
  const int tile = blockIdx.x, rc = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  extern __shared__ float gs[];
  __shared__ float fold[8 * COLS_THREADS];
  float* sK = gs; float* sM = gs + a.groups; float* sR = gs + 2 * a.groups;
  for (int g = t; g < a.groups; g += COLS_THREADS)
    gn_group_stats(a.part, a.x, b, g, a.groups, a.nchunks, a.n, a.C, a.cg, a.eps, sK[g], sM[g], sR[g]);
  __syncthreads();
  const int qt = min(COLS_THREADS, (a.C >> 2) - tile * COLS_THREADS);
  const int rows_par = COLS_THREADS / qt;
  const int rsub = t / qt, cq = t - rsub * qt;
  const bool active = rsub < rows_par;
  const int c = (tile * COLS_THREADS + cq) * 4;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    const int g = c / a.cg;
    const float K = sK[g], m = sM[g], rs = sR[g];
    const float4 wv = *reinterpret_cast<const float4*>(a.weight + c);
    const float4 bv = *reinterpret_cast<const float4*>(a.bias + c);
    const float w[4] = {wv.x, wv.y, wv.z, wv.w}, bi[4] = {bv.x, bv.y, bv.z, bv.w};
    const int r1 = min(gnb_rows<LENS>(a, b), (rc + 1) * GNB_ROWS);
    for (int r = rc * GNB_ROWS + rsub; r < r1; r += rows_par) {
      const long row = (long)b * a.n + r;
      const float4 xv = *reinterpret_cast<const float4*>(a.x + row * a.C + c);
      const float4 gv = *reinterpret_cast<const float4*>(a.dy + row * a.lddy + c);
      const float x[4] = {xv.x, xv.y, xv.z, xv.w}, dy[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = ((x[e] - K) - m) * rs;
        const float dz = dy[e] * silu_grad(xh * w[e] + bi[e]);
        acc[e] += dz * xh;
        acc[4 + e] += dz;
      }
    }
  }
  fold_row_subgroups<8>(acc, fold, rsub, rows_par, t, qt, active);
  if (active && rsub == 0) {
    float* slot = a.slots + ((long)b * a.rchunks + rc) * 2 * a.C;
    *reinterpret_cast<float4*>(slot + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(slot + a.C + c) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

// grid (ceil(n / GN_APPLY_ROWS), B); dynamic LDS: 5 * groups floats.  <true>: N = len * cg; a row at or beyond the utterance's length is
// not read (x and dy may hold NaN there) and its dx is written as zeros.
template <bool LENS>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_apply_kernel(const GnBwdArgs a) {
  const int b = blockIdx.y, t = threadIdx.x;
  extern __shared__ float gs[];
  float* sK = gs; float* sM = gs + a.groups; float* sR = gs + 2 * a.groups; float* s1 = gs + 3 * a.groups; float* s2 = gs + 4 * a.groups;
  const int len = gnb_rows<LENS>(a, b);
  const float inv_n = 1.0f / ((float)len * (float)a.cg);
  for (int g = t; g < a.groups; g += GN_THREADS) {
    gn_group_stats(a.part, a.x, b, g, a.groups, a.nchunks, a.n, a.C, a.cg, a.eps, sK[g], sM[g], sR[g]);
    const float* cs = a.colsum + (long)b * 2 * a.C;
    float u = 0.f, v = 0.f;
    for (int c = g * a.cg; c < (g + 1) * a.cg; ++c) {        // a group has a few dozen columns: ascending order, one thread
      u += a.weight[c] * cs[a.C + c];
      v += a.weight[c] * cs[c];
    }
    s1[g] = u * inv_n;
    s2[g] = v * inv_n;
  }
  __syncthreads();
  const int r0 = blockIdx.x * GN_APPLY_ROWS;
  const int q = a.C >> 2;
  for (int it = t; it < GN_APPLY_ROWS * q; it += GN_THREADS) {
    const int r = r0 + it / q, c = (it % q) * 4;
    if (r >= len) break;                               // (rows ascend with `it`; <false>: len = n)
    const long row = (long)b * a.n + r;
    const int g = c / a.cg;
    const float4 xv = *reinterpret_cast<const float4*>(a.x + row * a.C + c);
    const float4 gv = *reinterpret_cast<const float4*>(a.dy + row * a.lddy + c);
    const float4 wv = *reinterpret_cast<const float4*>(a.weight + c);
    const float4 bv = *reinterpret_cast<const float4*>(a.bias + c);
    const float x[4] = {xv.x, xv.y, xv.z, xv.w}, dy[4] = {gv.x, gv.y, gv.z, gv.w};
    const float w[4] = {wv.x, wv.y, wv.z, wv.w}, bi[4] = {bv.x, bv.y, bv.z, bv.w};
    const float K = sK[g], m = sM[g], rs = sR[g], u = s1[g], v = s2[g];
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = ((x[e] - K) - m) * rs;
      const float dxh = dy[e] * silu_grad(xh * w[e] + bi[e]) * w[e];
      o[e] = rs * (dxh - u - xh * v);
    }
    *reinterpret_cast<float4*>(a.dx + row * a.C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
  if constexpr (LENS) {                                // a loop of its own: the one above keeps the <false> kernel's body, hence its bits
    for (int it = t; it < GN_APPLY_ROWS * q; it += GN_THREADS) {
      const int r = r0 + it / q, c = (it % q) * 4;
      if (r >= a.n) break;
      if (r >= len) *reinterpret_cast<float4*>(a.dx + ((long)b * a.n + r) * a.C + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// ---------------------------------------------------------------- to_pred heads, backward: out = relu(h . w + b)
// g = dout where out > 0 (the same rows as pre > 0), else 0;  dh[m, :] = g[m] w;  dw = sum_m g[m] h[m, :];  db = sum_m g[m].
// grid (ceil(K / 1024), ceil(M / RDB_ROWS)): slot [chunk][K + 1] = the chunk's dw | db; the slots are added in order by ns2_reduce_slices' kernel.
__global__ __launch_bounds__(COLS_THREADS) void row_dot_bwd_kernel(const float* dout, const float* out, const float* h, long ldh,
                                                                    const float* w, int M, int K, float* dh, long lddh, float* slots) {
  const int tile = blockIdx.x, chunk = blockIdx.y, t = threadIdx.x;
  __shared__ float fold[5 * COLS_THREADS];
  const int qt = min(COLS_THREADS, (K >> 2) - tile * COLS_THREADS);
  const int rows_par = COLS_THREADS / qt;
  const int rsub = t / qt, cq = t - rsub * qt;
  const bool active = rsub < rows_par;
  const int c = (tile * COLS_THREADS + cq) * 4;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    const float4 wv = *reinterpret_cast<const float4*>(w + c);
    const int m1 = min(M, (chunk + 1) * RDB_ROWS);
    for (int m = chunk * RDB_ROWS + rsub; m < m1; m += rows_par) {
      const float g = out[m] > 0.f ? dout[m] : 0.f;
      const float4 hv = *reinterpret_cast<const float4*>(h + (long)m * ldh + c);
      *reinterpret_cast<float4*>(dh + (long)m * lddh + c) = make_float4(g * wv.x, g * wv.y, g * wv.z, g * wv.w);
      acc[0] += g * hv.x; acc[1] += g * hv.y; acc[2] += g * hv.z; acc[3] += g * hv.w;
      acc[4] += g;
    }
  }
  fold_row_subgroups<5>(acc, fold, rsub, rows_par, t, qt, active);
  if (active && rsub == 0) {
    float* slot = slots + (long)chunk * (K + 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) slot[c + e] = acc[e];
    if (c == 0) slot[K] = acc[4];
  }
}

// ---------------------------------------------------------------- length regulator (NS2:87-104, 164-175, 1449-1455)
constexpr int LR_THREADS = 256;
constexpr int LR_TF = 64;                // frames per tile
constexpr int LR_TD = 32;                // channels per tile

// repeats.int() of a ReLU output; a negative duration (never produced by the predictor) counts as 0 frames
NS2_DEVINL int dur_frames(float d) { const int r = (int)d; return r > 0 ? r : 0; }

// f0_to_coarse (NS2:164-175) in the reference's fp32 operation order; mel_min / mel_max are the reference's fp32 constants
NS2_DEVINL int f0_coarse(float f0, float mel_min, float mel_max) {
#pragma clang fp contract(off)
  float m = 1127.0f * logf(1.0f + f0 / 700.0f);
  if (m > 0.f) m = (m - mel_min) * 254.0f / (mel_max - mel_min) + 1.0f;
  if (m <= 1.0f) m = 1.0f;
  if (m > 255.0f) m = 255.0f;
  const int c = (int)(m + 0.5f);
  return c < 1 ? 1 : (c > 255 ? 255 : c);          // NaN pitch: keep the table read in bounds
}

// inclusive prefix sum of the utterance's frame counts into cum[n_ph] (LDS or global), by the whole block; returns the total
NS2_DEVINL int block_cumsum(const float* dur, int n_ph, int* cum, int* part) {
  const int t = threadIdx.x;
  const int per = (n_ph + LR_THREADS - 1) / LR_THREADS;
  const int i0 = min(t * per, n_ph), i1 = min(i0 + per, n_ph);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += dur_frames(dur[i]);
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < LR_THREADS; o <<= 1) {         // Hillis-Steele over the 256 segment sums (integers: exact)
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (cum) {
    s = part[t] - s;                                 // exclusive prefix of this segment
    for (int i = i0; i < i1; ++i) { s += dur_frames(dur[i]); cum[i] = s; }
  }
  const int total = part[LR_THREADS - 1];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(LR_THREADS) void lr_totals_kernel(const float* dur, int n_ph, int* totals) {
  __shared__ int part[LR_THREADS];
  const int b = blockIdx.x;
  const int tot = block_cumsum(dur + (long)b * n_ph, n_ph, nullptr, part);
  if (threadIdx.x == 0) totals[b] = tot;
}

// grid (ceil(n_frames / LR_TF), ceil(D / LR_TD), B); dynamic LDS: cum[n_ph]
__global__ __launch_bounds__(LR_THREADS) void lr_expand_kernel(const float* dur, const float* pitch, const float* enc,
                                                               const float* table, int n_ph, int D, int n_frames, float mel_min,
                                                               float mel_max, float* out) {
  extern __shared__ int cum[];
  __shared__ int part[LR_THREADS];
  __shared__ int s_ph[LR_TF], s_co[LR_TF];
  __shared__ float tile[LR_TF][LR_TD + 1];
  const int b = blockIdx.z, f0 = blockIdx.x * LR_TF, d0 = blockIdx.y * LR_TD, t = threadIdx.x;
  const int total = block_cumsum(dur + (long)b * n_ph, n_ph, cum, part);
  if (t < LR_TF) {
    const int f = f0 + t;
    int ph = -1;
    if (f < total) {                                 // first phoneme whose inclusive prefix exceeds f
      int lo = 0, hi = n_ph - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > f) hi = mid; else lo = mid + 1;
      }
      ph = lo;
    }
    s_ph[t] = ph;
    s_co[t] = ph >= 0 ? f0_coarse(pitch[(long)b * n_ph + ph], mel_min, mel_max) : 0;
  }
  __syncthreads();
  // gather along channels (coalesced reads of enc / table rows) ...
  for (int i = t; i < LR_TF * LR_TD; i += LR_THREADS) {
    const int j = i / LR_TD, d = i % LR_TD;
    float v = 0.f;
    const int ph = s_ph[j];
    if (ph >= 0 && d0 + d < D)
      v = enc[((long)b * n_ph + ph) * D + d0 + d] + table[(long)s_co[j] * D + d0 + d];
    tile[j][d] = v;
  }
  __syncthreads();
  // ... and write along frames: out [B, D, n_frames]
  for (int i = t; i < LR_TF * LR_TD; i += LR_THREADS) {
    const int d = i / LR_TF, j = i % LR_TF;
    if (d0 + d < D && f0 + j < n_frames) out[((long)b * D + d0 + d) * n_frames + f0 + j] = tile[j][d];
  }
}

// ---------------------------------------------------------------- to_pred heads (NS2:467-471): one wave per row
__global__ __launch_bounds__(256) void row_dot_kernel(const float* x, int ldx, int M, int K, const float* w, const float* bias,
                                                      int relu, float* out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + row * ldx;
  float s = 0.f;
  for (int c = lane * 4; c < K; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(xr + c), b = *reinterpret_cast<const float4*>(w + c);
    s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  s = wave_sum(s);
  if (lane == 0) {
    if (bias) s += bias[0];
    out[row] = relu ? fmaxf(s, 0.f) : s;
  }
}

// ---- launchers of the training kernels (C entries: capi_train.cpp)
int gn_bwd_row_chunks(int n) { return (n + GNB_ROWS - 1) / GNB_ROWS; }
int row_dot_bwd_chunks(long M) { return (int)((M + RDB_ROWS - 1) / RDB_ROWS); }

// stats = the workspace the forward (ns2_groupnorm_silu) left; slots [B * gn_bwd_row_chunks(n)][2 C]; colsum [B][2 C]; dwb [2 C] = dweight | dbias.
// row_lens (include/ns2hip_train.h): int32 [B] on the device and stats = what ns2_groupnorm_silu_lens left, or nullptr: the
// <true> kernels in the same grids, the same two reductions between them.
hipError_t launch_groupnorm_silu_bwd(const float* dy, long lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                                     const float* bias, float eps, const void* stats, float* dx, float* dwb, float* slots, float* colsum,
                                     hipStream_t s, const int* row_lens) {
  if (B <= 0 || n <= 0 || groups <= 0 || groups > 1024 || C <= 0 || C % groups || (C / groups) % 4 || C / groups > GN_CHUNK || lddy < C ||
      (lddy & 3) || B > 65535)
    return hipErrorInvalidValue;
  GnBwdArgs a;
  a.x = x; a.dy = dy; a.lddy = lddy; a.weight = weight; a.bias = bias; a.part = reinterpret_cast<const float4*>(stats);
  a.slots = slots; a.colsum = colsum; a.dx = dx;
  a.B = B; a.n = n; a.C = C; a.groups = groups; a.cg = C / groups; a.nchunks = gn_chunks(n, a.cg); a.rchunks = gn_bwd_row_chunks(n);
  a.eps = eps; a.row_lens = row_lens;
  const int q = C >> 2;
  const dim3 cols_grid((q + COLS_THREADS - 1) / COLS_THREADS, a.rchunks, B);
  if (row_lens)
    hipLaunchKernelGGL(gn_bwd_cols_kernel<true>, cols_grid, dim3(COLS_THREADS), 3 * groups * sizeof(float), s, a);
  else
    hipLaunchKernelGGL(gn_bwd_cols_kernel<false>, cols_grid, dim3(COLS_THREADS), 3 * groups * sizeof(float), s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_reduce_slices(slots, B, a.rchunks, 2L * C, colsum, 0, s);          // per utterance: what the group sums need
  if (e != hipSuccess) return e;
  e = launch_reduce_slices(colsum, 1, B, 2L * C, dwb, 0, s);                    // over the utterances: dweight | dbias
  if (e != hipSuccess) return e;
  const dim3 apply_grid((n + GN_APPLY_ROWS - 1) / GN_APPLY_ROWS, B);
  if (row_lens)
    hipLaunchKernelGGL(gn_bwd_apply_kernel<true>, apply_grid, dim3(GN_THREADS), 5 * groups * sizeof(float), s, a);
  else
    hipLaunchKernelGGL(gn_bwd_apply_kernel<false>, apply_grid, dim3(GN_THREADS), 5 * groups * sizeof(float), s, a);
  return hipGetLastError();
}

// slots [row_dot_bwd_chunks(M)][K + 1]; dwb [K + 1] = dw | db
hipError_t launch_row_dot_relu_bwd(const float* dout, const float* out, const float* h, long ldh, const float* w, long M, int K, float* dh,
                                   long lddh, float* dwb, float* slots, hipStream_t s) {
  if (M <= 0 || M > 0x7fffffffL - RDB_ROWS || K <= 0 || (K & 3) || ldh < K || (ldh & 3) || lddh < K || (lddh & 3)) return hipErrorInvalidValue;
  const int chunks = row_dot_bwd_chunks(M);
  if (chunks > 65535) return hipErrorInvalidValue;
  const int q = K >> 2;
  hipLaunchKernelGGL(row_dot_bwd_kernel, dim3((q + COLS_THREADS - 1) / COLS_THREADS, chunks), dim3(COLS_THREADS), 0, s, dout, out, h, ldh, w,
                     (int)M, K, dh, lddh, slots);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_reduce_slices(slots, 1, chunks, (long)K + 1, dwb, 0, s);
}

}  // namespace ns2

using namespace ns2;

#define DP_HIPRET(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return NS2_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
#define DP_ARGCHK(cond, msg) \
  do {                       \
    if (!(cond)) {           \
      set_error("%s", msg);  \
      return NS2_ERR_ARG;    \
    }                        \
  } while (0)

extern "C" int64_t ns2_groupnorm_workspace_bytes(int B, int n, int C, int groups) {
  if (B <= 0 || n <= 0 || groups <= 0 || C <= 0 || C % groups) return 0;
  return (int64_t)B * groups * gn_chunks(n, C / groups) * (int64_t)sizeof(float4);
}

extern "C" int ns2_groupnorm_silu(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                                  const float* resid, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  GnArgs a;
  const int rc = gn_fill_args("ns2_groupnorm_silu", x, B, n, C, groups, weight, bias, eps, resid, out_f32, out_hi, out_lo, ldo, precision,
                              workspace, workspace_bytes, &a);
  if (rc != NS2_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel<false>, dim3(a.nchunks, groups, B), dim3(GN_THREADS), 0, s, a);
  DP_HIPRET(hipGetLastError());
  hipLaunchKernelGGL(gn_apply_kernel<false>, dim3((n + GN_APPLY_ROWS - 1) / GN_APPLY_ROWS, B), dim3(GN_THREADS),
                     3 * groups * sizeof(float), s, a);
  DP_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_length_regulate_totals(const float* duration, int B, int n_ph, int* totals, void* stream) {
  DP_ARGCHK(duration && totals && B > 0 && n_ph > 0, "ns2_length_regulate_totals: bad arguments");
  hipLaunchKernelGGL(lr_totals_kernel, dim3(B), dim3(LR_THREADS), 0, (hipStream_t)stream, duration, n_ph, totals);
  DP_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_length_regulate(const float* duration, const float* pitch, const float* enc, const float* pitch_table, int B,
                                   int n_ph, int D, int n_frames, float mel_min, float mel_max, float* out, void* stream) {
  DP_ARGCHK(duration && pitch && enc && pitch_table && out && B > 0 && n_ph > 0 && D > 0 && n_frames > 0,
            "ns2_length_regulate: bad arguments");
  DP_ARGCHK(n_ph <= 8192, "ns2_length_regulate: at most 8192 phonemes per utterance");
  hipLaunchKernelGGL(lr_expand_kernel, dim3((n_frames + LR_TF - 1) / LR_TF, (D + LR_TD - 1) / LR_TD, B), dim3(LR_THREADS),
                     (size_t)n_ph * sizeof(int), (hipStream_t)stream, duration, pitch, enc, pitch_table, n_ph, D, n_frames, mel_min,
                     mel_max, out);
  DP_HIPRET(hipGetLastError());
  return NS2_OK;
}

extern "C" int ns2_row_dot(const float* x, int ldx, int M, int K, const float* w, const float* bias, int relu, float* out, void* stream) {
  DP_ARGCHK(x && w && out && M > 0 && K > 0 && K % 4 == 0 && ldx % 4 == 0 && ldx >= K, "ns2_row_dot: bad arguments");
  DP_ARGCHK(((uintptr_t)x | (uintptr_t)w) % 16 == 0, "ns2_row_dot: x and w must be 16-byte aligned");
  hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, M, K, w, bias, relu, out);
  DP_HIPRET(hipGetLastError());
  return NS2_OK;
}
