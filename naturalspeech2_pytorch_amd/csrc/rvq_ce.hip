// RVQ cross-entropy of the training loss (NS2:1668-1684, `codec.rq(x_start, codes)`) on gfx950, forward and unit gradient in one launch.
// Per quantizer q the logits of a row are the NEGATIVE Euclidean distances of its running residual r to the C codes, the loss is
// lse_c(-dist_c) + dist_target, and the residual loses its nearest code (detached).  Nothing of size [rows, C] ever exists: the walk is
// rvq_encode_kernel's (rvq.hip) -- 16 residual rows per wave in registers across all stages, 64-code tiles through a double-buffered LDS
// ring, r.e - |e|^2/2 on the fp32 MFMA as D[code][row] -- with an online log-sum-exp next to the running arg-max, and, when the gradient
// is wanted, a SECOND sweep over the stage's codebook that recomputes dist, forms w_c = (softmax_c - onehot_c) / dist_c and accumulates
//     dL/dr = -(sum_c w_c) r + sum_c w_c e_c .
// The second sum is a [rows, C] x [C, 128] product on the same MFMA: the D[code][row] accumulator (lane = row, register i = code 4 g + i)
// IS the B operand of v_mfma_f32_16x16x4_f32 contracting the codes {i, 4 + i, 8 + i, 12 + i}, and the A operand E[code 4 g + i][k] comes
// from the same LDS tile, so w never leaves its lane.  r_{q+1} = r_q - nearest.detach(), hence dL/dx = sum_q dL/dr_q; the kernel writes
// G = (1 / M) sum_q dL/dr_q (each stage's loss is a mean over the M rows).  Everything is fp32, no atomics, every sum in a fixed order:
// loss and G are bit-reproducible.
//
// Edge behaviour (also in include/ns2hip_train.h):
//   * target outside [0, C) (-1 included): that row's loss and its row of G are NaN -- loud, and no host read;
//   * dist == 0 (the residual IS a code): the loss is the well-defined value, that code's w_c is 0;
//   * near-ties of the nearest code are not re-decided in fp64 (rvq_encode_kernel does): either code is a valid stage result.
// Distances: the sweeps use the expanded form |r|^2 - 2 (r.e - |e|^2/2) clamped at 0 (what the MFMA yields, and what the PyTorch
// composite computes); the target's own distance -- the term the loss is most sensitive to -- is the direct form sum (r - e)^2.
//
// Ragged batches (ns2_rvq_ce_lens, include/ns2hip_train.h): the same kernel instantiated on RvqCeLensArgs.  A row at or behind its
// utterance's length is a DEAD row: its x and its targets are not read (the residual starts at 0, the target is code 0, so nothing of it
// is NaN), its rows of row_loss and G are stored as 0, and a workgroup of dead rows alone returns before the first codebook tile.  A live
// row's arithmetic is unchanged (rows never mix: a row is one column of every MFMA), and its G is divided by B len instead of M.  The
// instantiations on RvqCeArgs are the kernels as they were.
#include <type_traits>

#include "ns2_common.h"
#include "ns2_kernels.h"

namespace ns2 {

constexpr int RC_D = 128;
constexpr int RC_ROWF = RC_D + 4;                 // padded LDS row (floats), as rvq.hip
constexpr int RC_TILE = 64;                       // codes per tile
constexpr int RC_STAGE_F = RC_TILE * RC_ROWF + RC_TILE;   // tile + its 64 half-norms
constexpr int RC_ROWS = 128;                      // rows per workgroup: 8 waves x 16 rows

// Lane (l15 = lane & 15, g = lane >> 4) owns row l15 and the 32 feature columns K(g, s) = 16 g + s (s < 16), 64 + 16 g + (s - 16) (s >= 16):
// the contraction slots of the first product AND the output columns of the second (there the MFMA output row m = 4 g + reg is column
// 4 m + kt, resp. 64 + 4 m + (kt - 4), of k-tile kt, so that a lane reads its A operands as two conflict-free 16-byte LDS loads).
NS2_DEVINL int rc_col(int g, int s) { return (s < 16 ? 0 : 48) + 16 * g + s; }

// the length of the utterance that owns `row` (< B n), clamped into [1, n], and the row's place in it
NS2_DEVINL bool rc_row_live(const RvqCeLensArgs& a, long row, int* len) {
  const long b = row / a.n;
  *len = min(max(a.row_lens[b], 1), a.n);
  return row - b * a.n < *len;
}

template <bool GRAD, typename Args>
__global__ __launch_bounds__(512, 2) void rvq_ce_kernel(const Args a) {
  constexpr bool LENS = std::is_same<Args, RvqCeLensArgs>::value;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const long row = (long)blockIdx.x * RC_ROWS + wave * 16 + l15;
  bool row_ok = row < a.M;
  if constexpr (LENS) {
    const bool in_batch = row_ok;
    int len;
    row_ok = in_batch && rc_row_live(a, row, &len);
    if (in_batch && !row_ok) {                                                   // a dead row: its outputs, and nothing else of it
      if (g == 0)
        for (int q = 0; q < a.Q; ++q) a.row_loss[row * a.Q + q] = 0.f;
      if constexpr (GRAD) {
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) *reinterpret_cast<float4*>(a.grad + row * RC_D + rc_col(g, 4 * s4)) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    if (!__syncthreads_or((int)row_ok)) return;                                  // no live row in this workgroup: no codebook tile
  }

  float rf[32];                                   // rf[s] = r[row][K(g, s)]
#pragma unroll
  for (int s4 = 0; s4 < 8; ++s4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok) v = *reinterpret_cast<const float4*>(a.x + row * RC_D + rc_col(g, 4 * s4));
    rf[4 * s4] = v.x; rf[4 * s4 + 1] = v.y; rf[4 * s4 + 2] = v.z; rf[4 * s4 + 3] = v.w;
  }
  // gacc[kt][r] = sum over the stages of dL/dr[row][K(g, s)], s = 4 r + kt (kt < 4), 16 + 4 r + (kt - 4) (kt >= 4)
  f32x4 gacc[8];
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) gacc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntile = a.C / RC_TILE;
  constexpr int NSWEEP = GRAD ? 2 : 1;
  struct TileRegs { f32x4 v[4]; float nrm; };
  auto load_tile = [&](TileRegs& tr, int q, int ct) {
    const float* src = a.codebooks + ((long)q * a.C + (long)ct * RC_TILE) * RC_D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 512 * i;
      tr.v[i] = *reinterpret_cast<const f32x4*>(src + (long)(c >> 5) * RC_D + (c & 31) * 4);
    }
    tr.nrm = (tid < RC_TILE) ? a.cb_norm[(long)q * a.C + ct * RC_TILE + tid] : 0.f;
  };
  auto store_tile = [&](const TileRegs& tr, int sidx) {
    float* base = lds + sidx * RC_STAGE_F;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 512 * i;
      *reinterpret_cast<f32x4*>(base + (c >> 5) * RC_ROWF + (c & 31) * 4) = tr.v[i];
    }
    if (tid < RC_TILE) base[RC_TILE * RC_ROWF + tid] = tr.nrm;
  };

  // ONE stream of tiles through the ring over (stage, sweep, tile): buffer = it & 1, the next tile is fetched while this one is used
  TileRegs tr;
  load_tile(tr, 0, 0);
  store_tile(tr, 0);
  __syncthreads();
  int it = 0;

  for (int q = 0; q < a.Q; ++q) {
    const float* cbq = a.codebooks + (long)q * a.C * RC_D;
    // |r|^2 of the row, the same bits in its four lanes (a symmetric butterfly)
    float rn = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) rn = fmaf(rf[s], rf[s], rn);
    rn = __fadd_rn(rn, __shfl_xor(rn, 16, 64));
    rn = __fadd_rn(rn, __shfl_xor(rn, 32, 64));

    // the target and its distance in direct form
    long tgt = row_ok ? (long)a.targets[row * a.Q + q] : 0;
    const bool tgt_ok = tgt >= 0 && tgt < a.C;
    if (!tgt_ok) tgt = -1;
    float dist_t;
    {
      const float* et = cbq + (tgt_ok ? tgt : 0) * RC_D;
      float d2 = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) {
        const float4 v = *reinterpret_cast<const float4*>(et + rc_col(g, 4 * s4));
        const float t0 = rf[4 * s4] - v.x, t1 = rf[4 * s4 + 1] - v.y, t2 = rf[4 * s4 + 2] - v.z, t3 = rf[4 * s4 + 3] - v.w;
        d2 = fmaf(t0, t0, d2); d2 = fmaf(t1, t1, d2); d2 = fmaf(t2, t2, d2); d2 = fmaf(t3, t3, d2);
      }
      d2 = __fadd_rn(d2, __shfl_xor(d2, 16, 64));
      d2 = __fadd_rn(d2, __shfl_xor(d2, 32, 64));
      dist_t = tgt_ok ? sqrtf(d2) : __builtin_nanf("");
    }

    float best_v = -INFINITY; int best_i = 0;     // running nearest code: max of r.e - |e|^2/2, first maximum in code order
    float mx = -INFINITY, se = 0.f;               // online log-sum-exp of -dist over this lane's codes
    float lse = 0.f, sw = 0.f;                    // sweep 2: the row's log-sum-exp, this lane's sum of w_c

    for (int sweep = 0; sweep < NSWEEP; ++sweep) {
      for (int ct = 0; ct < ntile; ++ct, ++it) {
        // the tile after this one in the stream
        int nq = q, nct = ct + 1;
        if (nct == ntile) { nct = 0; if (sweep + 1 == NSWEEP) nq = q + 1; }
        const bool more = nq < a.Q;
        if (more) load_tile(tr, nq, nct);
        const float* tb = lds + (it & 1) * RC_STAGE_F;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {                                       // two pairs of 16-code groups per tile
          f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
          const float* e0 = tb + ((2 * cp) * 16 + l15) * RC_ROWF;              // A operand: E[code = l15][K(g, s)]
          const float* e1 = e0 + 16 * RC_ROWF;
#pragma unroll
          for (int s4 = 0; s4 < 8; ++s4) {
            const float4 x0 = *reinterpret_cast<const float4*>(e0 + rc_col(g, 4 * s4));
            const float4 x1 = *reinterpret_cast<const float4*>(e1 + rc_col(g, 4 * s4));
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, rf[4 * s4 + 0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, rf[4 * s4 + 0], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, rf[4 * s4 + 1], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, rf[4 * s4 + 1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, rf[4 * s4 + 2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, rf[4 * s4 + 2], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, rf[4 * s4 + 3], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, rf[4 * s4 + 3], acc1, 0, 0, 0);
          }
          // lane (row l15, group g) register i of code group cg is code  ct*64 + cg*16 + 4 g + i  (increasing in cg, i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int cg = 2 * cp + h;
            const float4 n4 = *reinterpret_cast<const float4*>(tb + RC_TILE * RC_ROWF + cg * 16 + 4 * g);
            const float nb[4] = {n4.x, n4.y, n4.z, n4.w};
            const f32x4 acc = h ? acc1 : acc0;
            const int code0 = ct * RC_TILE + cg * 16 + 4 * g;
            float sc[4], dist[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              sc[i] = __fsub_rn(acc[i], nb[i]);                                // r.e - |e|^2/2
              dist[i] = sqrtf(fmaxf(fmaf(-2.f, sc[i], rn), 0.f));              // |r - e|, expanded form
            }
            if (sweep == 0) {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (sc[i] > best_v) { best_v = sc[i]; best_i = code0 + i; }
              const float lo = fminf(fminf(dist[0], dist[1]), fminf(dist[2], dist[3]));
              const float mn = fmaxf(mx, -lo);
              float add = __fadd_rn(__fadd_rn(expf(-dist[0] - mn), expf(-dist[1] - mn)), __fadd_rn(expf(-dist[2] - mn), expf(-dist[3] - mn)));
              se = __fadd_rn(__fmul_rn(se, expf(mx - mn)), add);
              mx = mn;
            } else if constexpr (GRAD) {
              f32x4 w;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const bool is_t = (long)(code0 + i) == tgt;
                const float d = is_t ? dist_t : dist[i];
                const float p = expf(-d - lse);
                const float wi = d > 0.f ? (p - (is_t ? 1.f : 0.f)) / d : 0.f;
                w[i] = wi;
                sw += wi;
              }
              // sum_c w_c e_c: B = w[i] (codes {4 g + i}), A = E[code 4 g + i][column of output row l15 in k-tile kt]
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float* ea = tb + (cg * 16 + 4 * g + i) * RC_ROWF + 4 * l15;
                const float4 a0 = *reinterpret_cast<const float4*>(ea);
                const float4 a1 = *reinterpret_cast<const float4*>(ea + 64);
                gacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, w[i], gacc[0], 0, 0, 0);
                gacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, w[i], gacc[1], 0, 0, 0);
                gacc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, w[i], gacc[2], 0, 0, 0);
                gacc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, w[i], gacc[3], 0, 0, 0);
                gacc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, w[i], gacc[4], 0, 0, 0);
                gacc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, w[i], gacc[5], 0, 0, 0);
                gacc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, w[i], gacc[6], 0, 0, 0);
                gacc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, w[i], gacc[7], 0, 0, 0);
              }
            }
          }
        }
        if (more) store_tile(tr, (it + 1) & 1);
        __syncthreads();
      }

      if (sweep == 0) {
        // merge the four lane groups of the row (disjoint code sets): two butterfly steps; every step is symmetric in the two partners,
        // so the four lanes end with the same bits
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
          const float pv = __shfl_xor(best_v, off, 64);
          const int pi = __shfl_xor(best_i, off, 64);
          if (pv > best_v || (pv == best_v && pi < best_i)) { best_v = pv; best_i = pi; }
          const float pm = __shfl_xor(mx, off, 64), ps = __shfl_xor(se, off, 64);
          const float mn = fmaxf(mx, pm);
          se = __fadd_rn(__fmul_rn(se, expf(mx - mn)), __fmul_rn(ps, expf(pm - mn)));
          mx = mn;
        }
        lse = __fadd_rn(mx, logf(se));
        if (row_ok && g == 0) {
          a.row_loss[row * a.Q + q] = __fadd_rn(lse, dist_t);                  // lse - (-dist_target); NaN for a target outside [0, C)
          if (a.nearest) a.nearest[row * a.Q + q] = (int64_t)best_i;
        }
      }
    }

    if constexpr (GRAD) {
      sw = __fadd_rn(sw, __shfl_xor(sw, 16, 64));
      sw = __fadd_rn(sw, __shfl_xor(sw, 32, 64));
      if (!tgt_ok) sw = __builtin_nanf("");
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          gacc[kt][r] = fmaf(-sw, rf[(kt < 4 ? 0 : 16) + 4 * r + (kt & 3)], gacc[kt][r]);
    }

    // residual -= E[nearest]
    const float* esel = cbq + (long)best_i * RC_D;
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      const float4 v = *reinterpret_cast<const float4*>(esel + rc_col(g, 4 * s4));
      rf[4 * s4 + 0] -= v.x; rf[4 * s4 + 1] -= v.y; rf[4 * s4 + 2] -= v.z; rf[4 * s4 + 3] -= v.w;
    }
  }

  if constexpr (GRAD) {
    if (row_ok) {
      float m = (float)a.M;
      if constexpr (LENS) {
        int len;
        rc_row_live(a, row, &len);
        m = (float)(a.B * len);                                                // <= M
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<float4*>(a.grad + row * RC_D + rc_col(g, 16 * hf + 4 * r)) =
              make_float4(gacc[4 * hf][r] / m, gacc[4 * hf + 1][r] / m, gacc[4 * hf + 2][r] / m, gacc[4 * hf + 3][r] / m);
    }
  }
}

// loss = sum_q mean_m row_loss[m][q]: one workgroup, fp64 partial sums per thread in index order, then a fixed tree
__global__ __launch_bounds__(1024) void rvq_ce_reduce_kernel(const float* row_loss, long n, int M, float* loss) {
  __shared__ double part[1024];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 1024) s += (double)row_loss[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(part[0] / (double)M);
}

// loss = (1 / B) sum_b (1 / len_b) sum_{t < len_b} sum_q row_loss[b][t][q]: one workgroup; per utterance a thread sums its part of the
// utterance's own len_b Q contiguous values in index order and adds it, divided by len_b, to its fp64 partial sum; then a fixed tree
__global__ __launch_bounds__(1024) void rvq_ce_reduce_lens_kernel(const float* row_loss, const int* row_lens, int B, int n, int Q, float* loss) {
  __shared__ double part[1024];
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const int len = min(max(row_lens[b], 1), n);
    const float* r = row_loss + (long)b * n * Q;
    double u = 0.0;
    for (long i = threadIdx.x; i < (long)len * Q; i += 1024) u += (double)r[i];
    s += u / (double)len;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(part[0] / (double)B);
}

// rvq_decode_kernel (rvq.hip) with lengths: the same sum in the same order for a live row, 0 and no read of `codes` for a dead one
__global__ void rvq_ce_decode_lens_kernel(const int64_t* codes, const float* cb, float* emb, const int* row_lens, int B, int n, int Q, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * n * RC_D) return;
  const long m = i / RC_D;
  const int k = (int)(i - m * RC_D);
  const long b = m / n;
  float acc = 0.f;
  if (m - b * n < min(max(row_lens[b], 1), n))
    for (int q = 0; q < Q; ++q) {
      const long c = codes[m * Q + q];
      acc += cb[((long)q * C + c) * RC_D + k];
    }
  emb[i] = acc;
}

template <typename Args>
static hipError_t launch_rvq_ce_main(const Args& a, hipStream_t s) {
  if (a.M <= 0 || a.Q <= 0 || a.D != RC_D || a.C <= 0 || (a.C % RC_TILE)) return hipErrorInvalidValue;
  if (a.quantized_out && !a.nearest) return hipErrorInvalidValue;
  const size_t lds = 2 * RC_STAGE_F * sizeof(float);
  const dim3 grid((a.M + RC_ROWS - 1) / RC_ROWS);
  if (a.grad) {
    static DynLdsAttr attr;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&rvq_ce_kernel<true, Args>), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rvq_ce_kernel<true, Args>), grid, dim3(512), lds, s, a);
  } else {
    static DynLdsAttr attr;
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&rvq_ce_kernel<false, Args>), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rvq_ce_kernel<false, Args>), grid, dim3(512), lds, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_rvq_ce_lens(const RvqCeLensArgs& a, hipStream_t s) {
  if (!a.row_lens || a.B <= 0 || a.n <= 0 || (long)a.B * a.n != (long)a.M) return hipErrorInvalidValue;
  hipError_t e = launch_rvq_ce_main(a, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rvq_ce_reduce_lens_kernel, dim3(1), dim3(1024), 0, s, a.row_loss, a.row_lens, a.B, a.n, a.Q, a.loss);
  e = hipGetLastError();
  if (e != hipSuccess || !a.quantized_out) return e;
  const long n = (long)a.M * RC_D;
  hipLaunchKernelGGL(rvq_ce_decode_lens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.nearest, a.codebooks, a.quantized_out,
                     a.row_lens, a.B, a.n, a.Q, a.C);
  return hipGetLastError();
}

hipError_t launch_rvq_ce(const RvqCeArgs& a, hipStream_t s) {
  hipError_t e = launch_rvq_ce_main(a, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rvq_ce_reduce_kernel, dim3(1), dim3(1024), 0, s, a.row_loss, (long)a.M * a.Q, a.M, a.loss);
  e = hipGetLastError();
  if (e != hipSuccess || !a.quantized_out) return e;
  return launch_rvq_decode(a.nearest, a.codebooks, a.quantized_out, a.M, a.Q, a.C, a.D, s);
}

}  // namespace ns2
