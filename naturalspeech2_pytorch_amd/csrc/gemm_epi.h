// Epilogue layer of the GEMM kernels (gemm.hip: 128x128 tile, 64-row wave tiles; gemm2.hip and its lean relatives: 256x256 tile,
// 128-row wave tiles), three headers:
//   gemm_epi.h           (this file) the accumulator layout, the Wavenet gate between the K phases, the fused RMSNorm tail and the
//                        GENERIC epilogue: bounds, format and activation decided per stored value -- any tile, any alignment;
//   gemm_epi_fast.h      the STAGED epilogues of whole wave tiles: through the wave's private LDS region, 16-byte stores;
//   gemm_epi_dispatch.h  wave_tile_epilogue: the one place that decides between the two.
// A wave owns MI x 2 accumulator tiles of v_mfma_f32_32x32x16_bf16 (C layout: col = lane & 31, row = acc_row(r, lane >> 5)),
// rows [row_base, row_base + 32 * MI), cols [col_base, col_base + 64).  A row's stored bits do not depend on the path its tile took
// (tests/test_kernels_gpu.py, test_epilogue_paths_store_identical_bits), nor on the alignment or the strides of its destination, and no
// path stores outside the rectangle the call owns (tests/test_gemm_dest_gpu.py: sentinel arenas, every route).
#pragma once
#include "ns2_common.h"
#include "ns2_kernels.h"

namespace ns2 {

// row of accumulator register r inside its 32 x 32 tile (hi = lane >> 5)
NS2_DEVINL constexpr int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// value of lane ^ 1 (DPP quad_perm [1,0,3,2]): one VALU move, no LDS crossbar
NS2_DEVINL float lane_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

// Pair adjacent columns for 4-byte stores of two 16-bit values: a lane holds rows 2rp (v0) and 2rp + 1 (v1) of its column; afterwards
// the even lane holds row 2rp and the odd lane row 2rp + 1 of columns (l31 & ~1, l31 | 1) in (c_lo, c_hi).  Returns that row's
// accumulator register.  The exchange is the DPP move (staged epilogues) or a shuffle (generic epilogue): the same values.
template <bool DPP>
NS2_DEVINL int pair_cols(bool odd, int rp, float v0, float v1, float& c_lo, float& c_hi) {
  const float send = odd ? v0 : v1;
  const float recv = DPP ? lane_xor1(send) : __shfl_xor(send, 1, 64);
  c_lo = odd ? recv : v0;
  c_hi = odd ? v1 : recv;
  return 2 * rp + (odd ? 1 : 0);
}

// WavenetResBlock NS2:629-636: h = conv(x)+b ; h = h*gamma_t+beta_t ; h = tanh(h)*sigmoid(h) ; (then += res_conv(x)).
// tanh(h)*sigmoid(h) = sign(h) * (1-u) * (h<0 ? u : 1) / (1+u^2),  u = exp(-|h|)   (one exp, no overflow)
// `uni` (wave-uniform): the wave tile lies inside ONE utterance, so gamma / beta are per column and are loaded once per column tile
// instead of once per element (with a row / seq_len division each).  The per-element structure (one small diamond per value) is
// kept on purpose: a straight-line variant of this loop made the register allocator spill 100-300 VGPRs.
template <int MI, int NI>
NS2_DEVINL void wavenet_midgate(f32x16 (&acc)[MI][NI], const GemmArgs& g, int z, int row_base, int col_base, int l31, int hi, bool uni = false) {
  const float* film = g.film + (long)z * g.film_zs;
  const float* bias = g.bias + (long)z * g.bias_zs;
  const float* bias2 = g.bias2 + (long)z * g.bias_zs;
  const float* film_u = film + (long)(uni ? row_base / g.seq_len : 0) * g.film_ld;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int col = col_base + ni * 32 + l31;
      const bool cok = col < g.N;
      const float bc = cok ? bias[col] : 0.f;
      const float b2 = cok ? bias2[col] : 0.f;
      const float gam_u = (uni && cok) ? film_u[col] : 0.f;
      const float bet_u = (uni && cok) ? film_u[g.N + col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row_base + mi * 32 + acc_row(r, hi);
        float v = 0.f;
        if (cok && row < g.M) {
          float gam = gam_u, bet = bet_u;
          if (!uni) {
            const int b = row / g.seq_len;
            gam = film[(long)b * g.film_ld + col];
            bet = film[(long)b * g.film_ld + g.N + col];
          }
          const float h = (acc[mi][ni][r] + bc) * gam + bet;
          const float u = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(h));     // v_exp_f32: <= 1 ulp, |arg| error ~1e-7*|h|
          const float t = (1.f - u) * (h < 0.f ? u : 1.f) * __builtin_amdgcn_rcpf(1.f + u * u);
          v = copysignf(t, h) + b2;
        }
        acc[mi][ni][r] = v;
      }
    }
}

// The RMSNorm behind a residual update (GemmArgs::nrm_*), after the row's sum of squares `ss` is known: x = columns c .. c + 3 of row
// `row` of the N-column update, gm = gamma at those columns (read only with g.nrm_gamma).  One expression order for the fused
// 128x128 epilogue and the split-K finishing pass; rmsnorm_kernel (elementwise.hip) multiplies in another order.
NS2_DEVINL void norm_tail_store4(const GemmArgs& g, int N, long row, int c, const float4& x, float ss, const float (&gm)[4]) {
  const float inv = sqrtf((float)N) / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize eps (NS2:727-746)
  float o[4] = {x.x * inv, x.y * inv, x.z * inv, x.w * inv};
  if (g.nrm_gamma) { o[0] *= gm[0]; o[1] *= gm[1]; o[2] *= gm[2]; o[3] *= gm[3]; }
  if (g.nrm_cond) {
    const float* gc = g.nrm_cond + (g.nrm_seq_len > 0 ? row / g.nrm_seq_len : 0) * (long)g.nrm_cond_ld;
    const float4 t = *reinterpret_cast<const float4*>(gc + c), u = *reinterpret_cast<const float4*>(gc + N + c);
    o[0] = o[0] * t.x + u.x; o[1] = o[1] * t.y + u.y; o[2] = o[2] * t.z + u.z; o[3] = o[3] * t.w + u.w;
  }
  const bool nil = g.nrm_lo != nullptr;
  store_cols4(g.nrm_hi + row * pld(g.nrm_ld, nil), c, o[0], o[1], o[2], o[3], g.nrm_fmt, nil);
}
NS2_DEVINL void norm_gamma4(const GemmArgs& g, int c, float (&gm)[4]) {
  gm[0] = gm[1] = gm[2] = gm[3] = 1.f;
  if (g.nrm_gamma) { const float4 t = *reinterpret_cast<const float4*>(g.nrm_gamma + c); gm[0] = t.x; gm[1] = t.y; gm[2] = t.z; gm[3] = t.w; }
}

// ---- Ragged skipping in the training pass (GemmArgs::zero_hidden, include/ns2hip.h): a hidden tile of EVERY output
// of the product gets zero bits -- what the tile's epilogue would have covered, nothing else.  Zero bits are the value 0 in every
// format (fp32, bf16 hi / lo, IEEE half, the e5m2 bytes of FMT_H8).  Rows [row0, row0 + rows) lie inside one utterance and one skipping
// granule (the caller's tile height divides 256 and lens_seq % 256 == 0); col0 / bn: the tile's first (packed) column and its width, a
// multiple of 128.  Called by the whole workgroup on its early return; no barrier, no LDS.
// logical columns [c0, c1) (c0 % 32 == 0, c1 even) of the rows of split-plane matrix `hi` (interleaved lines when il)
NS2_DEVINL void zero_tile_planes(bf16_t* hi, int ld, bool il, int fmt, int row0, int rows, int c0, int c1, int tid, int nthreads) {
  if (rows <= 0 || c1 <= c0) return;
  const long rs = pld(ld, il);                                  // physical row stride, 16-bit elements
  const int c1w = il ? (c1 & ~31) : c1;                         // whole lines / the dense range: physically contiguous
  const int p0 = il ? 2 * c0 : c0, p1 = il ? 2 * c1w : c1w;     // physical element range of it
  bf16_t* base = hi + (long)row0 * rs;
  if (p1 > p0) {
    const bool v16 = ((reinterpret_cast<uintptr_t>(base + p0) & 15) == 0) && ((rs & 7) == 0) && (((p1 - p0) & 7) == 0);
    if (v16) {
      const int per = (p1 - p0) >> 3;
      for (int i = tid; i < rows * per; i += nthreads) {
        const int r = i / per;
        *reinterpret_cast<uint4*>(base + (long)r * rs + p0 + ((i - r * per) << 3)) = make_uint4(0u, 0u, 0u, 0u);
      }
    } else {
      const int per = (p1 - p0) >> 1;
      for (int i = tid; i < rows * per; i += nthreads) {
        const int r = i / per;
        *reinterpret_cast<uint32_t*>(base + (long)r * rs + p0 + ((i - r * per) << 1)) = 0u;
      }
    }
  }
  if (c1w < c1) {                                               // the started line of an interleaved matrix: column pairs, as store_cols2 addresses them
    const int per = (c1 - c1w) >> 1;
    for (int i = tid; i < rows * per; i += nthreads) {
      const int r = i / per, c = c1w + ((i - r * per) << 1);
      bf16_t* line = base + (long)r * rs + ((c & ~31) << 1);
      *reinterpret_cast<uint32_t*>(line + (c & 31)) = 0u;
      if (fmt == FMT_H8) {
        unsigned char* bytes = reinterpret_cast<unsigned char*>(line) + 64 + (c & 31);
        *reinterpret_cast<uint16_t*>(bytes) = 0; *reinterpret_cast<uint16_t*>(bytes + 32) = 0;
      } else {
        *reinterpret_cast<uint32_t*>(line + 32 + (c & 31)) = 0u;
      }
    }
  }
}
template <int EPI>
NS2_DEVINL void zero_hidden_tile(const GemmArgs& g, int z, int row0, int rows, int col0, int bn, int tid, int nthreads) {
  if constexpr (EPI == EPI_F32) {
    zero_tile_f32(g.out_f + z * g.out_f_zs, g.ldo_f, row0, rows, col0, min(bn, g.N - col0), tid, nthreads);
  } else {
    const bool il = g.out_lo != nullptr;
    bf16_t* out_hi = g.out_hi + pcol((int)(z * g.out_zs), il);
    if constexpr (EPI == EPI_GEGLU) {                           // packed [x 32 | gate 32] column blocks -> 32 output columns each
      zero_tile_planes(out_hi, g.ldo_s, il, g.out_fmt, row0, rows, col0 >> 1, min((col0 + bn) >> 1, g.out_ncols), tid, nthreads);
    } else {
      zero_tile_planes(out_hi, g.ldo_s, il, g.out_fmt, row0, rows, col0, min(col0 + bn, g.out_ncols), tid, nthreads);
      if constexpr (EPI == EPI_QKV) {                           // V^T[b][feature][n]: 4 tokens per store, as the epilogue writes them
        const int f0 = max(col0, g.split_col) - g.split_col, f1 = min(col0 + bn, g.N) - g.split_col;
        if (f1 > f0 && g.seq_len > 0 && rows >= 4) {
          const bool vil = g.vt_lo != nullptr;
          const int b = row0 / g.seq_len, n0 = row0 - b * g.seq_len, per = rows >> 2;
          for (int i = tid; i < (f1 - f0) * per; i += nthreads) {
            const int f = i / per, n = n0 + ((i - f * per) << 2);
            const long o = ((long)b * g.vt_rows + f0 + f) * pld(g.vt_ld, vil) + pcol(n, vil);
            *reinterpret_cast<uint2*>(g.vt_hi + o) = make_uint2(0u, 0u);
            if (vil) *reinterpret_cast<uint2*>(g.vt_lo + o) = make_uint2(0u, 0u);
          }
        }
      }
    }
  }
}

// The generic epilogue.  ocol_base: first output column of this wave for EPI_GEGLU (= half of the packed column index)
template <int EPI, int MI>
NS2_DEVINL void gemm_epilogue(f32x16 (&acc)[MI][2], const GemmArgs& g, int z, int row_base, int col_base, int ocol_base, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  const bool odd = lane & 1;
  const bool il = g.out_lo != nullptr;               // interleaved 128-B output lines: bf16 [hi32|lo32] or FMT_H8 (ns2_common.h)

  if constexpr (EPI == EPI_F32) {
    // out = acc + bias (+ residual)      (to_out / FF-out / final_conv / to_pred)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = col_base + ni * 32 + l31;
        if (col >= g.N) continue;
        const float bc = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row_base + mi * 32 + acc_row(r, hi);
          if (row >= g.M) continue;
          float v = acc[mi][ni][r] + bc;
          if (g.act) v = apply_act(v, g.act);
          if (g.resid) v += g.resid[(long)row * g.ldr + col];
          g.out_f[z * g.out_f_zs + (long)row * g.ldo_f + col] = v;
        }
      }
  } else if constexpr (EPI == EPI_GEGLU) {
    // wave tile = [x(32 cols) | gate(32 cols)] ; out[:, ocol] = gelu(gate) * x   (NS2:1006-1007)
    const int col = (ocol_base + l31) & ~1;
    const float bx = g.bias[col_base + l31], bg = g.bias[col_base + 32 + l31];      // packed (padded) bias: always in range
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int rp = 0; rp < 8; ++rp) {
        const float v0 = gelu_erf(acc[mi][1][2 * rp] + bg) * (acc[mi][0][2 * rp] + bx);
        const float v1 = gelu_erf(acc[mi][1][2 * rp + 1] + bg) * (acc[mi][0][2 * rp + 1] + bx);
        float c_lo, c_hi;
        const int row = row_base + mi * 32 + acc_row(pair_cols<false>(odd, rp, v0, v1, c_lo, c_hi), hi);
        if (row < g.M && col < g.out_ncols) store_cols2(g.out_hi + (long)row * pld(g.ldo_s, il), col, c_lo, c_hi, g.out_fmt, il);
      }
    }
  } else {
    // EPI_SPLIT / EPI_QKV / EPI_WAVENET: split planes, optionally the tail columns transposed (V^T for attention)
    const float* bias = g.bias ? g.bias + (long)z * g.bias_zs : nullptr;
    const long zo = pcol((int)(z * g.out_zs), il);    // out_zs = logical column offset of slice z
    bf16_t* out_hi = g.out_hi + zo;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = col_base + ni * 32 + l31;
        float bc = 0.f;
        if constexpr (EPI != EPI_WAVENET) bc = (bias && col < g.N) ? bias[col] : 0.f;   // wavenet biases were applied mid-loop
        const bool transposed = (EPI == EPI_QKV) && (col_base + ni * 32 >= g.split_col);   // wave-uniform
        if (!transposed) {
#pragma unroll
          for (int rp = 0; rp < 8; ++rp) {
            float v0 = acc[mi][ni][2 * rp] + bc, v1 = acc[mi][ni][2 * rp + 1] + bc;
            if (EPI == EPI_SPLIT && g.act) { v0 = apply_act(v0, g.act); v1 = apply_act(v1, g.act); }
            float c_lo, c_hi;
            const int row = row_base + mi * 32 + acc_row(pair_cols<false>(odd, rp, v0, v1, c_lo, c_hi), hi);
            const int c0 = col & ~1;
            if (row < g.M && c0 < g.out_ncols) {
              if (c0 >= g.N) c_lo = 0.f;             // zero the K-padding columns of the next GEMM's operand
              if (c0 + 1 >= g.N) c_hi = 0.f;
              store_cols2(out_hi + (long)row * pld(g.ldo_s, il), c0, c_lo, c_hi, g.out_fmt, il);
            }
          }
        } else {
          // V^T[b][feature][n]: this lane owns feature `col - split_col` and 4 consecutive tokens per register group
          const int feat = col - g.split_col;
          if (col < g.N) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int row0 = row_base + mi * 32 + acc_row(4 * gq, hi);
              if (row0 >= g.M) continue;
              const int b = row0 / g.seq_len, n0 = row0 - b * g.seq_len;
              // transposed values are attention operands: bf16 (with or without lo plane) or dense IEEE half, never FMT_H8
              uint32_t h01, l01, h23, l23;
              split2f(acc[mi][ni][4 * gq + 0] + bc, acc[mi][ni][4 * gq + 1] + bc, h01, l01, g.vt_fmt == FMT_F16);
              split2f(acc[mi][ni][4 * gq + 2] + bc, acc[mi][ni][4 * gq + 3] + bc, h23, l23, g.vt_fmt == FMT_F16);
              const bf16_t h[4] = {(bf16_t)(h01 & 0xffffu), (bf16_t)(h01 >> 16), (bf16_t)(h23 & 0xffffu), (bf16_t)(h23 >> 16)};
              const bf16_t l[4] = {(bf16_t)(l01 & 0xffffu), (bf16_t)(l01 >> 16), (bf16_t)(l23 & 0xffffu), (bf16_t)(l23 >> 16)};
              const bool vil = g.vt_lo != nullptr;
              const long o = ((long)b * g.vt_rows + feat) * pld(g.vt_ld, vil) + pcol(n0, vil);
              if ((g.seq_len & 3) == 0) {            // 4 tokens stay inside one utterance (and one 32-block), 8-B aligned
                *reinterpret_cast<uint2*>(g.vt_hi + o) = make_uint2(h01, h23);
                if (vil) *reinterpret_cast<uint2*>(g.vt_lo + o) = make_uint2(l01, l23);
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int row = row0 + e;
                  if (row < g.M) {
                    const int bb = row / g.seq_len, nn = row - bb * g.seq_len;
                    const long oo = ((long)bb * g.vt_rows + feat) * pld(g.vt_ld, vil) + pcol(nn, vil);
                    g.vt_hi[oo] = h[e];
                    if (vil) g.vt_lo[oo] = l[e];
                  }
                }
              }
            }
          }
        }
      }
  }
}

}  // namespace ns2
