// The STAGED epilogues (gemm_epi.h lists the epilogue layer's three headers): a whole wave tile -- 32 * MI rows x 64 columns, all valid,
// destination 16-byte aligned -- leaves through the wave's private LDS region, free after the K loop (the fp32 one also has a
// bounds-checked form for the 256x256 family's edge tiles).
//
// Why: the generic epilogue of gemm_epi.h tests `row < M && col < N` per store, picks the plane format per store at run time,
// bumps the saturation counter with one branch + atomic per converted pair, exchanges lanes through ds_bpermute and stores
// 2-4 bytes per lane.  The block timeline (tools/trace_blocks.py, profiles/r03_block_timeline_*.txt) showed every epilogue
// type at 15-19 us per block whatever it wrote (64 KiB ... 256 KiB): ~20k mostly-scalar instructions with ~600 branches --
// as long as the whole K loop of a K = 512 GEMM in the single-product modes.  Here:
//   * the plane format is a template parameter, bounds are checked once per wave (gemm_epi_dispatch.h);
//   * the range guard of the IEEE-half formats is a running max + NaN flag per lane, ONE atomic per lane at the end;
//   * adjacent columns are paired with a DPP quad permute (no LDS crossbar round trip);
//   * the tile is transposed through LDS and leaves as 16-byte stores: one wave-instruction writes whole 128-B / 256-B row
//     segments (the vector-memory path costs ~40-60 cycles per wave-instruction whatever its width; 4-byte stores were 4-12x
//     as many instructions);
//   * V^T (EPI_QKV) is transposed in LDS too: 256 contiguous bytes per feature row instead of 8-byte scattered stores.
// Results are bit-identical to the generic path: the same conversions (ns2_common.h) and the same gelu_erf on the same values.
#pragma once
#include <type_traits>

#include "gemm_epi.h"

namespace ns2 {

constexpr int EPI_LDS_WAVE_BYTES = 18432;     // a wave's region in the 256x256 family: 128 rows x (128 B + 16 B pad)

enum FastPlaneFmt : int { PF_F16 = 0, PF_BF16IL = 1, PF_H8 = 2, PF_BF16 = 3 };
template <int PF> struct PlaneGeom {
  static constexpr bool il = (PF == PF_BF16IL || PF == PF_H8);     // interleaved 128-B lines of 32 logical columns
  static constexpr int bytes_per_col32 = il ? 128 : 64;            // global bytes of 32 logical columns of one row
  static constexpr float limit = (PF == PF_H8) ? H8_MAX : 65504.f;
  static constexpr bool guarded = (PF == PF_F16 || PF == PF_H8);   // formats with the IEEE-half range
};

// range guard of the IEEE-half formats (ns2_common.h): a running max and a NaN flag per lane, one atomic at the end
struct RangeTrack {
  float mx = 0.f;
  bool nan = false;
  NS2_DEVINL void see(float a, float b) {
    mx = fmaxf(mx, fmaxf(fabsf(a), fabsf(b)));
    nan = nan || (a != a) || (b != b);
  }
  NS2_DEVINL void flush(float limit) {
    if (nan || !(mx <= limit)) atomicAdd(&ns2_sat_counter, 1u);
  }
};

// two adjacent logical columns (c even, 0 <= c < 64 inside the wave tile) of one staged LDS row, in global byte order
template <int PF>
NS2_DEVINL void lds_put2(unsigned char* rowp, int c, float v0, float v1, RangeTrack& rt) {
  if constexpr (PF == PF_F16) {
    rt.see(v0, v1);
    *reinterpret_cast<uint32_t*>(rowp + c * 2) = cvt2h_q(v0, v1);
  } else if constexpr (PF == PF_BF16) {
    *reinterpret_cast<uint32_t*>(rowp + c * 2) = cvt2(v0, v1);
  } else if constexpr (PF == PF_BF16IL) {
    uint32_t ph, pl;
    split2(v0, v1, ph, pl);
    unsigned char* line = rowp + (c >> 5) * 128 + (c & 31) * 2;
    *reinterpret_cast<uint32_t*>(line) = ph;
    *reinterpret_cast<uint32_t*>(line + 64) = pl;
  } else {
    rt.see(v0, v1);
    uint32_t h16, h8, l8;
    cvt2_h8_q(v0, v1, h16, h8, l8);
    unsigned char* line = rowp + (c >> 5) * 128;
    *reinterpret_cast<uint32_t*>(line + (c & 31) * 2) = h16;
    *reinterpret_cast<uint16_t*>(line + 64 + (c & 31)) = (uint16_t)h8;
    *reinterpret_cast<uint16_t*>(line + 96 + (c & 31)) = (uint16_t)l8;
  }
}

// staged rows -> global: ROWS rows of ROWB bytes (LDS row stride ROWB + 16), 16 bytes per lane, whole row segments per instruction
template <int ROWB, int ROWS>
NS2_DEVINL void lds_flush_rows(const unsigned char* wbuf, unsigned char* gbase, long row_stride_bytes, int lane) {
  constexpr int LPR = ROWB / 16, RPI = 64 / LPR, RS = ROWB + 16;
  static_assert(ROWS % RPI == 0, "row count must be a multiple of the rows per store instruction");
  const int lr0 = lane / LPR, ch = lane % LPR;
#pragma unroll
  for (int it = 0; it < ROWS / RPI; ++it) {
    const int lr = it * RPI + lr0;
    const uint4 v = *reinterpret_cast<const uint4*>(wbuf + lr * RS + ch * 16);
    *reinterpret_cast<uint4*>(gbase + (long)lr * row_stride_bytes + ch * 16) = v;
  }
}

// ---- split planes: EPI_SPLIT (bias; calls with an activation keep the generic path), EPI_WAVENET (biases were applied mid-loop), the q / k part of EPI_QKV
// MI = 32-row accumulator tiles of the wave (4: gemm2.hip's 128 x 64 wave tile, 2: gemm.hip's 64 x 64), WBUF = bytes of the wave's
// private LDS region: the tile leaves in passes of the most rows (a power of two, at least 32) that fit it.
template <int PF, bool BIAS_ACT, int MI = 4, int WBUF = 18432>
NS2_DEVINL void epi_planes_fast(f32x16 (&acc)[MI][2], const GemmArgs& g, int z, int row_base, int col_base, int lane, unsigned char* wbuf) {
  using G = PlaneGeom<PF>;
  constexpr int ROWB = 2 * G::bytes_per_col32;            // 64 columns of one row
  constexpr int RS = ROWB + 16;
  constexpr int RPP = (32 * MI * RS <= WBUF) ? 32 * MI : ((16 * MI * RS <= WBUF) ? 16 * MI : 32);   // rows per pass
  static_assert(RPP * RS <= WBUF && RPP >= 32 && (32 * MI) % RPP == 0, "the wave's LDS region holds at least one 32-row pass");
  const int l31 = lane & 31, hi = lane >> 5;
  const bool odd = lane & 1;
  float bc[2] = {0.f, 0.f};
  if constexpr (BIAS_ACT) {
    if (g.bias) {
      const float* bias = g.bias + (long)z * g.bias_zs;
      bc[0] = bias[col_base + l31];
      bc[1] = bias[col_base + 32 + l31];
    }
  }
  const long rsb = pld(g.ldo_s, G::il) * 2;
  unsigned char* gbase = reinterpret_cast<unsigned char*>(g.out_hi + pcol((int)(z * g.out_zs), G::il)) + (long)row_base * rsb +
                         (long)(col_base >> 5) * G::bytes_per_col32;
  RangeTrack rt;
#pragma unroll
  for (int pass = 0; pass < 32 * MI / RPP; ++pass) {
#pragma unroll
    for (int mh = 0; mh < RPP / 32; ++mh) {
      const int mi = pass * (RPP / 32) + mh;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int rp = 0; rp < 8; ++rp) {
          const float v0 = acc[mi][ni][2 * rp] + bc[ni], v1 = acc[mi][ni][2 * rp + 1] + bc[ni];
          float c_lo, c_hi;
          const int lr = mh * 32 + acc_row(pair_cols<true>(odd, rp, v0, v1, c_lo, c_hi), hi);
          lds_put2<PF>(wbuf + lr * RS, ni * 32 + (l31 & ~1), c_lo, c_hi, rt);
          if ((rp & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // keep the live set small: this code runs at the VGPR cap
        }
    }
    __builtin_amdgcn_wave_barrier();
    lds_flush_rows<ROWB, RPP>(wbuf, gbase + (long)pass * RPP * rsb, rsb, lane);
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (G::guarded) rt.flush(G::limit);
}

// ---- V^T of EPI_QKV: the wave tile's 64 value features x 128 tokens, transposed in LDS, 256 contiguous bytes per feature row.
// Dense 16-bit formats only (F16: IEEE half with the range guard, else bf16); needs seq_len % 128 == 0 (one utterance per tile).
// (MI = 32-token accumulator tiles of the wave: 4 in gemm2.hip, needs seq_len % 128 == 0; 2 in gemm.hip, seq_len % 64 == 0)
template <bool F16, int MI = 4>
NS2_DEVINL void epi_vt_fast(f32x16 (&acc)[MI][2], const GemmArgs& g, int row_base, int col_base, int lane, unsigned char* wbuf) {
  constexpr int TOKB = 64 * MI;                      // bytes of the wave tile's 32 * MI tokens in one feature row
  constexpr int RS = TOKB + 16;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = row_base / g.seq_len, n0 = row_base - b * g.seq_len;
  const int feat0 = col_base - g.split_col;
  RangeTrack rt;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const float a0 = acc[mi][ni][4 * gq + 0], a1 = acc[mi][ni][4 * gq + 1], a2 = acc[mi][ni][4 * gq + 2], a3 = acc[mi][ni][4 * gq + 3];
        uint32_t p01, p23;
        if constexpr (F16) { rt.see(a0, a1); rt.see(a2, a3); p01 = cvt2h_q(a0, a1); p23 = cvt2h_q(a2, a3); }
        else { p01 = cvt2(a0, a1); p23 = cvt2(a2, a3); }
        const int tok = mi * 32 + acc_row(4 * gq, hi);
        *reinterpret_cast<uint2*>(wbuf + (ni * 32 + l31) * RS + tok * 2) = make_uint2(p01, p23);
        if (gq == 3) __builtin_amdgcn_sched_barrier(0);
      }
  __builtin_amdgcn_wave_barrier();
  unsigned char* gbase = reinterpret_cast<unsigned char*>(g.vt_hi + ((long)b * g.vt_rows + feat0) * g.vt_ld + n0);
  lds_flush_rows<TOKB, 64>(wbuf, gbase, (long)g.vt_ld * 2, lane);
  __builtin_amdgcn_wave_barrier();
  if constexpr (F16) rt.flush(65504.f);
}

// ---- GEGLU: wave tile = [x(32 cols) | gate(32 cols)] -> 32 output columns gelu(gate) * x
template <int PF, int MI = 4>
NS2_DEVINL void epi_geglu_fast(f32x16 (&acc)[MI][2], const GemmArgs& g, int row_base, int col_base, int ocol_base, int lane, unsigned char* wbuf) {
  using G = PlaneGeom<PF>;
  constexpr int ROWB = G::bytes_per_col32;
  constexpr int RS = ROWB + 16;
  const int l31 = lane & 31, hi = lane >> 5;
  const bool odd = lane & 1;
  const float bx = g.bias[col_base + l31], bg = g.bias[col_base + 32 + l31];      // packed (padded) bias: always in range
  const long rsb = pld(g.ldo_s, G::il) * 2;
  unsigned char* gbase = reinterpret_cast<unsigned char*>(g.out_hi) + (long)row_base * rsb + (long)(ocol_base >> 5) * G::bytes_per_col32;
  RangeTrack rt;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int rp = 0; rp < 8; ++rp) {
      float v0 = gelu_erf(acc[mi][1][2 * rp] + bg) * (acc[mi][0][2 * rp] + bx);
      float v1 = gelu_erf(acc[mi][1][2 * rp + 1] + bg) * (acc[mi][0][2 * rp + 1] + bx);
      asm volatile("" : "+v"(v0), "+v"(v1));      // finish this pair before the next one starts: keeps the live set small
      float c_lo, c_hi;
      const int lr = mi * 32 + acc_row(pair_cols<true>(odd, rp, v0, v1, c_lo, c_hi), hi);
      lds_put2<PF>(wbuf + lr * RS, l31 & ~1, c_lo, c_hi, rt);
      if ((rp & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  __builtin_amdgcn_wave_barrier();
  lds_flush_rows<ROWB, 32 * MI>(wbuf, gbase, rsb, lane);
  __builtin_amdgcn_wave_barrier();
  if constexpr (G::guarded) rt.flush(G::limit);
}

// ---- fp32 (+ bias, activation, residual): LDS rows of 64 fp32 + 16 B pad, read back as float4 -- whole row segments per store instruction
constexpr int F32_RS = 272;

// accumulator tiles [mi0, mi0 + NT) of the wave, + bias (bc0 / bc1: the lane's two columns) and activation -> 32 * NT staged rows
template <int NT, int MI>
NS2_DEVINL void f32_stage_rows(const f32x16 (&acc)[MI][2], int mi0, float bc0, float bc1, int act, int lane, unsigned char* wbuf) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int mh = 0; mh < NT; ++mh)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = acc[mi0 + mh][ni][r] + (ni ? bc1 : bc0);
        if (act) t = apply_act(t, act);
        *reinterpret_cast<float*>(wbuf + (mh * 32 + acc_row(r, hi)) * F32_RS + (ni * 32 + l31) * 4) = t;
      }
}

// ROWS staged rows -> rows row0 ... of out_f, + residual: 2^lcpr 16-byte chunks per row (16 = all 64 columns), 64 >> lcpr rows per store
// instruction.  LCPR: lcpr at compile time (the loop unrolls), 0 = at run time.  EDGE: rows and columns are tested against M and N, a
// ragged last chunk goes value by value.  rr: the array of this lane's residual chunks loaded ahead by the caller, or nullptr (loaded
// here).  after(it, lr, v): what a caller keeps of the stored chunk v of staged row lr.
template <int ROWS, int LCPR, bool EDGE, class RR, class After>
NS2_DEVINL void f32_store_rows(const GemmArgs& g, int z, int row0, int col_base, int lcpr, int lane, const unsigned char* wbuf, const RR& rr,
                               After&& after) {
  const int lr0 = lane >> lcpr, ch = lane & ((1 << lcpr) - 1), rpi = 64 >> lcpr;
  const int col = col_base + ch * 4;
  // the lane's part of every address once; what an iteration adds is the same for the whole wave (a scalar offset)
  const long r0 = row0 + lr0;
  float* const obase = g.out_f + z * g.out_f_zs + r0 * g.ldo_f + col;
  const long roff = r0 * g.ldr + col;
  auto body = [&](int it) __attribute__((always_inline)) {
    const int lr = it * rpi + lr0;
    float4 v = *reinterpret_cast<const float4*>(wbuf + lr * F32_RS + ch * 16);
    float* const o = obase + (long)it * rpi * g.ldo_f;
    if constexpr (EDGE) {
      if (!(row0 + lr < g.M && col < g.N)) return;
      if (col + 3 >= g.N) {
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < g.N) o[e] = g.resid ? x[e] + g.resid[roff + (long)it * rpi * g.ldr + e] : x[e];
        return;
      }
    }
    if (g.resid) {
      float4 t;
      if constexpr (std::is_null_pointer_v<RR>) t = *reinterpret_cast<const float4*>(g.resid + roff + (long)it * rpi * g.ldr);
      else t = rr[it];
      v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    *reinterpret_cast<float4*>(o) = v;
    after(it, lr, v);
  };
  if constexpr (LCPR != 0) {
#pragma unroll
    for (int it = 0; it < (ROWS >> (6 - LCPR)); ++it) body(it);
  } else {                                            // run-time trip count: an unroll request would ask for a run-time unrolled loop with a remainder
    for (int it = 0; it < (ROWS >> (6 - lcpr)); ++it) body(it);
  }
}

// The staged fp32 epilogue of one wave tile in passes of 16 * MI rows (what the wave's LDS share holds in every kernel: 64 rows of
// the 256x256 family's 18 KiB, 32 rows of the 128x128 kernel's 10 KiB).  LCPR, EDGE: see f32_store_rows; nvc: valid columns of the
// tile (LCPR == 0: a power of two >= 16).  A whole interior tile (LCPR = 4, no EDGE) issues a pass's residual loads before the pass
// is staged: they fly meanwhile.
template <int MI, int LCPR, bool EDGE>
NS2_DEVINL void epi_f32_staged(f32x16 (&acc)[MI][2], const GemmArgs& g, int z, int row_base, int col_base, int nvc, int lane, unsigned char* wbuf) {
  constexpr int RPP = 16 * MI;
  constexpr bool WHOLE = LCPR == 4 && !EDGE;
  const int l31 = lane & 31;
  const float bc0 = (g.bias && (WHOLE || col_base + l31 < g.N)) ? g.bias[col_base + l31] : 0.f;
  const float bc1 = (g.bias && (WHOLE || col_base + 32 + l31 < g.N)) ? g.bias[col_base + 32 + l31] : 0.f;
  const int lcpr = LCPR ? LCPR : 31 - __builtin_clz(nvc >> 2);
#pragma unroll
  for (int pass = 0; pass < 32 * MI / RPP; ++pass) {
    const int row0 = row_base + pass * RPP;
    const auto stage = [&]() __attribute__((always_inline)) {
      f32_stage_rows<RPP / 32>(acc, pass * (RPP / 32), bc0, bc1, EDGE ? g.act : 0, lane, wbuf);
      __builtin_amdgcn_wave_barrier();
    };
    const auto keep_nothing = [](int, int, const float4&) {};
    if constexpr (WHOLE) {
      float4 rr[RPP / 4];
      if (g.resid) {
        const float* rbase = g.resid + (long)(row0 + (lane >> 4)) * g.ldr + col_base + (lane & 15) * 4;
#pragma unroll
        for (int it = 0; it < RPP / 4; ++it) rr[it] = *reinterpret_cast<const float4*>(rbase + (long)it * 4 * g.ldr);
      }
      stage();
      f32_store_rows<RPP, LCPR, EDGE>(g, z, row0, col_base, lcpr, lane, wbuf, rr, keep_nothing);
    } else {
      stage();
      f32_store_rows<RPP, LCPR, EDGE>(g, z, row0, col_base, lcpr, lane, wbuf, nullptr, keep_nothing);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// The same for the 128x128 kernel's tile with the RMSNorm of the updated rows behind it (GemmArgs::nrm_*; launch_gemm guarantees
// N == 128 == BN and M % 128 == 0, so the block owns 128 whole rows and all four waves are here): the lane keeps its 16 float4 of x, the
// row's sum of squares is 16 lanes of this wave + the half of the wave beside it (the other 64 columns) through 64 floats of LDS per
// wave, added in a fixed order.  LDS layout this relies on (gemm_kernel's): the regions of the two waves that share a row block, column
// halves (wm, 0) and (wm, 1), are neighbours WBUF bytes apart, (wm, 0) first; which half this wave is follows from col_base (N == 128).
template <int WBUF>
NS2_DEVINL void epi_f32_staged_norm(f32x16 (&acc)[2][2], const GemmArgs& g, int row_base, int col_base, int lane, unsigned char* wbuf) {
  static_assert(32 * F32_RS + 64 * 4 <= WBUF, "32 staged rows + the wave's 64 partial sums behind them");
  const int l31 = lane & 31, wn = (col_base >> 6) & 1;
  const float bc0 = (g.bias && col_base + l31 < g.N) ? g.bias[col_base + l31] : 0.f;
  const float bc1 = (g.bias && col_base + 32 + l31 < g.N) ? g.bias[col_base + 32 + l31] : 0.f;
  float4 keep[2][8];
  float* s_part = reinterpret_cast<float*>(wbuf + 32 * F32_RS);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    f32_stage_rows<1>(acc, mi, bc0, bc1, 0, lane, wbuf);
    __builtin_amdgcn_wave_barrier();
    f32_store_rows<32, 4, false>(g, 0, row_base + mi * 32, col_base, 4, lane, wbuf, nullptr, [&](int it, int lr, const float4& v) __attribute__((always_inline)) {
      keep[mi][it] = v;
      float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 8, 64);
      if ((lane & 15) == 0) s_part[mi * 32 + lr] = ss;
    });
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  const float* p0 = s_part - wn * (WBUF / 4);           // the row's column halves: waves (wm, 0) and (wm, 1)
  const float* p1 = p0 + WBUF / 4;
  const int c = col_base + (lane & 15) * 4;
  float gm[4];
  norm_gamma4(g, c, gm);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int lr = mi * 32 + it * 4 + (lane >> 4);
      norm_tail_store4(g, g.N, row_base + lr, c, keep[mi][it], p0[lr] + p1[lr], gm);
    }
}

}  // namespace ns2
