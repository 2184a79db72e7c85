// The epilogue dispatcher (gemm_epi.h lists the epilogue layer's three headers): ONE decision per wave tile -- whole tile, right format,
// aligned destination -> a staged epilogue of gemm_epi_fast.h, else the generic one of gemm_epi.h -- for every GEMM kernel.
#pragma once
#include <type_traits>

#include "gemm_epi_fast.h"

namespace ns2 {

// Which plane formats a caller can be asked for, i.e. which staged instances it carries: the IEEE-half formats (FMT_F16, FMT_H8),
// interleaved bf16 hi / lo lines, dense bf16.  The callers' three spellings:
template <bool HALF, bool BF_IL, bool BF_DENSE>
struct EpiFormats { static constexpr bool half = HALF, bf_il = BF_IL, bf_dense = BF_DENSE; };
// the 128x128 kernel: a kernel on IEEE-half operands writes F16 / H8, one on bf16 operands bf16 planes (dense: the one-product mode)
template <int NSPLIT, bool F16> using G1Formats = EpiFormats<F16, !F16, !F16 && NSPLIT == 1>;
// the 256x256 family: the same, and bf16 hi / lo lines from the mixed product's EPI_SPLIT: q | k | v of the mixed TRAINING arithmetic,
// whose attention stays bf16 x3
template <int NSPLIT, int EPI, bool F16> using G2Formats = EpiFormats<F16, !F16 || (NSPLIT == 2 && EPI == EPI_SPLIT), !F16 && NSPLIT == 1>;
// the split-K finishing kernel serves both arithmetics
using FinishFormats = EpiFormats<true, true, true>;

// Epilogue of one wave tile of 32 * MI rows x 64 columns.  wbuf: the wave's private LDS region of WBUF bytes (0: none, generic only);
// the rows per staged pass follow from MI and WBUF.  ocol_base: first output column of this wave for EPI_GEGLU.
template <int EPI, int MI, class F, int WBUF>
NS2_DEVINL void wave_tile_epilogue(f32x16 (&acc)[MI][2], const GemmArgs& g, int z, int row_base, int col_base, int ocol_base, int lane,
                                   unsigned char* wbuf) {
  static_assert(WBUF == 0 || WBUF >= 32 * MI * 144, "a GEGLU tile (128-byte lines + pad) or a V^T tile (64 features x 32 * MI tokens + pad)");
  const bool rows_in = row_base + 32 * MI <= g.M;
  if constexpr (WBUF > 0 && EPI == EPI_F32) {
    const bool al = g.act == 0 && (g.ldo_f & 3) == 0 && (reinterpret_cast<uintptr_t>(g.out_f) & 15) == 0 &&
                    (!g.resid || ((g.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(g.resid) & 15) == 0));
    if constexpr (MI == 4) {
      // every tile is staged: measured 1.45x-1.65x on the whole launch against per-value stores (FF-out 218 -> 150 us at M = 32768)
      if (rows_in && col_base + 64 <= g.N && al) epi_f32_staged<MI, 4, false>(acc, g, z, row_base, col_base, 64, lane, wbuf);
      else epi_f32_staged<MI, 4, true>(acc, g, z, row_base, col_base, 64, lane, wbuf);
      return;
    } else {
      // whole rows of 16, 32 or 64 valid columns (the SEANet codec's 16 ... 128-channel convolutions run here, 80 k blocks per launch)
      const int nvc = min(64, g.N - col_base);
      if (nvc <= 0) return;
      if (rows_in && nvc >= 16 && (nvc & (nvc - 1)) == 0 && al) {
        if (g.nrm_hi) epi_f32_staged_norm<WBUF>(acc, g, row_base, col_base, lane, wbuf);
        else epi_f32_staged<MI, 0, false>(acc, g, z, row_base, col_base, nvc, lane, wbuf);
        return;
      }
    }
  } else if constexpr (WBUF > 0) {
    auto planes = [&](auto&& fn) __attribute__((always_inline)) {
      if ((reinterpret_cast<uintptr_t>(g.out_hi) & 15) != 0 || (g.ldo_s & 31) != 0) return false;
      if constexpr (F::half) {
        if (g.out_fmt == FMT_F16 && !g.out_lo) { fn(std::integral_constant<int, PF_F16>{}); return true; }
        if (g.out_fmt == FMT_H8) { fn(std::integral_constant<int, PF_H8>{}); return true; }
      }
      if constexpr (F::bf_il) {
        if (g.out_fmt == FMT_BF16 && g.out_lo) { fn(std::integral_constant<int, PF_BF16IL>{}); return true; }
      }
      if constexpr (F::bf_dense) {
        if (g.out_fmt == FMT_BF16 && !g.out_lo) { fn(std::integral_constant<int, PF_BF16>{}); return true; }
      }
      return false;
    };
    if (rows_in) {
      if constexpr (EPI == EPI_SPLIT) {                  // calls with an activation keep the generic path
        if (col_base + 64 <= g.N && g.act == 0 &&
            planes([&](auto pf) __attribute__((always_inline)) { epi_planes_fast<decltype(pf)::value, true, MI, WBUF>(acc, g, z, row_base, col_base, lane, wbuf); }))
          return;
      } else if constexpr (EPI == EPI_WAVENET) {
        if (col_base + 64 <= g.N &&
            planes([&](auto pf) __attribute__((always_inline)) { epi_planes_fast<decltype(pf)::value, false, MI, WBUF>(acc, g, z, row_base, col_base, lane, wbuf); }))
          return;
      } else if constexpr (EPI == EPI_GEGLU) {
        if (ocol_base + 32 <= g.out_ncols &&
            planes([&](auto pf) __attribute__((always_inline)) { epi_geglu_fast<decltype(pf)::value, MI>(acc, g, row_base, col_base, ocol_base, lane, wbuf); }))
          return;
      } else if constexpr (EPI == EPI_QKV) {
        if (col_base + 64 <= g.N && !g.bias) {
          if (col_base + 64 <= g.split_col) {
            if (planes([&](auto pf) __attribute__((always_inline)) { epi_planes_fast<decltype(pf)::value, false, MI, WBUF>(acc, g, 0, row_base, col_base, lane, wbuf); }))
              return;
          } else if (col_base >= g.split_col && !g.vt_lo && g.seq_len > 0 && (g.seq_len & (32 * MI - 1)) == 0 && (g.vt_ld & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(g.vt_hi) & 15) == 0) {      // V^T: the tile's tokens lie in one utterance
            if (F::half && g.vt_fmt == FMT_F16) { epi_vt_fast<true, MI>(acc, g, row_base, col_base, lane, wbuf); return; }
            if ((F::bf_il || F::bf_dense) && g.vt_fmt == FMT_BF16) { epi_vt_fast<false, MI>(acc, g, row_base, col_base, lane, wbuf); return; }
          }
        }
      }
    }
  }
  gemm_epilogue<EPI, MI>(acc, g, z, row_base, col_base, ocol_base, lane);
}

// ---- epilogue of a 256 x 256 block whose eight waves hold 128 x 64 accumulator tiles (wave -> (wm, wn) = (wave & 1, wave >> 1)): shared by
// gemm2_kernel, the lean linear kernel (gemm3_kernel.h) and the lean Wavenet block (wavenet3_kernel.h).  All waves are past the K loop's
// last barrier: the LDS ring is free, every wave takes a private 18 KiB region.
constexpr int G2_BM = 256, G2_BN = 256;

template <int NSPLIT, int EPI, bool F16>
NS2_DEVINL void g2_block_epilogue(f32x16 (&acc)[4][2], const GemmArgs& g, const int z, const int tm, const int tn, const int wave, const int lane,
                                  unsigned char* smem) {
  const int wm = wave & 1, wn = wave >> 1;
  const int col_base = tn * G2_BN + wn * 64;
  const int ncols_needed = (EPI == EPI_GEGLU || EPI == EPI_F32 || EPI == EPI_QKV) ? g.N : max(g.N, g.out_ncols);
  if (col_base < ncols_needed)
    wave_tile_epilogue<EPI, 4, G2Formats<NSPLIT, EPI, F16>, EPI_LDS_WAVE_BYTES>(acc, g, z, tm * G2_BM + wm * 128, col_base, tn * 128 + wn * 32, lane,
                                                                               smem + wave * EPI_LDS_WAVE_BYTES);
}

}  // namespace ns2
