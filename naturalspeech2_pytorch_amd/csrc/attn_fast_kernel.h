// The self-attention forward of the one-half-product plans at head dimension 64 on whole tiles: a second kernel beside attn_kernel
// (attention.hip, which includes this header so that both share the translation unit's range-guard counter).
//
// Why: attn_kernel<1, true, 4, false, 64> runs QK^T, waits, runs the whole softmax, then PV, then a workgroup barrier, once per
// 64-key tile and wave; the matrix pipe is busy a quarter of the time and the overlap of one wave's exp / max / convert work with
// another wave's MFMAs is left to whichever three workgroups share a SIMD.  Here:
//   * a wave owns TWO 32-row query blocks A and B (a workgroup = 4 waves = 256 query rows).  Every K and V^T fragment read from
//     LDS feeds both blocks' MFMAs: half the ds_read_b128 per MFMA.  As compiled, the 16 S MFMAs of a tile issue back to back
//     (S_A, S_B), then softmax_A; in-wave overlap of vector work with the matrix pipe exists only in the two PV phases (block
//     B's row maximum and exponentials in the gaps of PV_A / PV_B, 7-8 v_exp per gap).  The rest of the overlap still comes
//     from the SIMD's second wave (another workgroup).  Pinning the softmax slices between the S MFMAs was tried and was
//     slower: the gain of this kernel is the shared fragments and staging, not a tighter interleave;
//   * every staged K / V^T tile serves 256 query rows: half the global re-reads, half the LDS writes and barriers per MFMA;
//   * the output format is a template parameter; O is normalised, converted and staged through the wave's share of the (by then
//     free) tile buffers and leaves as 16-byte stores of whole 128-B / 256-B row segments, with the range guard as a running
//     maximum per lane and one atomic at the end (RangeTrack, gemm_epi_fast.h) instead of three 4-8-byte stores per four columns.
// The arithmetic is attn_kernel's, operation for operation (same S accumulation order, raw scores with the scale folded into the
// exponent's fma, same m / alpha / l recurrences including the contracted l * alpha + psum, psum in (js, r) order, the alpha != 1
// skip, the same conversions): the two kernels agree bit for bit, which tests/test_attention_fast_gpu.py asserts.
// Eligibility: attn_fast_eligible() in attention.hip.  No key masking, no ragged tiles, no lo planes: none of those branches exist here.
// LENS (a separate instantiation, as WLSE / DROP are of attn_kernel: the kernels without it compile to what they were): per-utterance key
// counts (AttnArgs::klens).  Utterance b walks ceil(len_b / 64) key tiles -- whole tiles beyond its length are never staged -- and its
// partial last tile takes a workgroup-uniform slow path (peeled out of the loop over whole tiles) that does what attn_kernel does with keys
// at or beyond Nk: K rows staged as zeros, the V^T chunk cut with mask_chunk, scores set to -inf.  Nk stays the stride of every address.
#pragma once
#include "gemm_epi_fast.h"

#include <type_traits>

namespace ns2 {

constexpr int AF_QB = 256;                 // query rows per workgroup: 4 waves x 2 blocks x 32
constexpr int AF_STAGE = AtGeom<64>::KPLANE + AtGeom<64>::VPLANE;       // one K tile + one V^T tile: 18 KiB
constexpr int AF_LDS = 2 * AF_STAGE;                                    // two stages: 36 KiB, two workgroups per CU
constexpr int AF_WBUF = AF_LDS / 4;                                     // a wave's share for the epilogue: 9216 B
static_assert(64 * (128 + 16) <= AF_WBUF && 32 * (256 + 16) <= AF_WBUF, "a wave stages 64 dense rows or 32 interleaved rows at a time");

// four adjacent logical columns (c % 4 == 0, 0 <= c < 64) of one staged output row, in global byte order
template <int PF>
NS2_DEVINL void af_put4(unsigned char* rowp, int c, float v0, float v1, float v2, float v3, RangeTrack& rt) {
  rt.see(v0, v1);
  rt.see(v2, v3);
  if constexpr (PF == PF_F16) {
    *reinterpret_cast<uint2*>(rowp + c * 2) = make_uint2(cvt2h_q(v0, v1), cvt2h_q(v2, v3));
  } else {
    static_assert(PF == PF_H8, "IEEE-half outputs only");
    uint32_t ha, hb, h8a, h8b, l8a, l8b;
    cvt2_h8_q(v0, v1, ha, h8a, l8a);
    cvt2_h8_q(v2, v3, hb, h8b, l8b);
    unsigned char* line = rowp + (c >> 5) * 128;
    *reinterpret_cast<uint2*>(line + (c & 31) * 2) = make_uint2(ha, hb);
    *reinterpret_cast<uint32_t*>(line + 64 + (c & 31)) = h8a | (h8b << 16);
    *reinterpret_cast<uint32_t*>(line + 96 + (c & 31)) = l8a | (l8b << 16);
  }
}

// QSKIP: ragged skipping (attn_kernel's QSKIP) -- a 256-row query workgroup at or behind the utterance's computed extent returns before its
// first load; a separate instantiation
template <int PF, bool LENS = false, bool QSKIP = false>
__global__ __launch_bounds__(256, 2) void attn_fast_kernel(const AttnArgs a) {
  using G = AtGeom<64>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  // the query tiles of one (batch, head) get consecutive remapped ids: one XCD's L2 serves their K / V^T re-reads (attn_kernel)
  const int nqt = a.Nq / AF_QB;
  int bid = QSKIP ? xcd_spread(blockIdx.x, gridDim.x, nqt) : xcd_remap(blockIdx.x, gridDim.x);
  const int qt = bid % nqt;
  bid /= nqt;
  const int h = bid % a.H, b = bid / a.H;
  if constexpr (QSKIP) {
    if (qt * AF_QB >= ragged_extent(a.qlens[b], a.Nq)) return;
  }
  const int qrow0 = qt * AF_QB + wave * 64;            // block A: rows qrow0 + l31, block B: 32 further
  int nk = a.Nk;                                       // keys this utterance attends to
  if constexpr (LENS) nk = min(max(a.klens[b], 1), a.Nk);

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q = l31][d = 16c + 8hi .. +7] of each block
  bf16x8 qf[2][4];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint4 v = ld16g(a.q_hi + ((long)b * a.Nq + qrow0 + 32 * blk + l31) * a.ldq + a.q_col0 + h * 64 + 16 * c + 8 * hi);
      qf[blk][c] = *reinterpret_cast<const bf16x8*>(&v);
    }

  // ---- staging: two 16-B chunks of the K tile (key row / 8-dim chunk) and of the V^T tile (feature row / 8-key chunk) per thread
  const int srow = tid >> 3, sch = tid & 7;            // chunk i: row srow + 32 i
  const bf16_t* kp = a.k_hi + ((long)b * a.Nk + srow) * a.ldk + a.k_col0 + h * 64 + sch * 8;
  const bf16_t* vp = a.vt_hi + ((long)b * a.H * 64 + h * 64 + srow) * a.vt_ld + sch * 8;
  const long kstep = 32L * a.ldk, vstep = 32L * a.vt_ld;
  const int st_off = srow * AT_ROWB + sch * 16;        // ROWB_K == AT_ROWB at D = 64
  static_assert(G::ROWB_K == AT_ROWB, "one row pitch for both tiles");
  uint4 rk[2], rv[2];
  auto load_tile = [&](int key0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rk[i] = ld16g(kp + (long)key0 * a.ldk + i * kstep);
      rv[i] = ld16g(vp + key0 + i * vstep);
    }
  };
  auto store_tile = [&](int s, int key0) {               // key0: first key of the tile in the registers (read with LENS only)
    if constexpr (LENS) {
      // the utterance's partial last tile: what lies at or beyond its length may hold anything.  Cut here, where the loaded registers are
      // waited for anyway, not behind the loads: the loop's issue order stays that of the kernel without lengths
      if (key0 + 64 > nk) {
        const int nvalid = nk - key0 - sch * 8;          // of this thread's 8-key V^T chunks
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (key0 + srow + 32 * i >= nk) rk[i] = make_uint4(0u, 0u, 0u, 0u);
          if (nvalid <= 0) rv[i] = make_uint4(0u, 0u, 0u, 0u);
          else if (nvalid < 8) rv[i] = mask_chunk(rv[i], nvalid);
        }
      }
    }
    unsigned char* base = smem + s * AF_STAGE + st_off;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<uint4*>(base + i * 32 * AT_ROWB) = rk[i];
      *reinterpret_cast<uint4*>(base + G::KPLANE + i * 32 * AT_ROWB) = rv[i];
    }
  };

  // pi: swap bits 2 and 3 of the MFMA row index -> key row inside a 32-key sub-tile (attn_kernel)
  const int pi_row = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
  const int k_frag_off = pi_row * G::ROWB_K + hi * 16;                // + js*32*ROWB_K + c*32
  const int v_frag_off = G::KPLANE + l31 * AT_ROWB + hi * 16;         // + dt*32*ROWB + js*64 + g1*32

  f32x16 ot[2][2];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[blk][dt][r] = 0.f;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  const float sl2 = a.scale * 1.4426950408889634f;

  // S^T = K Q^T of one block: two sub-tiles of 32 keys, four 16-deep chunks each, in attn_kernel's order
  auto scores = [&](f32x16 (&st)[2], const bf16x8 (&q)[4], const unsigned char* sb) {
#pragma unroll
    for (int js = 0; js < 2; ++js) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[js][r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sb + k_frag_off + js * 32 * G::ROWB_K + c * 32);
        st[js] = mma16<true>(kf, q[c], st[js]);
      }
    }
  };
  // online softmax of one block for query l31 (attn_kernel's recurrences); leaves P as packed halves, the PV product's B operand
  auto softmax = [&](f32x16 (&st)[2], float& m, float& l, f32x16 (&o)[2], uint4 (&pf)[2][2]) {
    // the row maximum: four independent chains instead of attn_kernel's one of 16 (max is exact in any order), and the two half-waves
    // exchange it with v_permlane32_swap instead of a ds_bpermute round trip through the LDS queue
    float mc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mc[i] = fmaxf(st[i >> 1][8 * (i & 1)], st[i >> 1][8 * (i & 1) + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 2; r < 8; r += 2) mc[i] = fmaxf(fmaxf(mc[i], st[i >> 1][8 * (i & 1) + r]), st[i >> 1][8 * (i & 1) + r + 1]);
    float mx = fmaxf(fmaxf(mc[0], mc[1]), fmaxf(mc[2], mc[3]));
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float m_new = fmaxf(m, mx * sl2);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    float psum = 0.f;
#pragma unroll
    for (int js = 0; js < 2; ++js)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[js][r], sl2, -m_new));
        psum += p;
        st[js][r] = p;
      }
    l = __builtin_fmaf(l, alpha, psum);                  // contracted, as attn_kernel compiles it
    if (__any(alpha != 1.0f)) {                          // the running maximum rarely moves after the first tiles
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    }
#pragma unroll
    for (int js = 0; js < 2; ++js)
#pragma unroll
      for (int g1 = 0; g1 < 2; ++g1)
        pf[js][g1] = make_uint4(cvt2h_inrange(st[js][8 * g1 + 0], st[js][8 * g1 + 1]), cvt2h_inrange(st[js][8 * g1 + 2], st[js][8 * g1 + 3]),
                                cvt2h_inrange(st[js][8 * g1 + 4], st[js][8 * g1 + 5]), cvt2h_inrange(st[js][8 * g1 + 6], st[js][8 * g1 + 7]));
  };
  // O^T += V^T P^T of one block, in attn_kernel's (js, g1) order
  auto pv = [&](f32x16 (&o)[2], const uint4 (&pf)[2][2], const unsigned char* sb) {
#pragma unroll
    for (int js = 0; js < 2; ++js)
#pragma unroll
      for (int g1 = 0; g1 < 2; ++g1)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sb + v_frag_off + dt * 32 * AT_ROWB + js * 64 + g1 * 32);
          o[dt] = mma16<true>(vf, *reinterpret_cast<const bf16x8*>(&pf[js][g1]), o[dt]);
        }
  };

  const int ntiles = LENS ? (nk + 63) / 64 : a.Nk / 64;
  load_tile(0);
  store_tile(0, 0);
  __syncthreads();

  // one key tile.  masked (a type: the whole tiles' body has no branch for it): the utterance's partial last tile, scores of keys at or
  // beyond its length are -inf before the softmax
  auto tile = [&](int t, bool more, auto masked) {
    if (more) load_tile((t + 1) * 64);                   // in flight during this tile's products
    const unsigned char* sb = smem + (t & 1) * AF_STAGE;
    f32x16 sa[2], sbk[2];
    uint4 pa[2][2], pb[2][2];
    scores(sa, qf[0], sb);
    scores(sbk, qf[1], sb);                              // same K fragments as S_A; the compiler issues all 16 MFMAs before softmax_A
    if constexpr (decltype(masked)::value) {             // register r of sub-tile js is key 64 t + 32 js + 16 (r >> 3) + 8 hi + (r & 7) (attn_kernel)
#pragma unroll
      for (int js = 0; js < 2; ++js)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t * 64 + 32 * js + 16 * (r >> 3) + 8 * hi + (r & 7) >= nk) { sa[js][r] = -INFINITY; sbk[js][r] = -INFINITY; }
    }
    softmax(sa, m_run[0], l_run[0], ot[0], pa);
    pv(ot[0], pa, sb);                                   // the compiler places block B's maximum and exponentials in PV_A's and PV_B's gaps
    softmax(sbk, m_run[1], l_run[1], ot[1], pb);
    pv(ot[1], pb, sb);                                   // same V^T fragments as PV_A
    if (more) store_tile((t + 1) & 1, (t + 1) * 64);     // the other stage: every wave left it at the previous barrier
    __syncthreads();
  };
  if constexpr (!LENS) {
    for (int t = 0; t < ntiles; ++t) tile(t, (t + 1) < ntiles, std::false_type{});
  } else {
    const int nfull = nk / 64;                           // whole tiles, then at most one partial tile: a workgroup-uniform path of its own
    for (int t = 0; t < nfull; ++t) tile(t, (t + 1) < ntiles, std::false_type{});
    if (nfull < ntiles) tile(nfull, false, std::true_type{});
  }

  // ---- normalise, convert, stage through the wave's share of the tile buffers (free after the last barrier), store whole row segments
  unsigned char* wbuf = smem + wave * AF_WBUF;
  RangeTrack rt;
  if constexpr (PF == PF_F16) {
    constexpr int RS = 128 + 16;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const float inv = 1.0f / (l_run[blk] + __shfl_xor(l_run[blk], 32, 64));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)        // lane holds d = 32dt + 8gq + 4hi + e for its query
          af_put4<PF>(wbuf + (32 * blk + l31) * RS, 32 * dt + 8 * gq + 4 * hi, ot[blk][dt][4 * gq + 0] * inv, ot[blk][dt][4 * gq + 1] * inv,
                      ot[blk][dt][4 * gq + 2] * inv, ot[blk][dt][4 * gq + 3] * inv, rt);
    }
    __builtin_amdgcn_wave_barrier();
    unsigned char* gbase = reinterpret_cast<unsigned char*>(a.o_hi + ((long)b * a.Nq + qrow0) * a.ldo + h * 64);
    lds_flush_rows<128, 64>(wbuf, gbase, 2L * a.ldo, lane);
  } else {
    constexpr int RS = 256 + 16;
    const long rsb = 4L * a.ldo;                         // interleaved 128-B lines of 32 logical columns: 4 bytes per logical column
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const float inv = 1.0f / (l_run[blk] + __shfl_xor(l_run[blk], 32, 64));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          af_put4<PF>(wbuf + l31 * RS, 32 * dt + 8 * gq + 4 * hi, ot[blk][dt][4 * gq + 0] * inv, ot[blk][dt][4 * gq + 1] * inv,
                      ot[blk][dt][4 * gq + 2] * inv, ot[blk][dt][4 * gq + 3] * inv, rt);
      __builtin_amdgcn_wave_barrier();
      unsigned char* gbase = reinterpret_cast<unsigned char*>(a.o_hi) + ((long)b * a.Nq + qrow0 + 32 * blk) * rsb + h * 256;
      lds_flush_rows<256, 32>(wbuf, gbase, rsb, lane);
      __builtin_amdgcn_wave_barrier();
    }
  }
  rt.flush(PlaneGeom<PF>::limit);
}

}  // namespace ns2
