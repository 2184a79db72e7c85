// extern "C" surface of the backward (training) pass: declared in include/ns2hip_train.h.  Kernels: backward.hip; the
// contractions are calls of the forward GEMM family (gemm.hip / gemm2.hip) on re-packed weights / transposed operand planes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "ns2_host.h"

using namespace ns2;

extern "C" int ns2_weight_update(ns2_weight* w, const float* w_src, const float* extra1x1, void* stream) {
  ARGCHK(w && w_src && w->d_map, "ns2_weight_update: null weight / source");
  ARGCHK((extra1x1 != nullptr) == (w->has_extra != 0), "ns2_weight_update: extra1x1 must be given iff the weight was packed with one");
  hipStream_t s = (hipStream_t)stream;
  // same kernel and row map as ns2_weight_pack, in place: stream-ordered, no allocation, no synchronisation
  HIPRET(launch_pack_weight(w_src, w->cols, w->taps, w->cols_p, w->d_map, w->w.rows_p, w->w.hi, w->w.lo, w->w.ldk, 0, s, w->w.fmt));
  if (extra1x1)
    HIPRET(launch_pack_weight(extra1x1, w->cols, 1, w->cols_p, w->d_map, w->w.rows_p, w->w.hi, w->w.lo, w->w.ldk, w->taps * w->cols_p, s,
                              w->w.fmt));
  if (w->w.t3) return build_conv3_tiles(&w->owned, &w->w, s);      // the tiled copies follow the pack (no allocation: they exist)
  if (w->w.tl) return build_lin_tiles(&w->owned, &w->w, s);
  if (w->w.tw1) HIPRET(wavenet3_build_tiles(w->w.hi, w->w.rows_p, w->cols_p, 1, w->w.tw1, w->w.tw2, s));
  return NS2_OK;
}

// ---- all packs of a training pass in one launch (elementwise.hip repack_kernel).  The table lives in CALLER-owned device memory (the
// library keeps no state): ns2_weights_repack_build fills it from a host array of parts (once; synchronising copy), ns2_weights_repack
// replays it (stream-ordered, no allocation, no synchronisation).  A part is valid while its weight handle and its source storage live.
extern "C" int64_t ns2_weights_repack_table_bytes(int n) { return n > 0 ? (int64_t)n * (int64_t)sizeof(RepackDesc) : 0; }
extern "C" int ns2_weights_repack_build(const ns2_repack_part* parts, int n, void* table_device, int64_t table_bytes, int64_t* total_blocks, void* stream) {
  ARGCHK(parts && n > 0 && table_device && total_blocks, "ns2_weights_repack_build: null argument");
  ARGCHK(table_bytes >= ns2_weights_repack_table_bytes(n), "ns2_weights_repack_build: table too small (ns2_weights_repack_table_bytes)");
  std::vector<RepackDesc> tab((size_t)n);
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const ns2_repack_part& p = parts[i];
    ARGCHK(p.w && p.src, "ns2_weights_repack_build: null weight / source");
    const ns2_weight* w = p.w;
    ARGCHK(!w->geglu && !w->has_extra, "ns2_weights_repack_build: plain packs only (no GEGLU row permutation, no extra 1x1 block)");
    ARGCHK(p.rows > 0 && p.cols > 0 && p.row0 >= 0 && p.col0 >= 0 && p.row0 + p.rows <= w->w.N && p.col0 + p.cols <= w->cols,
           "ns2_weights_repack_build: part outside its weight");
    RepackDesc& d = tab[(size_t)i];
    const bool il = w->w.lo != nullptr;
    d.src = p.src; d.sr = (long)p.sr; d.sc = (long)p.sc; d.st = (long)p.st;
    d.dst_hi = w->w.hi; d.drs = il ? 2L * w->w.ldk : (long)w->w.ldk;
    d.row0 = p.row0; d.rows = p.rows; d.col0 = p.col0; d.cols = p.cols;
    d.Cp = w->cols_p; d.T = w->taps; d.fmt = w->w.fmt; d.il = il ? 1 : 0;
    d.chunks = (w->taps * ((p.cols + 3) / 4) + 255) / 256; d.pad_ = 0;          // a thread packs 4 columns
    d.block0 = blocks;
    blocks += (long)p.rows * d.chunks;
  }
  ARGCHK(blocks <= 0x7fffffffL, "ns2_weights_repack_build: too many blocks for one launch");
  HIPRET(hipMemcpyAsync(table_device, tab.data(), (size_t)n * sizeof(RepackDesc), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPRET(hipStreamSynchronize((hipStream_t)stream));         // the host vector dies here
  *total_blocks = blocks;
  return NS2_OK;
}
// the tiled images (ffconv_kernel.h / gemm3_kernel.h / wavenet3_kernel.h) of weights whose packs ns2_weights_repack has just refreshed:
// one small launch per weight that has images, none for the others; stream-ordered, no allocation (the images exist)
extern "C" int ns2_weights_retile(ns2_weight* const* ws, int n, void* stream) {
  ARGCHK(ws && n > 0, "ns2_weights_retile: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    ns2_weight* w = ws[i];
    ARGCHK(w, "ns2_weights_retile: null weight");
    int r = NS2_OK;
    if (w->w.t3) r = build_conv3_tiles(&w->owned, &w->w, s);
    else if (w->w.tl) r = build_lin_tiles(&w->owned, &w->w, s);
    else if (w->w.tw1) HIPRET(wavenet3_build_tiles(w->w.hi, w->w.rows_p, w->cols_p, 1, w->w.tw1, w->w.tw2, s));
    if (r != NS2_OK) return r;
  }
  return NS2_OK;
}
extern "C" int ns2_weights_repack(const void* table_device, int n, int64_t total_blocks, void* stream) {
  ARGCHK(table_device && n > 0 && total_blocks > 0, "ns2_weights_repack: bad arguments");
  HIPRET(launch_repack(static_cast<const RepackDesc*>(table_device), n, (long)total_blocks, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int64_t ns2_grad_prep_slices(int M, int64_t ld_t) { return M > 0 ? (int64_t)tplanes_slices(M, (long)ld_t) : 0; }

extern "C" int ns2_grad_prep(const float* x, int64_t ldx, int M, int C, int seq_len, int shift, uint16_t* row_hi, uint16_t* row_lo,
                             int ld_row, uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, float* colsum_partial,
                             int precision, void* stream) {
  ARGCHK(x && (row_hi || t_hi || colsum_partial), "ns2_grad_prep: nothing to do");
  ARGCHK(precision == 3 || precision == 4, "ns2_grad_prep: precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  TPlanesArgs a;
  memset(&a, 0, sizeof a);
  a.xf = x; a.ldx = (long)ldx; a.M = M; a.C = C; a.seq_len = seq_len; a.shift = shift;
  a.row_hi = row_hi; a.row_lo = row_lo; a.ld_row = ld_row;
  a.t_hi = t_hi; a.t_lo = t_lo; a.ld_t = (long)ld_t; a.per_batch = per_batch; a.t_rows_per_batch = t_rows; a.t_rows = t_rows;
  a.colsum_partial = colsum_partial;
  a.fmt = operand_fmt(precision);
  HIPRET(launch_tplanes(a, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_planes_transpose(const uint16_t* in_hi, const uint16_t* in_lo, int ld_in, int in_col0, int M, int C, int seq_len,
                                    int shift, uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, int precision,
                                    void* stream) {
  ARGCHK(in_hi && in_lo && t_hi && t_lo, "ns2_planes_transpose: null pointer (operands are interleaved lines: lo = hi + 32)");
  ARGCHK(precision == 3 || precision == 4, "ns2_planes_transpose: precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  TPlanesArgs a;
  memset(&a, 0, sizeof a);
  a.in_hi = in_hi; a.in_lo = in_lo; a.ld_in = ld_in; a.in_col0 = in_col0; a.M = M; a.C = C; a.seq_len = seq_len; a.shift = shift;
  a.t_hi = t_hi; a.t_lo = t_lo; a.ld_t = (long)ld_t; a.per_batch = per_batch; a.t_rows_per_batch = t_rows; a.t_rows = t_rows;
  a.fmt = operand_fmt(precision);
  HIPRET(launch_tplanes(a, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_reduce_slices(const float* partial, int64_t outer, int S, int64_t inner, float* out, int accumulate, void* stream) {
  ARGCHK(partial && out, "ns2_reduce_slices: null pointer");
  HIPRET(launch_reduce_slices(partial, (long)outer, S, (long)inner, out, accumulate, (hipStream_t)stream));
  return NS2_OK;
}

// ---- weight gradient: dW[r, k, t] = sum_m dY[m, r] * X_t[m, k]  as ONE GEMM over transposed planes, split-K into fixed slots
// Slices of the token axis: every slice is a grid-z layer of output tiles writing its own slot.  The 256 x 256 kernel runs ONE workgroup
// per CU, so a launch costs ceil(tiles * S / 256) rounds of (nkt / S) K tiles each; among the divisors of nkt that leave >= 8 K tiles
// per slice take the cheapest -- a slice also pays for storing its fp32 slot and for the fixed-order sum reading it (~12 K-tile
// times) -- and of equally cheap ones the smallest.  (Round 4 aimed at ~2.5 workgroups per CU whatever the shape: a 512 x 512 gradient
// got 128 slots = 128 MB of partial sums for two rounds of 8-tile blocks; now 64 slots, one round of 16-tile blocks.)
static int wgrad_split(int R, int ncols, int64_t ld_t) {
  const int nkt = (int)(ld_t / 32);
  const bool big = ncols > 128;
  const long tiles = big ? (long)((R + 255) / 256) * ((ncols + 255) / 256) : (long)((R + 127) / 128);
  const long per_round = big ? 256 : 512;                // workgroups the chip runs at once (the 128 x 128 kernel: two per CU)
  int S = 1;
  long best = -1;
  for (int d = 1; d <= nkt && d <= std::max(1, nkt / 8); ++d) {
    if (nkt % d) continue;                               // slices must cover whole K tiles evenly
    const long cost = ((tiles * d + per_round - 1) / per_round) * (nkt / d + 12);     // + a slot's fp32 store and its later read, in K-tile times
    if (best < 0 || cost < best) { best = cost; S = d; }
  }
  return S;
}
extern "C" int64_t ns2_wgrad_workspace_bytes(int R, int ncols, int64_t ld_t) {
  if (R <= 0 || ncols <= 0 || ld_t <= 0 || (ld_t & 31)) return 0;
  return (int64_t)wgrad_split(R, ncols, ld_t) * R * ncols * (int64_t)sizeof(float);
}
extern "C" int ns2_wgrad(const uint16_t* dyt_hi, const uint16_t* dyt_lo, const uint16_t* xt_hi, const uint16_t* xt_lo, int64_t ld_t, int R,
                         int T, int Kp, int K, float* dw, void* workspace, int64_t workspace_bytes, int precision, void* stream) {
  ARGCHK(dyt_hi && dyt_lo == dyt_hi + 32 && xt_hi && xt_lo == xt_hi + 32 && dw && workspace, "ns2_wgrad: null pointer / operands must be interleaved lines (lo = hi + 32)");
  ARGCHK(precision == 3 || precision == 4, "ns2_wgrad: precision 3 (bf16 x3) or 4 (half product + fp8 correction terms on FMT_H8 lines)");
  ARGCHK(R > 0 && T > 0 && K > 0 && Kp >= K && (Kp & 3) == 0 && ld_t > 0 && (ld_t & 31) == 0 && ld_t < (1LL << 30), "ns2_wgrad: bad shapes");
  const int ncols = T * Kp;
  const int S = wgrad_split(R, ncols, ld_t);
  ARGCHK(workspace_bytes >= (int64_t)S * R * ncols * (int64_t)sizeof(float), "ns2_wgrad: workspace too small (ns2_wgrad_workspace_bytes)");
  GemmArgs g;
  const int nkt = (int)(ld_t / 32) / S;
  g.a_hi = dyt_hi; g.a_lo = dyt_lo; g.lda = (int)ld_t;
  g.w_hi = xt_hi; g.w_lo = xt_lo; g.ldw = (int)ld_t;        // rows of X^T beyond T * Kp up to the next multiple of 256 must exist (zeros)
  g.M = R; g.N = ncols; g.nkt = nkt; g.kt_per_tap = nkt;
  g.nz = S; g.a_zs = (long)nkt * 32; g.w_zs = (long)nkt * 32; g.out_f_zs = (long)R * ncols;
  g.epi = EPI_F32; g.out_f = (float*)workspace; g.ldo_f = ncols;
  HIPRET(launch_gemm(g, precision, (hipStream_t)stream));
  HIPRET(launch_wgrad_reduce((const float*)workspace, S, R, ncols, T, Kp, K, dw, (hipStream_t)stream));
  return NS2_OK;
}

// The same gradient straight from the TOKEN-MAJOR planes (gemm2.hip TR: LDS transpose reads form the fragments; no transposed
// copies, no shifted copies of a conv's input).  Same slots, same fixed-order sum.
// The TR kernel is the 256 x 256 kernel: gradients it would run on a handful of half-empty tiles (the dim = 128 model, short batches) keep
// the transposed route, where launch_gemm picks the 128 x 128 kernel by the same rule (gemm2.hip launch_gemm: <= 64 blocks of 256 x 256).
extern "C" int ns2_wgrad_rows_preferred(int R, int ncols, int64_t M) {
  if (R <= 128 || ncols <= 128 || M <= 0) return 0;
  const int64_t ld_t = (M + 31) / 32 * 32;
  const long blocks256 = (long)((R + 255) / 256) * ((ncols + 255) / 256) * wgrad_split(R, ncols, ld_t);
  return blocks256 > 64;
}
// row_lens: null = ns2_wgrad_rows; else ns2_wgrad_rows_lens (seq_len checked by it), the LENS instantiations of the TR kernel
static int wgrad_rows_impl(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x,
                           int64_t M, int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes,
                           int precision, const int* row_lens, void* stream) {
  ARGCHK(dy_hi && dy_lo == dy_hi + 32 && x_hi && x_lo == x_hi + 32 && dw && workspace, "ns2_wgrad_rows: null pointer / operands must be interleaved lines (lo = hi + 32)");
  ARGCHK(precision == 3 || precision == 4, "ns2_wgrad_rows: precision 3 (bf16 x3) or 4 (half product + fp8 correction terms on FMT_H8 lines)");
  ARGCHK(M > 0 && M < (1LL << 30) && R > 0 && T > 0 && K > 0 && Kp >= K && (Kp & 31) == 0 && (ld_dy & 31) == 0 && (ld_x & 31) == 0 && ld_dy >= R && ld_x >= Kp,
         "ns2_wgrad_rows: bad shapes (Kp, ld_dy, ld_x multiples of 32; ld_dy >= R; ld_x >= Kp)");
  ARGCHK(T == 1 || (seq_len >= 32 && dil >= 1 && M % seq_len == 0), "ns2_wgrad_rows: a conv's gradient needs utterances of seq_len >= 32 tokens");
  const int ncols = T * Kp;
  const int64_t ld_t = (M + 31) / 32 * 32;
  const int S = wgrad_split(R, ncols, ld_t);
  ARGCHK(workspace_bytes >= (int64_t)S * R * ncols * (int64_t)sizeof(float), "ns2_wgrad_rows: workspace too small (ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32)))");
  GemmArgs g;
  const int nkt = (int)(ld_t / 32) / S;
  g.a_hi = dy_hi; g.a_lo = dy_lo; g.lda = ld_dy;
  g.w_hi = x_hi; g.w_lo = x_lo; g.ldw = ld_x;
  g.M = R; g.N = ncols; g.nkt = nkt; g.kt_per_tap = nkt; g.dil = dil > 0 ? dil : 1; g.seq_len = T > 1 ? seq_len : 0;
  g.nz = S; g.out_f_zs = (long)R * ncols;
  g.epi = EPI_F32; g.out_f = (float*)workspace; g.ldo_f = ncols;
  g.tr_tokens = (int)M; g.tr_kp = Kp; g.tr_taps = T > 1 ? T : 0;
  if (row_lens) { g.row_lens = row_lens; g.lens_seq = seq_len; }
  HIPRET(launch_gemm_tr(g, precision, (hipStream_t)stream));
  if (row_lens) note_train_skip_launch();
  HIPRET(launch_wgrad_reduce((const float*)workspace, S, R, ncols, T, Kp, K, dw, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_wgrad_rows(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x,
                              int64_t M, int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes,
                              int precision, void* stream) {
  return wgrad_rows_impl(dy_hi, dy_lo, ld_dy, x_hi, x_lo, ld_x, M, R, T, Kp, K, dil, seq_len, dw, workspace, workspace_bytes, precision, nullptr, stream);
}
// ... on a ragged batch: what the entry refuses on its own account comes first, under its own name
extern "C" int ns2_wgrad_rows_lens(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x,
                                   int64_t M, int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace,
                                   int64_t workspace_bytes, int precision, const int* row_lens, void* stream) {
  ARGCHK(row_lens != nullptr, "ns2_wgrad_rows_lens: row_lens is null (ns2_wgrad_rows is the call that multiplies every token)");
  ARGCHK(seq_len > 0 && (seq_len & 255) == 0, "ns2_wgrad_rows_lens: seq_len must be a positive multiple of 256 (whole skipping granules per utterance)");
  ARGCHK(M > 0 && M % seq_len == 0, "ns2_wgrad_rows_lens: M must be whole utterances of seq_len rows");
  return wgrad_rows_impl(dy_hi, dy_lo, ld_dy, x_hi, x_lo, ld_x, M, R, T, Kp, K, dil, seq_len, dw, workspace, workspace_bytes, precision, row_lens, stream);
}

extern "C" int ns2_film_gate_fwd(const float* h, int64_t ldh, const float* film, int film_ld, int seq_len, int64_t M, int d, float* out,
                                 int64_t ldo, void* stream) {
  ARGCHK(h && film && out, "ns2_film_gate_fwd: null pointer");
  HIPRET(launch_film_gate_fwd(h, (long)ldh, film, film_ld, seq_len, (long)M, d, out, (long)ldo, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_film_gate_slices(int seq_len) { return seq_len > 0 ? film_gate_slices(seq_len) : 0; }
extern "C" int ns2_film_gate_bwd(const float* dg, int64_t lddg, const float* h, int64_t ldh, const float* film, int film_ld, int B,
                                 int seq_len, int d, float* dh, int64_t lddh, float* partial, void* stream) {
  ARGCHK(dg && h && film && dh && partial, "ns2_film_gate_bwd: null pointer");
  HIPRET(launch_film_gate_bwd(dg, (long)lddg, h, (long)ldh, film, film_ld, B, seq_len, d, dh, (long)lddh, partial, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_geglu_fwd(const float* pre, int64_t ldp, int64_t M, int f, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                             void* stream) {
  ARGCHK(pre && out_hi && out_lo, "ns2_geglu_fwd: null pointer");
  ARGCHK(precision == 3 || precision == 4, "ns2_geglu_fwd: precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  HIPRET(launch_geglu_fwd(pre, (long)ldp, (long)M, f, out_hi, out_lo, ldo, (hipStream_t)stream, operand_fmt(precision)));
  return NS2_OK;
}
extern "C" int ns2_geglu_bwd(const float* dh, int64_t lddh, const float* pre, int64_t ldp, int64_t M, int f, float* dpre, int64_t lddp,
                             void* stream) {
  ARGCHK(dh && pre && dpre, "ns2_geglu_bwd: null pointer");
  HIPRET(launch_geglu_bwd(dh, (long)lddh, pre, (long)ldp, (long)M, f, dpre, (long)lddp, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_rmsnorm_bwd_slices(int seq_len) { return seq_len > 0 ? rmsnorm_bwd_slices(seq_len) : 0; }
extern "C" int ns2_rmsnorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, const float* cond,
                               int cond_ld, int B, int seq_len, int d, const float* dx_add, float* dx, int64_t lddx, float* cond_partial,
                               float* gamma_partial, void* stream) {
  ARGCHK(x && dy && dx, "ns2_rmsnorm_bwd: null pointer");
  NormBwdArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.ldx = (long)ldx; a.dy = dy; a.lddy = (long)lddy; a.gamma = gamma; a.cond = cond; a.cond_ld = cond_ld;
  a.dx_add = dx_add; a.dx = dx; a.lddx = (long)lddx; a.cond_partial = cond_partial; a.gamma_partial = gamma_partial;
  a.B = B; a.seq_len = seq_len; a.d = d;
  HIPRET(launch_rmsnorm_bwd(a, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_attention_delta(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H,
                                   int Nq, float* delta, int o_precision, void* stream) {
  ARGCHK(d_out && o_hi && delta, "ns2_attention_delta: null pointer");
  ARGCHK(o_precision == 3 || o_precision == 4, "ns2_attention_delta: o_precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  HIPRET(launch_attn_delta(d_out, (long)ld_dout, o_hi, o_lo, ldo, B, H, Nq, delta, (hipStream_t)stream, operand_fmt(o_precision)));
  return NS2_OK;
}
static int attention_bwd(const ns2_attn_bwd_args* p, const int* lens, void* stream, int head_dim = 0) {
  ARGCHK(p->gp_precision == 0 || p->gp_precision == 3 || p->gp_precision == 4, "ns2_attention_bwd: gp_precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  AttnBwdArgs a;
  if (const char* bad = set_attn_dropout(a, p->dropout_p, p->dropout_seed, p->dropout_call)) { set_error("ns2_attention_bwd: %s", bad); return NS2_ERR_ARG; }
  a.q_hi = p->q_hi; a.q_lo = p->q_lo; a.ldq = p->ldq; a.q_col0 = p->q_col0;
  a.k_hi = p->k_hi; a.k_lo = p->k_lo; a.ldk = p->ldk; a.k_col0 = p->k_col0;
  a.v_hi = p->v_hi; a.v_lo = p->v_lo; a.ldv = p->ldv; a.v_col0 = p->v_col0;
  a.do_hi = p->do_hi; a.do_lo = p->do_lo; a.lddo = p->lddo;
  a.lse = p->lse; a.delta = p->delta;
  a.dq = p->dq; a.lddq = p->lddq; a.dq_col0 = p->dq_col0;
  a.dk = p->dk; a.lddk = p->lddk; a.dk_col0 = p->dk_col0;
  a.dv = p->dv; a.lddv = p->lddv; a.dv_col0 = p->dv_col0;
  a.B = p->B; a.H = p->H; a.Nq = p->Nq; a.Nk = p->Nk; a.scale = p->scale;
  a.gp_hi = p->gp_hi; a.gp_lo = p->gp_lo; a.gp_ld = p->gp_ld; a.gp_q = p->gp_q; a.gp_kv = p->gp_kv;
  a.gp_fmt = operand_fmt(p->gp_precision);
  a.kmask = p->key_mask;
  a.lens = lens;
  if (head_dim) HIPRET(launch_attention_bwd_hd(a, head_dim, (hipStream_t)stream));
  else HIPRET(launch_attention_bwd(a, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_attention_bwd(const ns2_attn_bwd_args* p, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_bwd: null argument block");
  return attention_bwd(p, nullptr, stream);
}

// ---- ragged training batches: what these entries refuse comes first, under their own names; the blocks
// themselves are ns2_attention_fwd's and ns2_attention_bwd's
// what the four entries that take lengths refuse of a block alike, under the caller's `name`
static int self_attention_lens_chk(const char* name, int Nq, int Nk, const uint8_t* key_mask, float dropout_p) {
  ARGCHK_AS(name, Nq == Nk, "Nq != Nk (lengths belong to a self-attention)");
  ARGCHK_AS(name, !key_mask, "key_mask together with lens (one way of shortening the keys per call)");
  ARGCHK_AS(name, dropout_p == 0.f, "dropout together with lens (the denoiser's self-attention has none)");
  return NS2_OK;
}
extern "C" int ns2_attention_train_fwd_lens(const ns2_attn_args* p, const int* lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_train_fwd_lens: null argument block");
  ARGCHK(lens != nullptr, "ns2_attention_train_fwd_lens: lens is null (ns2_attention_fwd is the call without lengths)");
  ARGCHK(p->lse, "ns2_attention_train_fwd_lens: lse is missing (this is the training forward; ns2_attention_fwd_lens is the inference one)");
  NSCHK(self_attention_lens_chk("ns2_attention_train_fwd_lens", p->Nq, p->Nk, p->key_mask, p->dropout_p));
  AttnArgs a;
  if (int rc = attn_args_from(p, &a)) return rc;
  a.klens = lens;
  HIPRET(launch_attention(a, p->precision, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_attention_bwd_lens(const ns2_attn_bwd_args* p, const int* lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_bwd_lens: null argument block");
  ARGCHK(lens != nullptr, "ns2_attention_bwd_lens: lens is null (ns2_attention_bwd is the call without lengths)");
  ARGCHK(p->lse, "ns2_attention_bwd_lens: lse is missing");
  NSCHK(self_attention_lens_chk("ns2_attention_bwd_lens", p->Nq, p->Nk, p->key_mask, p->dropout_p));
  return attention_bwd(p, lens, stream);
}

// ---- training at head dims 32 / 128: every refusal is made here, before any device call
static bool head_dim_ok(int d) { return d == 0 || d == 32 || d == 64 || d == 128; }
extern "C" int ns2_attention_train_fwd_hd(const ns2_attn_args* p, const int* lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_train_fwd_hd: null argument block");
  ARGCHK(head_dim_ok(p->head_dim), "ns2_attention_train_fwd_hd: head_dim must be 32, 64 or 128 (0 = 64)");
  ARGCHK(p->lse, "ns2_attention_train_fwd_hd: lse is missing (this is the training forward; ns2_attention_fwd is the inference one)");
  ARGCHK(p->precision == 3, "ns2_attention_train_fwd_hd: the training forward runs in precision 3");
  ARGCHK(p->q_lo && p->k_lo && p->vt_lo && p->o_lo, "ns2_attention_train_fwd_hd: precision 3 operands and o come with their lo planes");
  ARGCHK(((p->q_col0 | p->k_col0) & 31) == 0, "ns2_attention_train_fwd_hd: q_col0 and k_col0 must be multiples of 32 (interleaved lines)");
  if (lens) NSCHK(self_attention_lens_chk("ns2_attention_train_fwd_hd", p->Nq, p->Nk, p->key_mask, p->dropout_p));
  ns2_attn_args q = *p;            // attn_args_from is ns2_attention_fwd's translation, which ties lse to a head dim of 64
  q.head_dim = 0;
  AttnArgs a;
  if (int rc = attn_args_from(&q, &a)) return rc;
  a.D = p->head_dim ? p->head_dim : 64;
  a.klens = lens;
  HIPRET(launch_attention_train_hd(a, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_attention_delta_hd(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H,
                                      int Nq, int head_dim, float* delta, int o_precision, void* stream) {
  ARGCHK(d_out && o_hi && delta, "ns2_attention_delta_hd: null pointer");
  ARGCHK(head_dim_ok(head_dim), "ns2_attention_delta_hd: head_dim must be 32, 64 or 128 (0 = 64)");
  ARGCHK(o_precision == 3 || o_precision == 4, "ns2_attention_delta_hd: o_precision 3 (bf16 hi / lo planes) or 4 (FMT_H8 lines)");
  HIPRET(launch_attn_delta_hd(d_out, (long)ld_dout, o_hi, o_lo, ldo, B, H, Nq, head_dim ? head_dim : 64, delta, (hipStream_t)stream,
                              operand_fmt(o_precision)));
  return NS2_OK;
}
extern "C" int ns2_attention_bwd_hd(const ns2_attn_bwd_args* p, int head_dim, const int* lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_bwd_hd: null argument block");
  ARGCHK(head_dim_ok(head_dim), "ns2_attention_bwd_hd: head_dim must be 32, 64 or 128 (0 = 64)");
  ARGCHK(p->lse && p->delta, "ns2_attention_bwd_hd: lse or delta is missing");
  ARGCHK(((p->q_col0 | p->k_col0 | p->v_col0) & 31) == 0, "ns2_attention_bwd_hd: q_col0, k_col0 and v_col0 must be multiples of 32 (interleaved lines)");
  ARGCHK(!p->gp_q || (p->dq_col0 & 31) == 0, "ns2_attention_bwd_hd: dq_col0 of a plane output must be a multiple of 32");
  ARGCHK(!p->gp_kv || ((p->dk_col0 | p->dv_col0) & 31) == 0, "ns2_attention_bwd_hd: dk_col0 and dv_col0 of a plane output must be multiples of 32");
  ARGCHK(p->gp_q || !p->dq || (p->dq_col0 & 3) == 0, "ns2_attention_bwd_hd: dq_col0 must be a multiple of 4");
  ARGCHK(p->gp_kv || !(p->dk || p->dv) || ((p->dk_col0 | p->dv_col0) & 3) == 0, "ns2_attention_bwd_hd: dk_col0 and dv_col0 must be multiples of 4");
  if (lens) NSCHK(self_attention_lens_chk("ns2_attention_bwd_hd", p->Nq, p->Nk, p->key_mask, p->dropout_p));
  return attention_bwd(p, lens, stream, head_dim ? head_dim : 64);
}
extern "C" int ns2_dropout_keep_mask(const uint32_t* seed, unsigned call, float dropout_p, int B, int H, int Nq, int Nk, uint8_t* out, void* stream) {
  ARGCHK(seed && out, "ns2_dropout_keep_mask: null pointer");
  HIPRET(launch_dropout_keep_mask(seed, call, dropout_p, B, H, Nq, Nk, out, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_silu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream) {
  ARGCHK(x && out, "ns2_silu_fwd: null pointer");
  HIPRET(launch_silu_fwd(x, (long)ldx, (long)M, C, out, (long)ldo, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_silu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream) {
  ARGCHK(dy && x && dx, "ns2_silu_bwd: null pointer");
  HIPRET(launch_silu_bwd(dy, (long)lddy, x, (long)ldx, (long)M, C, dx, (long)lddx, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_embedding_bwd(const int64_t* ids, int64_t M, int pad_id, const float* dy, int64_t lddy, int rows, int d, float* dw, void* stream) {
  ARGCHK(ids && dy && dw, "ns2_embedding_bwd: null pointer");
  HIPRET(launch_embedding_bwd((const long long*)ids, (long)M, pad_id, dy, (long)lddy, rows, d, dw, (hipStream_t)stream));
  return NS2_OK;
}

// ---- training of the DurationPitchPredictor (kernels: duration_pitch.hip)
extern "C" int64_t ns2_groupnorm_silu_bwd_workspace_bytes(int B, int n, int C) {
  if (B <= 0 || n <= 0 || C <= 0) return 0;
  return ((int64_t)B * gn_bwd_row_chunks(n) + B) * 2 * C * (int64_t)sizeof(float);
}
extern "C" int ns2_groupnorm_silu_bwd(const float* dy, int64_t lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                                      const float* bias, float eps, const void* stats, int64_t stats_bytes, float* dx, float* dweight_dbias,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(dy && x && weight && bias && stats && dx && dweight_dbias && workspace, "ns2_groupnorm_silu_bwd: null pointer");
  ARGCHK(B > 0 && n > 0 && groups > 0 && C > 0 && C % groups == 0 && (C / groups) % 4 == 0, "ns2_groupnorm_silu_bwd: C / groups must be a multiple of 4");
  ARGCHK(stats_bytes >= ns2_groupnorm_workspace_bytes(B, n, C, groups), "ns2_groupnorm_silu_bwd: stats = the workspace ns2_groupnorm_silu filled (too small)");
  ARGCHK(workspace_bytes >= ns2_groupnorm_silu_bwd_workspace_bytes(B, n, C), "ns2_groupnorm_silu_bwd: workspace too small");
  ARGCHK(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)stats | (uintptr_t)dx | (uintptr_t)workspace) % 16 == 0,
         "ns2_groupnorm_silu_bwd: buffers must be 16-byte aligned");
  float* slots = (float*)workspace;
  float* colsum = slots + (int64_t)B * gn_bwd_row_chunks(n) * 2 * C;
  HIPRET(launch_groupnorm_silu_bwd(dy, (long)lddy, x, B, n, C, groups, weight, bias, eps, stats, dx, dweight_dbias, slots, colsum, (hipStream_t)stream));
  return NS2_OK;
}
// ... of a ragged batch: the same launches on the <true> kernels
extern "C" int ns2_groupnorm_silu_bwd_lens(const float* dy, int64_t lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                                           const float* bias, float eps, const void* stats, int64_t stats_bytes, const int* row_lens, float* dx,
                                           float* dweight_dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!row_lens)
    return ns2_groupnorm_silu_bwd(dy, lddy, x, B, n, C, groups, weight, bias, eps, stats, stats_bytes, dx, dweight_dbias, workspace,
                                  workspace_bytes, stream);
  ARGCHK(dy && x && weight && bias && stats && dx && dweight_dbias && workspace, "ns2_groupnorm_silu_bwd_lens: null pointer");
  ARGCHK(B > 0 && B <= 65535 && n > 0 && groups > 0 && groups <= 1024, "ns2_groupnorm_silu_bwd_lens: bad arguments (at most 65535 utterances, 1024 groups)");
  ARGCHK(C > 0 && C % groups == 0 && (C / groups) % 4 == 0 && C / groups <= 4096,
         "ns2_groupnorm_silu_bwd_lens: C / groups must be a multiple of 4, at most 4096");
  ARGCHK(lddy >= C && lddy % 4 == 0, "ns2_groupnorm_silu_bwd_lens: lddy must be a multiple of 4, at least C");
  ARGCHK(stats_bytes >= ns2_groupnorm_workspace_bytes(B, n, C, groups), "ns2_groupnorm_silu_bwd_lens: stats = the workspace ns2_groupnorm_silu_lens filled (too small)");
  ARGCHK(workspace_bytes >= ns2_groupnorm_silu_bwd_workspace_bytes(B, n, C), "ns2_groupnorm_silu_bwd_lens: workspace too small");
  ARGCHK(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)stats | (uintptr_t)dx | (uintptr_t)workspace) % 16 == 0,
         "ns2_groupnorm_silu_bwd_lens: buffers must be 16-byte aligned");
  ARGCHK((uintptr_t)row_lens % 4 == 0, "ns2_groupnorm_silu_bwd_lens: row_lens must be 4-byte aligned");
  float* slots = (float*)workspace;
  float* colsum = slots + (int64_t)B * gn_bwd_row_chunks(n) * 2 * C;
  HIPRET(launch_groupnorm_silu_bwd(dy, (long)lddy, x, B, n, C, groups, weight, bias, eps, stats, dx, dweight_dbias, slots, colsum, (hipStream_t)stream,
                                   row_lens));
  return NS2_OK;
}
extern "C" int64_t ns2_row_dot_relu_bwd_workspace_bytes(int64_t M, int K) {
  if (M <= 0 || K <= 0) return 0;
  return (int64_t)row_dot_bwd_chunks((long)M) * (K + 1) * (int64_t)sizeof(float);
}
extern "C" int ns2_row_dot_relu_bwd(const float* dout, const float* out, const float* h, int64_t ldh, const float* w, int64_t M, int K, float* dh,
                                    int64_t lddh, float* dw_db, void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(dout && out && h && w && dh && dw_db && workspace, "ns2_row_dot_relu_bwd: null pointer");
  ARGCHK(workspace_bytes >= ns2_row_dot_relu_bwd_workspace_bytes(M, K), "ns2_row_dot_relu_bwd: workspace too small");
  ARGCHK(((uintptr_t)h | (uintptr_t)w | (uintptr_t)dh) % 16 == 0, "ns2_row_dot_relu_bwd: h, w and dh must be 16-byte aligned");
  HIPRET(launch_row_dot_relu_bwd(dout, out, h, (long)ldh, w, (long)M, K, dh, (long)lddh, dw_db, (float*)workspace, (hipStream_t)stream));
  return NS2_OK;
}

// ---- training of the Aligner (kernels: aligner.hip, the ReLU pair in backward.hip)
extern "C" int ns2_relu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream) {
  ARGCHK(x && out, "ns2_relu_fwd: null pointer");
  HIPRET(launch_relu_fwd(x, (long)ldx, (long)M, C, out, (long)ldo, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_relu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream) {
  ARGCHK(dy && x && dx, "ns2_relu_bwd: null pointer");
  HIPRET(launch_relu_bwd(dy, (long)lddy, x, (long)ldx, (long)M, C, dx, (long)lddx, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int64_t ns2_align_attn_bwd_workspace_bytes(int B, int T, int n, int C) {
  if (T > 8192 || n > 1024 || C > 256) return 0;
  return align_attn_bwd_workspace_bytes(B, T, n, C);
}
extern "C" int ns2_align_attn_bwd(const float* queries, const float* keys, const float* aln_log, const float* aln_soft, const float* g_log,
                                  const float* g_soft, const int* text_lens, int B, int T, int n, int C, float* dq, float* dk, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  ARGCHK(queries && keys && aln_log && aln_soft && text_lens && dq && dk && workspace && B > 0 && T > 0 && n > 0 && C > 0,
         "ns2_align_attn_bwd: bad arguments");
  ARGCHK(n <= 1024 && C <= 256 && T <= 8192 && B <= 65535, "ns2_align_attn_bwd: at most 1024 phonemes, 256 channels, 8192 mel frames");
  ARGCHK(workspace_bytes >= align_attn_bwd_workspace_bytes(B, T, n, C), "ns2_align_attn_bwd: workspace too small (ns2_align_attn_bwd_workspace_bytes)");
  ARGCHK((uintptr_t)workspace % 16 == 0, "ns2_align_attn_bwd: the workspace must be 16-byte aligned");
  HIPRET(launch_align_attn_bwd(queries, keys, aln_log, aln_soft, g_log, g_soft, text_lens, B, T, n, C, dq, dk, workspace, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int64_t ns2_align_losses_workspace_bytes(int B, int T, int n) {
  if (T > 8192 || n > 1024) return 0;
  return align_losses_workspace_bytes(B, T, n);
}
extern "C" int ns2_align_losses_fwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, int B, int T, int n,
                                    float blank_logprob, float* fs_loss, float* bin_loss, void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(aln_log && text_lens && workspace && (fs_loss || bin_loss) && B > 0 && T > 0 && n > 0, "ns2_align_losses_fwd: bad arguments");
  ARGCHK(!fs_loss || mel_lens, "ns2_align_losses_fwd: the forward-sum loss needs mel_lens");
  ARGCHK(!bin_loss || hard, "ns2_align_losses_fwd: the bin loss needs the hard alignment");
  ARGCHK(n <= 1024 && T <= 8192 && B <= 65535, "ns2_align_losses_fwd: at most 1024 phonemes and 8192 mel frames");
  ARGCHK(workspace_bytes >= align_losses_workspace_bytes(B, T, n), "ns2_align_losses_fwd: workspace too small (ns2_align_losses_workspace_bytes)");
  HIPRET(launch_align_losses_fwd(aln_log, hard, text_lens, mel_lens, B, T, n, blank_logprob, fs_loss, bin_loss, workspace, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_align_losses_bwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, const float* g_fs,
                                    const float* g_bin, int B, int T, int n, float blank_logprob, float* d_log, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  ARGCHK(aln_log && text_lens && workspace && d_log && (g_fs || g_bin) && B > 0 && T > 0 && n > 0, "ns2_align_losses_bwd: bad arguments");
  ARGCHK(!g_fs || mel_lens, "ns2_align_losses_bwd: the forward-sum loss needs mel_lens");
  ARGCHK(!g_bin || hard, "ns2_align_losses_bwd: the bin loss needs the hard alignment");
  ARGCHK(n <= 1024 && T <= 8192 && B <= 65535, "ns2_align_losses_bwd: at most 1024 phonemes and 8192 mel frames");
  ARGCHK(workspace_bytes >= align_losses_workspace_bytes(B, T, n), "ns2_align_losses_bwd: workspace = the one ns2_align_losses_fwd filled (too small)");
  HIPRET(launch_align_losses_bwd(aln_log, hard, text_lens, mel_lens, g_fs, g_bin, B, T, n, blank_logprob, d_log, workspace, (hipStream_t)stream));
  return NS2_OK;
}

// ---- the RVQ cross-entropy term of the training loss (rvq_ce.hip)
extern "C" int64_t ns2_rvq_ce_workspace_bytes(int M, int Q, int want_quantized) {
  if (M <= 0 || Q <= 0) return 0;
  return want_quantized ? (int64_t)M * Q * (int64_t)sizeof(int64_t) : 0;
}
// the codebook shape and the workspace, which ns2_rvq_ce and ns2_rvq_ce_lens check alike once M is known, under the caller's `name`
static int rvq_ce_chk(const char* name, int M, int Q, int C, int D, const float* quantized_out, const void* workspace, int64_t workspace_bytes) {
  ARGCHK_AS(name, D == 128 && C % 64 == 0, "needs codebook_dim 128 and codebook_size % 64 == 0 (EnCodec: 128 / 1024)");
  ARGCHK_AS(name, !quantized_out || (workspace && workspace_bytes >= ns2_rvq_ce_workspace_bytes(M, Q, 1)),
            "quantized_out needs a workspace (ns2_rvq_ce_workspace_bytes)");
  return NS2_OK;
}
extern "C" int ns2_rvq_ce(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss, float* loss,
                          float* quantized_out, float* grad, int M, int Q, int C, int D, void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(x && codebooks && cb_norm && indices && row_loss && loss, "ns2_rvq_ce: null pointer");
  ARGCHK(M > 0 && Q > 0 && C > 0, "ns2_rvq_ce: M, Q and C must be positive");
  NSCHK(rvq_ce_chk("ns2_rvq_ce", M, Q, C, D, quantized_out, workspace, workspace_bytes));
  RvqCeArgs a{x, codebooks, cb_norm, indices, row_loss, loss, quantized_out ? (int64_t*)workspace : nullptr, quantized_out, grad, M, Q, C, D};
  HIPRET(launch_rvq_ce(a, (hipStream_t)stream));
  return NS2_OK;
}
// ... of a ragged batch: the same kernel on RvqCeLensArgs; row_lens is device memory, nothing here reads it
extern "C" int ns2_rvq_ce_lens(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss,
                               float* loss, float* quantized_out, float* grad, int B, int n, const int* row_lens, int Q, int C, int D,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(x && codebooks && cb_norm && indices && row_loss && loss, "ns2_rvq_ce_lens: null pointer");
  ARGCHK(row_lens, "ns2_rvq_ce_lens: row_lens is null (ns2_rvq_ce is the call without lengths)");
  ARGCHK(B > 0 && n > 0 && Q > 0 && C > 0, "ns2_rvq_ce_lens: B, n, Q and C must be positive");
  ARGCHK((int64_t)B * n <= 0x7fffffffLL, "ns2_rvq_ce_lens: B * n must fit an int");
  const int M = B * n;
  NSCHK(rvq_ce_chk("ns2_rvq_ce_lens", M, Q, C, D, quantized_out, workspace, workspace_bytes));
  RvqCeLensArgs a;
  a.x = x; a.codebooks = codebooks; a.cb_norm = cb_norm; a.targets = indices; a.row_loss = row_loss; a.loss = loss;
  a.nearest = quantized_out ? (int64_t*)workspace : nullptr; a.quantized_out = quantized_out; a.grad = grad;
  a.M = M; a.Q = Q; a.C = C; a.D = D;
  a.row_lens = row_lens; a.B = B; a.n = n;
  HIPRET(launch_rvq_ce_lens(a, (hipStream_t)stream));
  return NS2_OK;
}
