// Internal (C++) launcher interface of libns2hip: one launcher per HIP kernel family.
// The public C ABI is the headers under include/; csrc/capi.cpp and csrc/model_exec.cpp sit on top of these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "ns2_fmt.h"
#include "ns2_sat_registry.h"

typedef uint16_t bf16_t;

namespace ns2 {

// Per-kernel "dynamic LDS size raised" flag, kept PER DEVICE (function attributes belong to the device's code object) and
// safe under concurrent first calls from several host threads (one thread per device is the supported model; a duplicated
// hipFuncSetAttribute is harmless).  This is the only host-side state a launcher keeps; it never allocates.
struct DynLdsAttr {
  static constexpr int kMaxDev = 64;
  std::atomic<int> bytes[kMaxDev];
  DynLdsAttr() { for (auto& b : bytes) b.store(0, std::memory_order_relaxed); }
  hipError_t ensure(const void* fn, int lds) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool tracked = dev >= 0 && dev < kMaxDev;
    if (tracked && bytes[dev].load(std::memory_order_acquire) >= lds) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess && tracked) bytes[dev].store(lds, std::memory_order_release);
    return e;
  }
};

// split-plane operands: a lo plane implies the interleaved [hi32|lo32] row layout, i.e. lo == hi + 32 (ns2_common.h)
inline bool planes_ok(const bf16_t* hi, const bf16_t* lo) { return lo == nullptr || lo == hi + 32; }

// The two format rules of a precision, each written once: what the GEMMs multiply in and write for each other (bf16 planes for 1 / 3, dense
// IEEE half for 2, FMT_H8 lines for 4), and what the attention kernels read (q, k, V^T: IEEE half also at precision 4)
inline int operand_fmt(int precision) { return precision == 2 ? FMT_F16 : (precision == 4 ? FMT_H8 : FMT_BF16); }
inline int attention_fmt(int precision) { return (precision == 2 || precision == 4) ? FMT_F16 : FMT_BF16; }

enum GemmEpilogue : int {
  EPI_F32 = 0,      // out_f = acc + bias (+ resid)
  EPI_SPLIT = 1,    // split planes = acc + bias
  EPI_QKV = 2,      // columns < split_col -> split planes, columns >= split_col -> transposed planes V^T[b][feat][n]
  EPI_GEGLU = 3,    // packed [x|gate] wave tiles -> split planes gelu(gate)*x
  EPI_WAVENET = 4,  // mid-loop FiLM + tanh*sigmoid gate, second K phase = res conv, split planes out
};

// Every field has a default: a default-constructed block is a valid "nothing optional" block (zero / null except the six sentinels
// dil, mid_kt, nz, pad_left, out_fmt, vt_fmt), and a caller names only what it uses
struct GemmArgs {
  // A operand: activations, bf16 split planes [M, lda]; every ld / column count in this struct is LOGICAL (the
  // physical row stride is 2*ld when the lo plane exists, see ns2_common.h); a_zs / out_zs are logical column offsets
  const bf16_t* a_hi = nullptr; const bf16_t* a_lo = nullptr; int lda = 0;
  // W operand: packed weights, bf16 split planes [ceil(N/128)*128, ldw], K contiguous
  const bf16_t* w_hi = nullptr; const bf16_t* w_lo = nullptr; int ldw = 0;
  const bf16_t* w_tl = nullptr;   // optional: the same FMT_H8 linear weight as tiled LDS images (gemm3_kernel.h); null = none
  const bf16_t* w_tw1 = nullptr; const bf16_t* w_tw2 = nullptr;   // optional (EPI_WAVENET, hybrid plan): tiled images of the dilated conv's half parts / of the res conv (wavenet3_kernel.h)
  const bf16_t* w_t3 = nullptr;   // optional: the same conv weight (k = 3, dense IEEE half) as tiled LDS images (ffconv_kernel.h); null = none
  int M = 0, N = 0;      // N = valid output columns
  int nkt = 0;           // number of 32-wide K tiles (total, all taps/phases)
  int kt_per_tap = 0;    // K tiles per tap (plain linear: == nkt)
  int conv_taps = 0;     // taps [0, conv_taps) are causal-shifted by (conv_taps-1-tap)*dil rows; later taps unshifted
  int dil = 1; int dil_z = 0;   // dilation; if dil_z the effective dilation is dil << blockIdx-z
  int seq_len = 0;       // tokens per utterance (rows never read across an utterance start); 0 = no sequence structure
  int mid_kt = -1;       // EPI_WAVENET: K tile index at which the gate transform runs
  int p1_half = 0;       // EPI_WAVENET at precision 4: the taps before mid_kt run as ONE half product (no fp8 correction terms, the byte half of the lines is not fetched)
  int epi = EPI_F32;
  // epilogue operands
  const float* bias = nullptr; const float* bias2 = nullptr;
  const float* film = nullptr; int film_ld = 0;   // gamma at film[b*film_ld + col], beta at film[b*film_ld + N + col]
  const float* resid = nullptr; int ldr = 0;
  float* out_f = nullptr; int ldo_f = 0;
  long out_f_zs = 0;     // EPI_F32 with nz > 1: slice z writes out_f + z * out_f_zs (split-K partial sums of the weight gradients)
  bf16_t* out_hi = nullptr; bf16_t* out_lo = nullptr; int ldo_s = 0; int out_ncols = 0;   // writes columns [0, out_ncols) (zero beyond N)
  bf16_t* vt_hi = nullptr; bf16_t* vt_lo = nullptr; int vt_ld = 0; int vt_rows = 0; int split_col = 0;
  // batching over blockIdx-z (wavenet columns): element offsets per z
  int nz = 1; long a_zs = 0, w_zs = 0, bias_zs = 0, film_zs = 0, out_zs = 0;
  int pad_left = -1;     // conv: zero rows in front of the sequence (-1 = causal: conv_taps-1); k=9 'same' padding = 4
  int act = 0;           // 1 = SiLU after the bias (EPI_F32 / EPI_SPLIT)
  int out_fmt = -1;      // PlaneFmt of the split-plane output (ns2_common.h).  -1 = operand_fmt(precision).  Attention operands (q, k:
                         // EPI_QKV columns < split_col, the cross-attention q projection) are attention_fmt(precision).
  int vt_fmt = -1;       // PlaneFmt of the transposed value planes (FMT_BF16 or FMT_F16); -1 = attention_fmt(precision)
  // Split-K for products too small to fill the chip (a batch of 1 ... 4 utterances: 8 ... 100 output tiles on 256 CUs, each a
  // serial K loop).  The caller lends scratch (sk_ws: fp32, sk_ws_floats elements; null = never split); launch_gemm then runs
  // the 128x128 kernel over grid-z K slices writing raw fp32 partial sums into fixed slots and a second launch that adds the
  // slots in slot order and applies the requested epilogue -- deterministic.  ksplit is set by launch_gemm: K tiles of EVERY tap
  // one slice covers (slice z: input columns [z * ksplit * 32, ...) of each tap); 0 = the plain launch.
  float* sk_ws = nullptr; long sk_ws_floats = 0;
  int ksplit = 0;
  // EPI_F32 on the 128 x 128 kernel with N == 128 (the dim = 128 model: a workgroup owns WHOLE rows): the RMSNorm that follows the
  // residual stream's update (NS2:727-746, 794-807) inside the same epilogue -- out_f = acc + bias + resid as always, then
  // nrm planes = F.normalize(out_f row) * sqrt(N) [* nrm_gamma] [* cond_g + cond_b] in format nrm_fmt, the next GEMM's operand.
  // nrm_hi == null: not requested.  gemm_fuses_norm() says whether launch_gemm will honour it for a given shape.
  bf16_t* nrm_hi = nullptr; bf16_t* nrm_lo = nullptr; int nrm_ld = 0, nrm_fmt = 0;
  const float* nrm_gamma = nullptr; const float* nrm_cond = nullptr; int nrm_cond_ld = 0, nrm_seq_len = 0;
  // launch_gemm_tr only (weight gradients from token-major planes, gemm2.hip TR): tokens the operands have, channels per tap block of
  // the N dimension (a multiple of 32), taps (0 / 1: no shift; tap t of a causal conv reads token m - (tr_taps - 1 - t) * dil)
  int tr_tokens = 0, tr_kp = 0, tr_taps = 0;
  // ragged skipping (include/ns2hip.h; last in the block: no other field moves): per-utterance frame counts in DEVICE
  // memory, int32 [M / lens_seq], read by the kernels alone, and the frames per utterance (a multiple of 256 that divides M).  Selects
  // the SKIP instantiations: a workgroup whose whole row tile lies at or behind its utterance's computed extent
  // min(lens_seq, 256 ceil(clamp(len, 1, lens_seq) / 256)) returns before its first load -- an fp32 output without a residual gets
  // zeros there, every other output keeps what it held.  null = every row is computed.  The split-K route takes no lengths.
  const int* row_lens = nullptr; int lens_seq = 0;
  // ragged skipping in the TRAINING pass (include/ns2hip_train.h; appended: no other field moves).  With row_lens: a hidden
  // tile of EVERY output -- fp32 with or without a residual, operand planes of either format, V^T -- is stored as zero bits instead of
  // being left as it was (gemm_epi.h zero_hidden_tile): the buffers of the pass come uninitialised, and the anticausal dgrads and the
  // kernels that do not skip read behind an utterance's extent.  0 = the sampling rule above.  launch_gemm_tr (weight gradients) with
  // row_lens: the LENS instantiations, which step over the 32-token K tiles behind an extent; it has no hidden output.
  int zero_hidden = 0;
};
// may g carry row_lens?  (what launch_gemm checks, and the stand-alone entries before any device call)
inline bool gemm_lens_ok(const GemmArgs& g) { return g.lens_seq > 0 && (g.lens_seq & 255) == 0 && g.M > 0 && (g.M % g.lens_seq) == 0; }

// precision: 3 = bf16 x3 ("exact"), 1 = bf16 ("fast"), 2 = one IEEE-half product ("half"), 4 = half product + both
// first-order correction terms on the fp8 MFMA ("mixed", FMT_H8 operands).  Dispatches gemm.hip / gemm2.hip by shape.
hipError_t launch_gemm(const GemmArgs& g, int precision, hipStream_t s);
bool gemm_fuses_norm(const GemmArgs& g, int precision);                 // gemm2.hip: launch_gemm would run the norm nrm_* requests in the product's epilogue
hipError_t launch_gemm_tr(const GemmArgs& g, int precision, hipStream_t s);   // gemm2.hip: both operands read transposed (precision 3 / 4)
void splitk_plan(int M, int N, int nkt, int kt_per_tap, bool epi_f32, long scratch_floats, int* S, int* c);   // gemm2.hip; S = 1: no split
void force_gemm_kernel(int k);                                          // test hook, the modes of ns2_debug_force_gemm (include/ns2hip.h); decoded by gemm2.hip gemm_hook()
// the dedicated FF causal conv kernel (ffconv_kernel.h, compiled in gemm2.hip): tiled weight images
size_t ffconv3_tiled_bytes_of(int N, int Cp);
hipError_t ffconv3_build_tiles(const bf16_t* w_hi, int ldw, int Cp, int rows_p, int N, bf16_t* out, hipStream_t s);
int ffconv3_lda(int Cp);                                                  // activations' row length (elements) the kernel wants for Cp packed columns per tap
// the lean mixed linear kernel (gemm3_kernel.h, compiled in gemm2.hip): tiled weight images of an FMT_H8 pack [rows_p][ldk]
size_t gemm3_tiled_bytes_of(int rows_p, int nkt);
hipError_t gemm3_build_tiles(const bf16_t* w_hi, int ldk, int rows_p, bf16_t* out, hipStream_t s);
// the lean Wavenet block kernel of the hybrid plan (wavenet3_kernel.h): tiled images of a stack's nz matrices [rows_p][4 dp]
size_t wavenet3_tiles_bytes(int rows_p, int dp, int nz, int phase);
hipError_t wavenet3_build_tiles(const bf16_t* w_hi, int rows_p, int dp, int nz, bf16_t* t1, bf16_t* t2, hipStream_t s);
constexpr long SPLITK_SCRATCH_FLOATS = 512L * 128 * 128;                // what any split needs at most: slices x output tiles <= 512 tiles of 128 x 128 (32 MiB)

// flash attention forward, head dim 64, non-causal (ATT:77-155 hot path).  Every field has a default: a default-constructed block is a
// valid "nothing optional" block, and a caller names only what it uses (capi.cpp attn_args_from, model_exec.cpp attention_call)
struct AttnArgs {
  const bf16_t* q_hi = nullptr; const bf16_t* q_lo = nullptr; int ldq = 0;     // [B*Nq, ldq], head h at columns q_col0 + 64h
  const bf16_t* k_hi = nullptr; const bf16_t* k_lo = nullptr; int ldk = 0;     // [B*Nk, ldk], head h at columns k_col0 + 64h
  const bf16_t* vt_hi = nullptr; const bf16_t* vt_lo = nullptr; int vt_ld = 0; // [B][H*64][vt_ld] transposed values
  bf16_t* o_hi = nullptr; bf16_t* o_lo = nullptr; int ldo = 0;                 // [B*Nq, ldo], head h at columns 64h
  int o_fmt = -1;                                      // PlaneFmt of o (-1: the operand format; FMT_H8 feeds a precision-4 GEMM)
  int q_col0 = 0, k_col0 = 0;
  int B = 0, H = 0, Nq = 0, Nk = 0;
  int D = 0;                                           // head dimension: 32, 64 or 128 (0 = 64); head h at columns col0 + D h, V^T rows H D per utterance
  float scale = 0.f;
  const unsigned char* kmask = nullptr;                  // optional key-padding mask [B, Nk], 1 = attend (ATT:92-94, 136-138)
  float* lse = nullptr;                                  // optional [B, H, Nq]: log2 of the softmax denominator of the SCALED scores
                                                         // (m + log2 l), what the backward kernels recompute P from; null = not wanted
  // attention dropout of the training kernel (dropout_keep.h; needs lse and precision 3): drop_seed = two 32-bit words in DEVICE memory
  // (null = no dropout), drop_thr = round(p 2^32), drop_scale = 1 / (1 - p), drop_call = index of this attention inside the pass
  const uint32_t* drop_seed = nullptr; uint32_t drop_thr = 0u, drop_call = 0u; float drop_scale = 1.f;
  // ragged batches (include/ns2hip.h): per-utterance key counts in DEVICE memory, int32 [B], read by the kernels alone (never on
  // the host: a captured launch follows rewritten values).  Utterance b attends to keys [0, clamp(klens[b], 1, Nk)); keys beyond are
  // treated as keys beyond Nk are (score -inf, K rows and V^T columns read as zeros, so they may hold anything); Nk stays the stride.
  // null = every utterance has Nk keys.  Excludes kmask and dropout.  Together with lse (the training forward of a ragged batch,
  // include/ns2hip_train.h; precision 3, Nq == Nk): the counts are the utterances' lengths on the query side too -- o rows from the
  // length on are written as zero bits, their lse as +inf.
  const int* klens = nullptr;
  // ragged skipping (include/ns2hip.h; last in the block): per-utterance frame counts on the QUERY side, int32 [B] in DEVICE
  // memory; needs Nq % 256 == 0.  A query workgroup whose rows all lie at or behind min(Nq, 256 ceil(clamp(qlens[b], 1, Nq) / 256)) returns
  // before its first load and leaves its o rows as they were; every other row is computed as without it.  With or without klens (the
  // cross attention to the resampled prompt has query lengths alone).  Excludes lse, kmask and dropout.  null = every query row is computed.
  const int* qlens = nullptr;
};                                                       // precision: 3 bf16x3, 1 bf16, 2 and 4: one IEEE-half product
hipError_t launch_attention(const AttnArgs& a, int precision, hipStream_t s);
hipError_t launch_attention_train_hd(const AttnArgs& a, hipStream_t s);   // the training forward (lse, precision 3) at a.D = 32 / 64 / 128
long long attention_fast_launches();                                   // test hook: launches that took attn_fast_kernel so far (ns2_debug_attention_fast_launches)
void force_attention_kernel(int k);                                     // test hook, the modes of ns2_debug_force_attention (include/ns2hip.h); decoded in attention.hip

// RMSNorm (NS2:727-746): out = x / max(|x|, 1e-12) * sqrt(d) [* gamma] [* g_c + b_c]  -> split planes
struct NormArgs {
  const float* x; int ldx;           // [M, d]
  const float* gamma;                // [d] or null
  const float* cond; int cond_ld;    // adaptive: g_c = cond[b*cond_ld + c], b_c = cond[b*cond_ld + d + c]; null = plain
  bf16_t* out_hi; bf16_t* out_lo; int ldo;
  float* out_f; int ldo_f;           // optional fp32 copy (e.g. resampler output)
  int M, d, seq_len;
  int fmt;                           // PlaneFmt of the output planes
};
hipError_t launch_rmsnorm(const NormArgs& a, hipStream_t s);
void force_norm_kernel(int k);      // test hook, the modes of ns2_debug_force_norm (include/ns2hip.h): 0 by shape, 1 = rmsnorm_kernel for every call
int norm_kernel_last();             // which kernel the last launch_rmsnorm ran: 1 = rmsnorm_kernel, 2 = rmsnorm_wide_kernel (0: none yet)

// x (+ add) -> split planes, with optional zero padding to ldo columns
hipError_t launch_split(const float* x, int ldx, const float* add, int ldadd, int add_rows_per_batch, int add_valid_rows,
                        bf16_t* out_hi, bf16_t* out_lo, int ldo, int M, int d, int seq_len, hipStream_t s, int fmt = 0);

// LearnedSinusoidalPosEmb + Linear(d+1, dt) + SiLU (NS2:108-120, 839-843): times[B] -> out[B, ld_out] columns [0, dt)
// wt is the Linear weight stored K-major [dim+1, dt]; feat_ws is a [B, dim+1] fp32 scratch.
hipError_t launch_time_embed(const float* times, const float* freqs, const float* wt, const float* bias, float* feat_ws,
                             float* out, int ld_out, int B, int dim, int dt, float* ws, size_t ws_bytes, hipStream_t s, int plan_B = 0);

// out[b, j] = act( sum_k in[b,k] * wt[k, j] + bias[j] ), wt stored K-major ([K, J]); act 0 none, 1 SiLU
// ws: caller-owned scratch of skinny_linear_workspace_bytes(B, K, J) for the split-K partial sums (null: no K split)
// plan_B > 0: split K as a batch of plan_B rows would (same order of partial sums: ns2_model_time_table)
size_t skinny_linear_workspace_bytes(int B, int K, int J, int plan_B = 0);
hipError_t launch_skinny_linear(const float* in, int ld_in, const float* wt, const float* bias, float* out, int ld_out,
                                int B, int K, int J, int act, float* ws, size_t ws_bytes, hipStream_t s, int plan_B = 0);
hipError_t launch_param_sample(const float* const* ptrs, const long* numels, int n, float* out, hipStream_t s);
hipError_t launch_add_row(const float* row, const float* add, float* out, int B, long J, hipStream_t s);

// batched fp32 [R, C] -> [C, R]
hipError_t launch_transpose_f32(const float* in, int batch, int R, int C, float* out, hipStream_t s);

// mean over n of [B, n, d] -> [B, d]
hipError_t launch_mean_rows(const float* in, int B, int n, int d, float* out, hipStream_t s);
// ragged_front.hip: the mean over rows [0, clamp(lens[b], 1, n)) of utterance b (ascending rows); out[b] = offset + clamp(lens[b], 1, n)
hipError_t launch_mean_rows_lens(const float* in, int B, int n, int d, const int* lens, float* out, hipStream_t s);
hipError_t launch_offset_lens(const int* lens, int B, int n, int offset, int* out, hipStream_t s);

// out[b*ld_out + e] = src[e] for e < row_elems (broadcast a parameter row over the batch)
hipError_t launch_bcast_rows(const float* src, float* out, int B, long row_elems, long ld_out, hipStream_t s);

hipError_t launch_embedding(const int64_t* ids, const float* table, float* out, long n, int dim, long pad_id, hipStream_t s);
hipError_t launch_join(const bf16_t* hi, const bf16_t* lo, int ld, float* out, int ldo, long M, int d, hipStream_t s, int fmt = 0);
hipError_t launch_transpose_into(const float* src, int R, int C, float* dst, long ld_dst, long col_off, hipStream_t s);

// DDIM update (NS2:1396-1429), objective 'v'/'eps'/'x0', sigmoid/cosine/linear schedule evaluated on device
struct DdimArgs {
  float* audio; const float* model_out; float* out;   // [B, n*d]; out may alias audio
  const float* times; const float* times_next;        // [B]
  int B; long per_batch;
  int objective;     // 0 'v', 1 'eps', 2 'x0'
  int schedule;      // 0 sigmoid, 1 cosine, 2 linear
  float scale;
};
hipError_t launch_ddim(const DdimArgs& a, hipStream_t s);

// CFG mix: out = null + (cond - null) * scale   (NS2:927)
hipError_t launch_cfg_mix(const float* cond, const float* null, float* out, long n, float scale, hipStream_t s);

// weight packing: fp32 [rows, C, T] (T taps, 1 for linear) -> split planes [rows_p, T*Cp]; row_map[r] = source row or -1
// one rectangular part of a packed weight and where its fp32 values live (elementwise.hip repack_kernel; built by ns2_weights_repack_build)
struct RepackDesc {
  const float* src; long sr, sc, st;        // element (r, c, tap) of the part at src[r * sr + c * sc + tap * st] (element strides, may be negative)
  bf16_t* dst_hi; long drs;                 // packed weight: first plane, physical row stride
  int row0, rows, col0, cols;               // packed rows [row0, row0 + rows), packed columns (per tap) [col0, col0 + cols)
  int Cp, T, fmt, il;                       // packed columns per tap, taps, PlaneFmt, interleaved lines
  long block0; int chunks, pad_;            // first block of the part, 256-element chunks per packed row
};
hipError_t launch_repack(const RepackDesc* tab, int n, long total_blocks, hipStream_t s);
hipError_t launch_pack_weight(const float* src, int C, int T, int Cp, const int* row_map, int rows_p, bf16_t* dst_hi,
                              bf16_t* dst_lo, int ldk, int k_off, hipStream_t s, int fmt = 0);
// the feed-forward fold (elementwise.hip): w_fold [dim, f, 3] = w_out [dim, f] . w_conv [f, f, 3], b_fold [dim] = w_out . b_conv + b_out
// (b_out may be null), fp32 FMAs in ascending order of the contracted index
hipError_t launch_ff_fold(const float* w_out, const float* w_conv, const float* b_conv, const float* b_out, int dim, int f, float* w_fold,
                          float* b_fold, hipStream_t s);
// the Wavenet tail fold (elementwise.hip): w_fold [dim, L * dim] = w_final [dim, dim] . [w_skip[0] | ... | w_skip[L - 1]] (w_skip [L, dim, dim]),
// b_fold [dim] = w_final . sum_l b_skip[l] + b_final (b_skip [L, dim]; b_final may be null), under the same rules
hipError_t launch_tail_fold(const float* w_final, const float* w_skip, const float* b_skip, const float* b_final, int dim, int L,
                            float* w_fold, float* b_fold, hipStream_t s);

// EnCodec residual VQ encode (HFENC:364-369, 424-447)
struct RvqArgs {
  const float* x;            // [M, D] latents
  const float* codebooks;    // [Q, C, D]
  const float* cb_norm;      // [Q, C] 0.5*|e|^2 (from launch_rvq_prepare)
  int64_t* codes;            // [M, Q]
  float* emb;                // [M, D] sum of selected codes (may be null)
  float* residual;           // [M, D] final residual (may be null)
  int* near_tie_count;       // optional counter of fp64 re-checks taken
  int M, Q, C, D;
  float tie_eps;
};
// EnCodec SEANet helpers (elementwise.hip): pre-convolution activation + reflect prefix + operand planes; prefix removal;
// one nn.LSTM layer (recurrent part; the input projections are a GEMM)
hipError_t launch_seanet_prep(const float* x, int ldx, int in_prefix, const float* add, int ldadd, int B, long T, int C, int elu,
                              int prefix, int im2col_k, bf16_t* out_hi, bf16_t* out_lo, int ldo, int fmt, hipStream_t s);
hipError_t launch_seanet_prep2(const float* x, int ldx, int in_prefix, int B, long T, int C, int prefix, bf16_t* elu_hi, bf16_t* elu_lo,
                               int elu_ld, int elu_col0, int elu_cols, bf16_t* raw_hi, bf16_t* raw_lo, int raw_ld, int raw_col0,
                               int raw_cols, int fmt, hipStream_t s);
hipError_t launch_seanet_conv_narrow(const float* x, long ldx, int in_prefix, int B, long T, int ci, int co, int k, int elu, const float* w,
                                     const float* bias, float* out, long ldo, hipStream_t s);
hipError_t launch_seanet_resblock_narrow(const float* x, long ldx, int in_prefix, int B, long T, int C, const float* w1p, const float* b1,
                                         const float* w2p, const float* wsp, const float* b2s, float* out, long ldo, hipStream_t s);
hipError_t launch_seanet_unpad(const float* src, long ld_src, int prefix, float* dst, long ld_dst, int B, long T, int C, hipStream_t s);
long lstm_state_floats(int B, int H);     // caller scratch of launch_lstm_layer (h exchange, cell state / barrier counter)
hipError_t launch_lstm_layer(const float* xproj, long ld_x, const float* w_hh, const float* b_hh, float* h_a, float* h_b,
                             float* c_state, long state_floats, const float* resid, long ld_r, float* out, long ld_o, int B,
                             long T, int H, hipStream_t s);

// both layers of a 2-layer LSTM (H = 512) in one launch, layer 2 overlapped with layer 1; hipErrorNotReady = not available on
// this device / switched off: run the layers one after the other
long lstm2_state_floats();
hipError_t launch_lstm2(const float* xproj, long ld_x, const float* w_hh1, const float* b_hh1, const float* w_ih2, const float* b_ih2,
                        const float* w_hh2, const float* b_hh2, float* state, long state_floats, const float* resid, long ld_r, float* out,
                        long ld_o, int B, long T, hipStream_t s);

hipError_t lstm_abort_inject(unsigned int n);   // test hook
unsigned int lstm_abort_read(bool reset);   // persistent-LSTM launches that gave up at their step barrier since the last reset (synchronising)

hipError_t launch_rvq_prepare(const float* codebooks, float* cb_norm, int Q, int C, int D, hipStream_t s);
hipError_t launch_rvq_encode(const RvqArgs& a, hipStream_t s);
// decode: emb[m] = sum_q codebooks[q][codes[m][q]]  (HFENC:440-447)
hipError_t launch_rvq_decode(const int64_t* codes, const float* codebooks, float* emb, int M, int Q, int C, int D,
                             hipStream_t s);

// RVQ cross-entropy of the training loss (rvq_ce.hip; NS2:1668-1684): row losses, their fixed-order mean, and optionally the sum of the
// nearest codes and the unit gradient G = d loss / d x, all from one walk over the codebooks
struct RvqCeArgs {
  const float* x;            // [M, D] rows (the predicted x_start)
  const float* codebooks;    // [Q, C, D]
  const float* cb_norm;      // [Q, C] 0.5*|e|^2 (from launch_rvq_prepare)
  const int64_t* targets;    // [M, Q] the codec's own codes; outside [0, C): that row's loss (and row of G) is NaN
  float* row_loss;           // [M, Q] lse_c(-dist) + dist_target
  float* loss;               // [1] sum_q mean_m row_loss
  int64_t* nearest;          // [M, Q] nearest code per stage (null unless quantized_out is wanted)
  float* quantized_out;      // [M, D] 0 + E_0[nearest_0] + E_1[nearest_1] + ... (may be null)
  float* grad;               // [M, D] G, already divided by M (may be null: no second sweep)
  int M, Q, C, D;
};
hipError_t launch_rvq_ce(const RvqCeArgs& a, hipStream_t s);
// ... of a ragged batch (ns2_rvq_ce_lens, include/ns2hip_train.h): M = B n rows, utterance b owns rows [b n, b n + row_lens[b]); the loss is the mean
// over utterances of each utterance's own mean, G of a row is divided by B row_lens[b], and every output row at or behind a length is 0
struct RvqCeLensArgs : RvqCeArgs {
  const int* row_lens;       // [B] on the device, clamped into [1, n] by the kernels
  int B, n;
};
hipError_t launch_rvq_ce_lens(const RvqCeLensArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------- backward pass (backward.hip)
// fp32 [M, C] (xf) or operand planes (in_hi / in_lo, interleaved bf16 hi/lo) -> row planes and / or TRANSPOSED planes
// T[c][m] (the operands of the weight-gradient GEMMs and of the attention backward), optionally shifted along the token axis
// inside each utterance: T[c][m] = in[m - shift][c] if m - shift lies in the utterance of m, else 0.
struct TPlanesArgs {
  const float* xf; long ldx;
  const bf16_t* in_hi; const bf16_t* in_lo; int ld_in; int in_col0;
  int M, C;
  int seq_len, shift;
  bf16_t* row_hi; bf16_t* row_lo; int ld_row;      // optional (fp32 input, shift 0): planes [M, ld_row], zero beyond C
  bf16_t* t_hi; bf16_t* t_lo; long ld_t;           // optional transposed planes, ld_t (logical, multiple of 32) token columns, zero beyond
  int per_batch;                                   // 0: row c, column m (all M tokens); 1: row b * t_rows_per_batch + c, column n
  int t_rows_per_batch; int t_rows;                // rows written (>= C, zeros beyond C): per utterance / in total
  float* colsum_partial;                           // optional (fp32 input): [slices][C] column sums of 64-row tiles (bias gradients)
  int fmt;                                         // FMT_BF16 (hi / lo lines) or FMT_H8 (the mixed training arithmetic): the format of the
                                                   // input planes, of the row planes and of the transposed planes alike
};
hipError_t launch_tplanes(const TPlanesArgs& a, hipStream_t s);
long tplanes_slices(int M, long ld_t);             // number of 64-row tiles (= colsum slots) of a non-per_batch launch
hipError_t launch_reduce_slices(const float* partial, long outer, int S, long inner, float* out, int accumulate, hipStream_t s);
// training the DurationPitchPredictor (duration_pitch.hip): backward of GroupNorm + SiLU from the forward's statistics slots, of the heads
int gn_bwd_row_chunks(int n);
int row_dot_bwd_chunks(long M);
hipError_t launch_groupnorm_silu_bwd(const float* dy, long lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                                     const float* bias, float eps, const void* stats, float* dx, float* dwb, float* slots, float* colsum,
                                     hipStream_t s, const int* row_lens = nullptr);   // row_lens: ns2_groupnorm_silu_bwd_lens
hipError_t launch_row_dot_relu_bwd(const float* dout, const float* out, const float* h, long ldh, const float* w, long M, int K, float* dh,
                                   long lddh, float* dwb, float* slots, hipStream_t s);
hipError_t launch_wgrad_reduce(const float* partial, int S, int R, long ldp, int T, int Kp, int K, float* out, hipStream_t s);
hipError_t launch_film_gate_fwd(const float* h, long ldh, const float* film, int film_ld, int seq_len, long M, int d, float* out,
                                long ldo, hipStream_t s);
int film_gate_slices(int seq_len);
hipError_t launch_film_gate_bwd(const float* dg, long lddg, const float* h, long ldh, const float* film, int film_ld, int B, int seq_len,
                                int d, float* dh, long lddh, float* partial, hipStream_t s);
hipError_t launch_geglu_fwd(const float* pre, long ldp, long M, int f, bf16_t* out_hi, bf16_t* out_lo, int ldo, hipStream_t s, int fmt = 0);
hipError_t launch_geglu_bwd(const float* dh, long lddh, const float* pre, long ldp, long M, int f, float* dpre, long lddp, hipStream_t s);
struct NormBwdArgs {
  const float* x; long ldx;            // the norm's input [B * seq_len, d]
  const float* dy; long lddy;          // gradient of its output
  const float* gamma;                  // learned scale [d] or null
  const float* cond; int cond_ld;      // adaptive [gamma_c | beta_c] per utterance or null
  const float* dx_add; float* dx; long lddx;   // dx = (dx_add ? dx_add : 0) + d(loss)/dx ; dx may alias dx_add
  float* cond_partial;                 // [B * slices][2 d] (required with cond)
  float* gamma_partial;                // [B * slices][d] or null
  int B, seq_len, d;
};
int rmsnorm_bwd_slices(int seq_len);
hipError_t launch_rmsnorm_bwd(const NormBwdArgs& a, hipStream_t s);
hipError_t launch_attn_delta(const float* dO, long lddo, const bf16_t* o_hi, const bf16_t* o_lo, int ldo, int B, int H, int Nq, float* delta,
                             hipStream_t s, int o_fmt = 0);
hipError_t launch_attn_delta_hd(const float* dO, long lddo, const bf16_t* o_hi, const bf16_t* o_lo, int ldo, int B, int H, int Nq, int D,
                                float* delta, hipStream_t s, int o_fmt);      // heads of D = 32 / 64 / 128 columns
struct AttnBwdArgs {                                                // (every field defaulted, as in AttnArgs)
  const bf16_t* q_hi = nullptr; const bf16_t* q_lo = nullptr; int ldq = 0, q_col0 = 0;    // [B*Nq, ldq], head h at columns q_col0 + 64 h
  const bf16_t* k_hi = nullptr; const bf16_t* k_lo = nullptr; int ldk = 0, k_col0 = 0;    // [B*Nk, ldk]
  const bf16_t* v_hi = nullptr; const bf16_t* v_lo = nullptr; int ldv = 0, v_col0 = 0;    // [B*Nk, ldv] values, ROW-major
  const bf16_t* do_hi = nullptr; const bf16_t* do_lo = nullptr; int lddo = 0;             // [B*Nq, lddo] gradient of the attention output, head h at 64 h
  const float* lse = nullptr; const float* delta = nullptr;                               // [B, H, Nq]
  float* dq = nullptr; int lddq = 0, dq_col0 = 0;                                         // fp32 outputs (null = not wanted; dk and dv come together)
  float* dk = nullptr; int lddk = 0, dk_col0 = 0;
  float* dv = nullptr; int lddv = 0, dv_col0 = 0;
  int B = 0, H = 0, Nq = 0, Nk = 0; float scale = 0.f;
  // round 5: the gradients as OPERAND PLANES instead of fp32 (what consumes dq | dk | dv of a self attention is the q | k | v projection's
  // dgrad and wgrad GEMMs, nothing else): gp planes [rows, gp_ld] in format gp_fmt (FMT_BF16 hi / lo lines or FMT_H8), dq at columns
  // dq_col0 + 64 h of row b Nq + q, dk / dv at dk_col0 / dv_col0 of row b Nk + k; gp_q / gp_kv say which halves go there
  bf16_t* gp_hi = nullptr; bf16_t* gp_lo = nullptr; int gp_ld = 0, gp_fmt = 0, gp_q = 0, gp_kv = 0;
  // the encoders' training pass: key-padding mask [B, Nk] (1 = attend; null = none) and attention dropout as in AttnArgs (drop_seed null =
  // none).  Either one selects the MD instantiations of the kernel; without them the kernels of the denoiser's pass run, unchanged.
  const unsigned char* kmask = nullptr; const uint32_t* drop_seed = nullptr; uint32_t drop_thr = 0u, drop_call = 0u; float drop_scale = 1.f;
  // ragged training batches (include/ns2hip_train.h): per-utterance lengths in DEVICE memory, int32 [B], read by the kernels alone.
  // Self-attention only (Nq == Nk); utterance b's gradients are those of rows [0, clamp(lens[b], 1, N)) alone, rows beyond are written as
  // zeros, N stays the stride.  Selects the LENS instantiations; excludes kmask and dropout.  null = every utterance has N rows.
  const int* lens = nullptr;
};
hipError_t launch_attention_bwd(const AttnBwdArgs& a, hipStream_t s);
hipError_t launch_attention_bwd_hd(const AttnBwdArgs& a, int D, hipStream_t s);      // head h at columns col0 + D h, D = 32 / 64 / 128

// the encoders' training pass (backward.hip): SiLU forward / backward on fp32 rows, the deterministic embedding gradient, and the
// dropout keep mask of dropout_keep.h as bytes [B, H, Nq, Nk]
hipError_t launch_silu_fwd(const float* x, long ldx, long M, int C, float* out, long ldo, hipStream_t s);
hipError_t launch_silu_bwd(const float* dy, long lddy, const float* x, long ldx, long M, int C, float* dx, long lddx, hipStream_t s);
hipError_t launch_relu_fwd(const float* x, long ldx, long M, int C, float* out, long ldo, hipStream_t s);
hipError_t launch_relu_bwd(const float* dy, long lddy, const float* x, long ldx, long M, int C, float* dx, long lddx, hipStream_t s);
hipError_t launch_embedding_bwd(const long long* ids, long M, int pad_id, const float* dy, long lddy, int rows, int d, float* dw, hipStream_t s);
hipError_t launch_dropout_keep_mask(const uint32_t* seed, uint32_t call, float p, int B, int H, int Nq, int Nk, unsigned char* out, hipStream_t s);

// training the Aligner (aligner.hip): backward of the distances + softmax, the forward-sum (CTC) and bin losses and their gradient
int64_t align_attn_bwd_workspace_bytes(int B, int T, int n, int C);
hipError_t launch_align_attn_bwd(const float* q, const float* k, const float* aln_log, const float* aln_soft, const float* g_log,
                                 const float* g_soft, const int* text_lens, int B, int T, int n, int C, float* dq, float* dk,
                                 void* workspace, hipStream_t s);
int64_t align_losses_workspace_bytes(int B, int T, int n);
hipError_t launch_align_losses_fwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, int B, int T, int n,
                                   float blank, float* fs_loss, float* bin_loss, void* workspace, hipStream_t s);
hipError_t launch_align_losses_bwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, const float* g_fs,
                                   const float* g_bin, int B, int T, int n, float blank, float* d_log, void* workspace, hipStream_t s);

// the YIN pitch estimator (pitch.hip; include/ns2hip_audio.h states the formula): audio [B, L] -> f0 [B, 1 + L / hop] in Hz, 0 unvoiced.
// The caller (capi.cpp) has checked 2 <= tau_min < tau_max <= PITCH_TAU_MAX, hop >= 1, L >= 1, 1 <= B <= 65535
constexpr int PITCH_TAU_MAX = 1024;
hipError_t launch_pitch_yin(const float* audio, int B, long L, long T, int sample_rate, int hop, int tau_min, int tau_max, float threshold,
                            float* f0, hipStream_t s, const int* sample_lens = nullptr);   // sample_lens [B] on the device: ns2_pitch_yin_lens

}  // namespace ns2
