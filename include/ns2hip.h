/* libns2hip — C ABI of the MI355X-native NaturalSpeech2 denoising hot path.
 *
 * The reference (lucidrains/naturalspeech2-pytorch) has no FFI/plugin layer: its boundary for this path is the
 * Python class surface.  This header is the core of the C-ABI a host binds instead -- what sampling needs; the
 * conditioning front-end (ns2hip_frontend.h), raw audio and the codec (ns2hip_audio.h), the training pass (ns2hip_train.h) and the
 * optimizer step (ns2hip_optim.h) have a header each, under the conventions stated here.  Each entry point cites the
 * reference interface it replaces (NS2 = naturalspeech2_pytorch/naturalspeech2_pytorch.py, ATT = attend.py,
 * HFENC = transformers/models/encodec/modeling_encodec.py, the restatement of the un-vendored encodec RVQ).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is named host_*; the caller owns all buffers
 *     (inputs, outputs, workspaces); the library owns only packed-weight blobs (ns2_weight / ns2_model).
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); calls are stream-ordered and never
 *     synchronise the device, except ns2_model_finalize / ns2_weight_pack which are one-time set-up calls.
 *   - return value 0 = ok; otherwise a negative code, message via ns2_last_error() (thread-local).
 *   - activations travel between kernels as 16-bit "split planes": hi = bf16(x), lo = bf16(x - hi).  precision
 *     3 = hi*hi+hi*lo+lo*hi on the bf16 MFMA (fp32-class, matches the fp32 reference to 1e-5), 1 = bf16 hi only,
 *     2 = ONE IEEE-half plane (x_lo == NULL, values saturate at +-65504) multiplied on the f16 MFMA, fp32 accumulate,
 *     4 = "mixed": the IEEE-half product plus BOTH first-order correction terms (a_hi.w_lo + a_lo.w_hi) evaluated in one
 *         block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, e5m2 operands) per 32-deep k block: 4e-5-class accuracy
 *         at two thirds of the MFMA work of precision 3.
 *   - the library keeps no mutable host state on a launch path and never allocates there: scratch is caller-owned
 *     (ns2_*_workspace_bytes), constants live in per-device __device__ storage, so one host thread per device (or one
 *     process per device) may drive several devices concurrently, also under stream capture.  What it does keep, all of it
 *     write-once or atomic: per-device "attribute raised" / occupancy answers, the environment switches NS2_GEMM,
 *     NS2_LSTM_PERSISTENT and NS2_LSTM_FUSED (read once per process), and the test hooks ns2_debug_*.  One thread-local
 *     pointer exists for the duration of a ns2_model_forward* / ns2_model_prepare_cond call: the split-K region of the
 *     workspace that call was given (set on entry, restored on return).
 *   - layout of a split-plane matrix (x_hi, x_lo, ld): `ld` is the LOGICAL column count, a multiple of 32.
 *     x_lo != NULL: ONE bf16 buffer [rows, 2*ld]; every 32 logical columns occupy a 128-byte line [hi(32) | lo(32)],
 *       i.e. element (r, c) has hi at r*2*ld + ((c & ~31) << 1) + (c & 31) and lo 32 elements further; the caller
 *       passes x_lo == x_hi + 32 (anything else is NS2_ERR_HIP / invalid value).  precision 3 needs this form.
 *     x_lo == NULL: the dense [rows, ld] hi plane alone (precision 1: bf16, precision 2: IEEE half).
 *     precision 4 operands use the interleaved form with the line [half(32) | e5m2(x)(32 B) | e5m2((x-half(x))*2^12)(32 B)]
 *       (x_lo == x_hi + 32 as above); the operands of ns2_attention_fwd (q, k, transposed values) are dense IEEE half at
 *       precision 4, which is also what the fused q | k | v form of ns2_linear writes there.
 *     Transposed value planes (vt_hi, vt_lo, vt_ld) use the same rule along the key axis.
 *
 * Ragged batches.  The entries named *_lens, *_lens_zero and *_skip take per-utterance lengths; one definition holds for all of them, in
 * every header of the library:
 *   - utterance i of a ragged batch computes what it computes when run ALONE at lens[i] rows (frames, keys, samples, phonemes) -- every
 *     value, and in the training pass every gradient.  Whatever the operands hold at or beyond a length, NaN included, reaches nothing
 *     before it.  What an entry writes at or beyond a length is stated with the entry.
 *   - lengths are int32 [B] in DEVICE memory and are read by the kernels alone, never on the host: a launch captured into a HIP graph
 *     follows values rewritten between replays.
 *   - a length outside its range is clamped into it by the kernel (the host cannot check it without a read); the range is [1, size]
 *     unless the entry names another.  Every entry checks its other arguments before any device call (NS2_ERR_ARG).
 * The computed extent.  Correctness needs the lengths in the kernels that mix rows alone; the skipping entries (ns2_linear_lens,
 * ns2_linear_lens_zero, ns2_wavenet_block_lens, ns2_attention_fwd_skip, ns2_model_forward_lens_skip, ns2_wgrad_rows_lens) hand them to
 * every product.  For a batch [B, N] with N % 256 == 0 the COMPUTED EXTENT of utterance i is
 *
 *     H_i = min(N, 256 * ceil(lens_i / 256))
 *
 * and row r of utterance i is HIDDEN when r >= H_i.  One granule of 256 rows for every kernel, whatever its own tile height (128 and
 * 256 rows in the GEMM family, 128 and 256 query rows in the attention kernels): producers and consumers agree on which rows exist.
 * A workgroup whose whole row tile is hidden returns before its first load; rows in [lens_i, H_i) share a tile with real frames and
 * are computed exactly as without skipping.  No bit of a row before H_i changes: the convolutions are causal, the self-attention
 * stops at the key counts, everything else is row-local, so a visible row never reads a hidden one.  The split-K route (batches of one
 * to four utterances) takes no lengths and computes every row.
 */
#ifndef NS2HIP_H
#define NS2HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS2_OK 0
#define NS2_ERR_ARG -1
#define NS2_ERR_HIP -2
#define NS2_ERR_STATE -3
#define NS2_UNAVAILABLE 1 /* not an error: this fast path does not apply here, take the general one (ns2_lstm2) */

const char* ns2_last_error(void);
int ns2_version(void);
/* test hook: force the GEMM kernel variant (0 = dispatch by shape, 1 = 128x128 register-staged, 2 = 256x256 LDS-DMA,
 * 3 = dispatch by shape but never split K, 4 = dispatch by shape but never the dedicated kernels (ffconv_kernel.h, gemm3_kernel.h,
 * wavenet3_kernel.h), 5 = dispatch by shape but never split K, and those kernels whenever a call is eligible, whatever its size).
 * 1 and 2 never split K either. */
int ns2_debug_force_gemm(int kernel);
/* test hook: the self-attention forward's kernel choice (0 = by eligibility, 1 = attn_kernel for every call, never the two-block
 * kernel of attn_fast_kernel.h: its reference and A/B partner).  Process-wide like the hook above; NS2_ATTN in the environment sets
 * the initial value.  Not to be flipped while a graph is being captured. */
int ns2_debug_force_attention(int kernel);
/* test hook: how many utterance chains ns2_model_forward / ns2_model_forward_row run the row-dependent part of a step as (0 = the
 * library's default, 1 = one chain: the whole batch on the caller's stream, 2 = two chains of ceil(B / 2) and floor(B / 2) utterances on
 * the caller's stream and a stream the model owns, wherever the chain rule allows: every product keeps the kernel it takes for the whole
 * batch, none splits K, each chain is whole 256-row tiles; never while the caller's stream is capturing or a debug tap is registered).
 * Results are bit-identical either way.  Process-wide like the hooks above; NS2_CHAINS in the environment sets the initial value. */
int ns2_debug_force_chains(int chains);
/* test hook: the number of chains (1 or 2) the last forward of this process ran; 0 before the first */
int ns2_debug_chains_last(void);
/* test hook: how many attention launches of this process took the two-block kernel so far (every other one took attn_kernel).
 * A test reads it before and after a call to see which kernel the call was routed to. */
int64_t ns2_debug_attention_fast_launches(void);
/* Split-K of small products.  ns2_model_forward* lend a region of their workspace to every GEMM of the pass: a product with too
 * few output tiles to fill the chip runs as K slices into fixed slots plus a second launch that adds the slots in order and
 * applies the epilogue (deterministic).  The stand-alone GEMM entry points below have no workspace argument and never split --
 * unless a test lends scratch to the calling host thread here: `scratch` = device memory of at least
 * ns2_splitk_scratch_bytes() bytes, used by every following stand-alone GEMM call of this thread until cleared with
 * (NULL, 0).  Test hook: the caller keeps the memory alive and the calls stream-ordered. */
int64_t ns2_splitk_scratch_bytes(void);
/* host arithmetic only (no device needed): the plan a product of M x N over k_tiles K tiles of 32 (k_tiles_per_tap per conv tap)
 * gets when scratch is lent -- `slices` (1 = not split) of `k_tiles_per_slice` K tiles of every tap */
int ns2_debug_splitk_plan(int M, int N, int k_tiles, int k_tiles_per_tap, int fp32_epilogue, int* slices, int* k_tiles_per_slice);
int ns2_debug_lend_splitk_scratch(void* scratch, int64_t bytes);

/* ------------------------------------------------------------------ packed weights (library-owned) */
typedef struct ns2_weight ns2_weight;
/* nn.Linear weight [rows, cols] (taps = 1) or Conv1d weight [rows, cols, taps] (NS2:583-595) -> K-contiguous bf16
 * split planes (precision 1 or 3: interleaved layout, usable at both; precision 2: dense IEEE-half rows; 4: the mixed-mode
 * lines; the latter two serve only their own precision), rows padded to 256, each tap's columns padded to 32.  geglu != 0 packs the rows of
 * FeedForward's first Linear (NS2:1021) so that GEGLU (NS2:1004-1007) fuses into the GEMM epilogue.
 * extra1x1 (may be null): a [rows, cols, 1] weight appended as one more, unshifted tap (WavenetResBlock.res_conv). */
int ns2_weight_pack(const float* w, int rows, int cols, int taps, int geglu, const float* extra1x1, int precision,
                    ns2_weight** out, void* stream);
void ns2_weight_free(ns2_weight* w);

/* ------------------------------------------------------------------ op-level entry points */
/* fp32 [M, d] (+ optional per-utterance addend) -> split planes [M, ldo] (zero padded) */
int ns2_split_f32(const float* x, int ldx, int M, int d, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                  void* stream);

/* split planes -> fp32 (hi + lo); lo may be null (dense hi-only layout) */
int ns2_join_f32(const uint16_t* hi, const uint16_t* lo, int ld, float* out, int ldo, int64_t M, int d, int precision,
                 void* stream);

/* nn.Linear / Conv1d as one GEMM (NS2:1051-1069, 1021-1024, 583-595): out = act(A W^T + bias) (+ resid).  ONE argument block describes
 * the call; a zero-initialised block plus `w`, the operand planes, `M`, `precision` and one output is the plain Linear, and every other
 * field switches one feature on:
 *   w, a, M    the packed weight; the activation planes [M, lda] in the operand format of `precision` (1 .. 4, see the conventions
 *              above), lda >= the weight's columns padded to 32.
 *   conv_taps  0 for a Linear, k for a Conv1d(kernel k) with `dilation`; seq_len = tokens per utterance (rows are never read across
 *              utterances); pad_left = zero frames in front of the sequence: -1 = causal (k - 1, CausalConv1d NS2:583-595), (k - 1) / 2 =
 *              the "same" padding of SpeechPromptEncoder's convs (NS2:316).  A zeroed block says 0, not causal: conv callers always set it.
 *   bias, act  bias [rows] (NULL = none); act after the bias: 0 none, 1 SiLU, 2 ELU.
 *   output     exactly one of  out_f32 [M, ldo_f] fp32, with the optional addend resid [M, ldr];
 *                              out_hi / out_lo [M, ldo] planes (ldo even), in the operand format of out_precision (0 = as `precision`;
 *              e.g. 3: bf16 hi / lo lines from a precision-4 product -- the q | k | v projection of the mixed training arithmetic, whose
 *              attention stays bf16 x3; out_lo NULL for dense IEEE half, hi + 32 for interleaved lines).
 *   vt_hi      non-NULL selects the fused q / k / v projection (NS2:1051-1053, 1063): columns < split_col -> the planes out [M, ldo],
 *              columns >= split_col (the values) -> transposed planes vt[b][col - split_col][n] with row stride vt_ld >= seq_len (for
 *              ns2_attention_fwd; both in the attention operands' format).  Needs seq_len; excludes bias, act, conv_taps, out_precision.
 *   GEGLU      selected by the weight having been packed with geglu = 1: FeedForward's first half GEGLU(Linear(x)) (NS2:1004-1007, 1021).
 *              bias is then the packed bias of ns2_geglu_pack_bias and required; out planes [M, ldo] with ldo = round_up(f, 32); excludes
 *              conv_taps, act, out_f32, vt_hi, out_precision.
 * Destinations (tests/test_gemm_dest_gpu.py pins every line):
 *   alignment  none beyond the element's own: any out_f32 / resid address, any ldo_f / ldr >= N; planes: ldo even (interleaved lines:
 *              a multiple of 32) and out_lo == out_hi + 32; vt_ld a multiple of 8 (interleaved V^T lines: of 32).  A 16-byte aligned
 *              base with ldo_f % 4 == 0 (resid, ldr the same) / ldo % 32 == 0 only selects the faster stores: the bits are the same.
 *   written    rows < M; fp32: columns < N; planes: columns < ldo, zero bits from N on -- so ldo <= round_up(N, 128), no kernel's column
 *              tiles reach further and a larger ldo is refused (ns2_wavenet_block: the same); q | k | v: columns < split_col of out
 *              (ldo >= split_col, a smaller one is refused: rows would overlap) and keys < seq_len of every vt row.
 *   never      fp32 columns >= N (up to ldo_f), rows >= M, q | k columns >= split_col, V^T keys >= seq_len (up to vt_ld), resid.
 * Every refusal is an NS2_ERR_ARG whose message starts "ns2_linear:" and names the field, made before any device call. */
typedef struct {
  const ns2_weight* w;
  const uint16_t* a_hi; const uint16_t* a_lo; int lda;
  int M, precision;
  int conv_taps, dilation, seq_len, pad_left;
  const float* bias; int act;
  float* out_f32; int ldo_f; const float* resid; int ldr;
  uint16_t* out_hi; uint16_t* out_lo; int ldo, out_precision;
  int split_col; uint16_t* vt_hi; uint16_t* vt_lo; int vt_ld;
} ns2_linear_args;
int ns2_linear(const ns2_linear_args* args, void* stream);
/* ns2_linear on a ragged batch of args->M / seq_len utterances of seq_len rows each: row tiles at or behind an utterance's computed
 * extent are skipped.  What a hidden tile leaves behind in sampling: an fp32 output WITHOUT a residual gets exact zeros (the residual
 * stream's first write and to_pred's output are read row by row by code that does not skip); every other output -- operand planes,
 * V^T, an fp32 output that accumulates into a residual -- keeps what it held.  Refused (NS2_ERR_ARG, before any device
 * call) when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0, or when args->seq_len is set and differs.
 * Whatever ns2_linear refuses is refused alike.  A product that splits K (ns2_debug_force_gemm 0 / 4 on a small batch) computes
 * every row. */
int ns2_linear_lens(const ns2_linear_args* args, const int* row_lens, int seq_len, void* stream);
/* ns2_linear_lens for the TRAINING pass, where what a hidden tile leaves behind differs for two reasons: the buffers of the pass come
 * uninitialised, and the dgrad of a causal conv is ANTICAUSAL -- the visible row H_i - 1 reads the rows behind it.
 * So A SKIPPING PRODUCT IN TRAINING WRITES ZERO BITS INTO THE HIDDEN TILES OF EVERY OUTPUT IT HAS: an fp32 output with or without a
 * residual, operand planes of either format, the attention's q | k | v lines, V^T.  Nothing in the pass then holds garbage, the
 * kernels that do not skip stay correct unchanged, and every reduction over tokens adds exact zeros where it added exact zeros
 * before (DESIGN section 9 walks the pass).
 * Rows before an utterance's computed extent have the bits ns2_linear gives.  Refused as ns2_linear_lens refuses: NS2_ERR_ARG,
 * before any device call, when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0, or when args->seq_len is set
 * and differs; whatever ns2_linear refuses is refused alike.  Every route ns2_linear can take a product down skips (the 128 x 128
 * kernel, the 256 x 256 kernel, the FF conv kernel, the lean linear kernel) except split K, which takes no lengths and computes
 * every row, as in ns2_linear_lens.
 * CONTRACT of an anticausal product (conv_taps > 1 with pad_left in [0, conv_taps - 1): the dgrad of a causal conv): a visible row
 * reads up to (conv_taps - 1 - pad_left) * dilation rows behind it, so the hidden rows of its operand must be ZEROS (what the
 * skipping products of the pass leave there, and what a cotangent holds behind a length).  A causal or plain product reads no hidden
 * row from a visible one: its operand's hidden rows may hold anything. */
int ns2_linear_lens_zero(const ns2_linear_args* args, const int* row_lens, int seq_len, void* stream);
/* Test hook: launches ns2_linear_lens_zero and ns2_wgrad_rows_lens (ns2hip_train.h) have sent WITH lengths so far in this process
 * (a product that ns2_linear_lens_zero routed to split K computed every row and is not counted).  Host arithmetic, no device-side counting: kernels with and without lengths may
 * give the same bits, so the tests read the counter around a pass. */
int64_t ns2_debug_train_skip_launches(void);
int ns2_geglu_pack_bias(const float* bias, int f, float* packed, int packed_len, void* stream);
/* The feed-forward causal conv (CausalConv1d(f, f, 3), NS2:1016 / 583-595) as one IEEE-half product has a kernel of its own
 * (csrc/ffconv_kernel.h).  It reads the weight as pre-tiled LDS images: ns2_weight_tile_conv3 builds them for a weight packed with
 * taps = 3 at precision 2 (one-time set-up, allocates once; ns2_weight_update keeps them current; after ns2_weights_repack call
 * ns2_weights_retile).  A later ns2_linear call with that weight and plane output takes the kernel when: conv_taps = 3,
 * dilation = 1, pad_left = -1, act = 0, M % 256 == 0, seq_len % 256 == 0, lda == ns2_conv3_input_ld(cols) (dense half rows padded to
 * a multiple of 128 columns; the padding is never multiplied), output dense half or FMT_H8 lines.  Results are bit-identical to the
 * general kernel's (same products, same summation order).  ns2_model_finalize does all of this for precisions 2 / 5 / 6. */
int ns2_weight_tile_conv3(ns2_weight* w, void* stream);
int ns2_conv3_input_ld(int cols);
/* The mixed linear products (precision 4, FMT_H8 operands) on full 256-row tiles have a lean kernel too (csrc/gemm3_kernel.h): same
 * arithmetic and summation order as the general kernel (bit-identical results), weights read as pre-tiled LDS images.
 * ns2_weight_tile_linear builds them for a weight packed with taps = 1 at precision 4 (also with geglu = 1); ns2_linear then takes the
 * kernel, whatever the output, when M % 256 == 0 and K >= 96.  Same life-cycle rules as ns2_weight_tile_conv3. */
int ns2_weight_tile_linear(ns2_weight* w, void* stream);
/* ... and so has the WavenetResBlock of the hybrid plan (csrc/wavenet3_kernel.h; NS2:597-642): ns2_weight_tile_wavenet builds the tiled
 * images of a weight packed with taps = 3 and extra1x1 at precision 4 (square, channels % 256 == 0); ns2_wavenet_block at precision 5
 * then takes the lean kernel when M % 256 == 0, seq_len % 256 == 0 and dilation <= 128.  Bit-identical to the general kernel. */
int ns2_weight_tile_wavenet(ns2_weight* w, void* stream);
/* WavenetResBlock (NS2:597-642) in one launch: out = tanh(g)*sigmoid(g) + res_conv(x), g = conv_dil(x)*gamma_t+beta_t.
 * w packed with taps=3 and extra1x1 = res_conv.weight; film[b] = [gamma(dim) | beta(dim)] = to_time_cond(t).
 * precision 5 (this entry point only): precision-4 operands and weight; the dilated conv multiplies their IEEE-half parts as
 * one product, res_conv keeps the fp8 correction terms (what model precision 5 runs; outputs wider than 128 columns) */
int ns2_wavenet_block(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                      int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                      uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
/* ns2_wavenet_block on a ragged batch (M / seq_len utterances): the same refusals as ns2_linear_lens on row_lens, seq_len and M.
 * Hidden row tiles of out_hi / out_lo keep what they held. */
int ns2_wavenet_block_lens(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                           int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                           uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, const int* row_lens, void* stream);
/* test hook: products that ns2_linear / ns2_wavenet_block / the model's steps have sent down a route so far, route = 0 split-K,
 * 1 the 128 x 128 kernel, 2 the 256 x 256 kernel, 3 the FF conv kernel, 4 the lean linear kernel, 5 the lean Wavenet kernel (-1 for any
 * other value): kernels of different routes may give the same bits, so the routing tests read the counter around a call. */
int64_t ns2_debug_gemm_route_launches(int route);

/* Attend.forward (ATT:77-155), non-causal: o = softmax(q k^T * scale) v.  ONE argument block describes the call; a zero-initialised
 * block plus the planes, the sizes, `scale` and `precision` is the plain forward, and every other field switches one feature on:
 *   q / k      row-major planes [B * Nq, ldq] / [B * Nk, ldk]; head h at columns col0 + h * head_dim.
 *   vt         transposed value planes [B][H * head_dim][vt_ld] (what ns2_linear writes with vt_hi set); o [B * Nq, ldo], head h at h * head_dim.
 *   head_dim   32, 64 or 128 (0 = 64): the reference's `dim_head` keyword (NS2:814-831 -> Attention ATT:77-155); scale is the
 *              caller's (dim_head ** -0.5).
 *   precision  1..4, the format of the operand planes (see the conventions above).  o_precision: the format of the output planes
 *              when it is not the operands' (4 = FMT_H8 lines for a precision-4 out-projection behind a bf16 x3 attention, 3 = bf16
 *              hi / lo lines; 0 = as `precision`).
 *   key_mask   [B, Nk] bytes, 1 = attend (ATT:92-94, 136-138; plain `Transformer` NS2:1073-1115; NULL = none).  Masked keys have P = 0
 *              (and dK = dV = 0 in the backward).  Every utterance must keep at least one key (the caller checks: the reference
 *              produces NaN there).
 *   lse        [B, H, Nq] (NULL = not wanted) = log2 of the softmax denominator of the scaled scores (m + log2 l): what the backward
 *              recomputes P from.  Training runs in the exact arithmetic at the backward's head dimension: precision 3, head_dim 64.
 *   dropout_p  in [0, 1), on the softmax output (ATT:100-101, 146): O = sum_k P_k keep_k / (1 - p) v_k, lse unchanged (and required).
 *              keep is a stateless function of (seed, call, b, h, q, k) -- csrc/dropout_keep.h, DESIGN.md §9 -- so forward and backward
 *              agree without storing it.  dropout_seed = two 32-bit words in DEVICE memory, read by the kernels (a captured graph sees
 *              the words of each replay); dropout_call = index of the attention inside the pass.  The backward takes the values its
 *              forward got.  dropout_p == 0: no dropout, the seed is not read (may be NULL) and the kernels without dropout run.
 * With key_mask == NULL and dropout_p == 0 the unmasked kernels run. */
typedef struct {
  const uint16_t* q_hi; const uint16_t* q_lo; int ldq, q_col0;
  const uint16_t* k_hi; const uint16_t* k_lo; int ldk, k_col0;
  const uint16_t* vt_hi; const uint16_t* vt_lo; int vt_ld;
  uint16_t* o_hi; uint16_t* o_lo; int ldo;
  int B, H, Nq, Nk; float scale;
  int head_dim, precision, o_precision;
  const uint8_t* key_mask;
  float* lse;
  float dropout_p; const uint32_t* dropout_seed; unsigned dropout_call;
} ns2_attn_args;
int ns2_attention_fwd(const ns2_attn_args* args, void* stream);
/* ns2_attention_fwd with per-utterance key counts: utterance b attends to keys [0, key_lens[b]).  args->Nk stays the stride of k and
 * of the V^T rows; a count is clamped into [1, Nk] (no read out of bounds, no empty softmax).  Keys at or beyond an utterance's length
 * are treated as keys at or beyond Nk: score -inf, K rows and V^T columns read as zeros -- what lies there may be anything, NaN
 * included.  Query rows at or beyond the length are computed like any other row, attending to the keys before it: every output is
 * finite and defined.  Refused (NS2_ERR_ARG, before any device call) when args or key_lens is null or when args->key_mask, args->lse
 * or args->dropout_p is set: key counts belong to the plain inference forward.  Precisions 2 / 4 at head_dim 64 with Nq % 256 == 0
 * and Nk % 64 == 0 run attn_fast_kernel and skip whole key tiles beyond a length; every other shape runs attn_kernel. */
int ns2_attention_fwd_lens(const ns2_attn_args* args, const int* key_lens, void* stream);
/* ns2_attention_fwd_lens (key_lens != NULL) / ns2_attention_fwd (key_lens == NULL: the cross attention to the resampled prompt has
 * query lengths alone) with per-utterance frame counts on the query side: a query workgroup whose rows all lie at or behind
 * H_b = min(Nq, 256 ceil(query_lens[b] / 256)) returns before its first load, and its rows of o keep what they held.  Key handling
 * is unchanged.  Refused (NS2_ERR_ARG, before any device call) when args or query_lens is null, args->Nq % 256 != 0, or
 * args->key_mask, args->lse or args->dropout_p is set. */
int ns2_attention_fwd_skip(const ns2_attn_args* args, const int* key_lens, const int* query_lens, void* stream);

/* RMSNorm.forward (NS2:727-746).  gamma may be null; cond (may be null) holds [gamma_c | beta_c] per batch row */
int ns2_rmsnorm(const float* x, int ldx, int M, int d, int seq_len, const float* gamma, const float* cond, int cond_ld,
                uint16_t* out_hi, uint16_t* out_lo, int ldo, float* out_f32, int ldo_f, int precision, void* stream);
/* test hook of ns2_rmsnorm and of every RMSNorm a model launches: 0 = by shape (the default): rmsnorm_wide_kernel for the hot case -- d a
 * multiple of 256 up to 1024, ldo == d, FMT_H8 / dense IEEE-half / interleaved bf16 planes, x, gamma, cond and the outputs 16-byte aligned,
 * cond_ld a multiple of 4, and (with cond) seq_len a multiple of 16 -- and rmsnorm_kernel for everything else; 1 = rmsnorm_kernel for every
 * call.  The two kernels give the same bits.  NS2_NORM in the environment sets the initial value.
 * ns2_debug_norm_last: the kernel the last RMSNorm launch of the process took: 1 = rmsnorm_kernel, 2 = rmsnorm_wide_kernel, 0 = none yet. */
int ns2_debug_force_norm(int kernel);
int ns2_debug_norm_last(void);

/* out[b, j] = act(in[b, :] . wt[:, j] + bias[j]); wt K-major [K, J]; act: 0 none, 1 SiLU (conditioning projections:
 * to_time_cond / to_gamma_beta / to_prompt_cond Linears on [batch, dim_cond] rows, NS2:623, 744, 841, 860).
 * workspace (may be null: slower single pass) = ns2_skinny_linear_workspace_bytes(B, K, J) bytes of caller-owned scratch
 * for the deterministic split-K partial sums */
int64_t ns2_skinny_linear_workspace_bytes(int B, int K, int J);
int ns2_skinny_linear(const float* in, int ld_in, const float* wt, const float* bias, float* out, int ld_out, int B, int K,
                      int J, int act, void* workspace, int64_t workspace_bytes, void* stream);
/* to_time_cond (NS2:108-120, 839-843); wt = Linear weight K-major [dim+1, dt]; feat_ws [B, dim+1] scratch;
 * workspace as for ns2_skinny_linear(B, dim + 1, dt) */
int ns2_time_embed(const float* times, const float* freqs, const float* wt, const float* bias, float* feat_ws, float* out,
                   int ld_out, int B, int dim, int dt, void* workspace, int64_t workspace_bytes, void* stream);
int ns2_transpose_f32(const float* in, int batch, int R, int C, float* out, void* stream);
/* nn.Embedding gather, ids < 0 -> pad_id (PhonemeEncoder NS2:281-284) */
int ns2_embedding(const int64_t* ids, const float* table, float* out, int64_t n, int dim, int64_t pad_id, void* stream);

/* ------------------------------------------------------------------ the two folds
 * FeedForward is Sequential(Linear(dim, 2f), GEGLU(), CausalConv1d(f, f, 3), Linear(f, dim)) (NS2:1009-1025).  Nothing stands between
 * the causal conv and the last Linear and both are linear maps, so the pair is one causal conv of kernel 3 from f to dim channels:
 *   w_fold[n, c, t] = sum_j w_out[n, j] w_conv[j, c, t]          b_fold[n] = sum_j w_out[n, j] b_conv[j] + b_out[n]
 * exactly, the zero frames in front of an utterance included (the padded input is the same).  A step then multiplies 2 M 3f dim
 * instead of 2 M f (3f + dim) per layer and the conv's output never exists.  ns2_model_finalize folds every layer once, from the fp32
 * parameters, and packs w_fold in the format of the conv site of the model's precision plan; ns2_model_forward* run the folded conv
 * (+ bias + residual) in that site's arithmetic.  Results are a reassociation of the same linear algebra, not the same bits.
 * The fold of one layer on the device: w_out [dim, f], w_conv [f, f, 3], b_conv [f], b_out [dim] or NULL -> w_fold [dim, f, 3]
 * (Conv1d's layout: ns2_weight_pack(w_fold, dim, f, 3, ..) packs it), b_fold [dim]; all fp32 device memory.  fp32 FMAs over ascending
 * j, one accumulator per output, no atomics: bit-identical from run to run.
 * ns2_linear with such a weight packed at precision 2 and tiled by ns2_weight_tile_conv3 takes the dedicated conv kernel
 * (csrc/ffconv_kernel.h) for an fp32 output as well -- out_f32 and resid 16-byte aligned, ldo_f and ldr multiples of 4, and the
 * conditions ns2_weight_tile_conv3 lists for the plane output -- bit-identical to the general kernel. */
int ns2_ff_fold(const float* w_out, const float* w_conv, const float* b_conv, const float* b_out, int dim, int f, float* w_fold,
                float* b_fold, void* stream);
/* test hook: 1 = fold (the default), 0 = the conv and FF-out stay two products -- bit for bit what the library computed before it
 * folded.  Read by ns2_model_finalize (a model keeps what it was finalized with) and by ns2_debug_chain_rule; process-wide like
 * ns2_debug_force_gemm; NS2_FOLD in the environment sets the initial value. */
int ns2_debug_force_fold(int fold);
/* Wavenet ends in `final_conv(sum of the blocks' skip convs)` (NS2:639-640, 685-686, 725): a Conv1d(dim, dim, 1) directly behind a sum of
 * L Conv1d(dim, dim, 1), i.e. a Linear behind a Linear over the L concatenated block outputs.  The pair is one Linear of K = L * dim:
 *   w_fold[n, l * dim + c] = sum_j w_final[n, j] w_skip[l][j, c]        b_fold[n] = sum_j w_final[n, j] (sum_l b_skip[l][j]) + b_final[n]
 * ns2_model_finalize folds once, from the fp32 parameters, and packs w_fold in the model's plan format; ns2_model_forward* then run ONE
 * product from the last stack's planes into the residual stream (like every other update of it: the RMSNorm that follows runs behind it,
 * or inside it where the product splits K), and neither the packed skip / final weights nor the skip sum's planes exist.  Results are a
 * reassociation of the same linear algebra, not the same bits.  The training pass keeps its two products.
 * Profiling (ns2_model_profile_begin): the folded product writes fp32 (gemm<f32 epilogue>) but is timed under category bit 1, where the skip
 * sum was: bench.py credits that category with the skip sum's 2 M dim L dim FLOPs, which are the FLOPs this product multiplies.  With the
 * fold on, category 1 therefore holds one fp32-epilogue launch per step beside the Wavenet's init conv.
 * The fold on the device: w_final [dim, dim], w_skip [layers, dim, dim], b_skip [layers, dim], b_final [dim] or NULL ->
 * w_fold [dim, layers * dim] (ns2_weight_pack(w_fold, dim, layers * dim, 1, ..) packs it), b_fold [dim]; all fp32 device memory.  fp32 FMAs
 * over ascending j (the bias sum over ascending l first), one accumulator per output, no atomics: bit-identical from run to run. */
int ns2_tail_fold(const float* w_final, const float* w_skip, const float* b_skip, const float* b_final, int dim, int layers, float* w_fold,
                  float* b_fold, void* stream);
/* test hook: 1 = fold (the default), 0 = the skip sum and final_conv stay two products -- bit for bit what the library computed before it
 * folded.  Read by ns2_model_finalize (a model keeps what it was finalized with) and by ns2_debug_chain_rule / ns2_debug_skip_rule;
 * process-wide like ns2_debug_force_gemm; NS2_TAIL_FOLD in the environment sets the initial value. */
int ns2_debug_force_tail_fold(int fold);

/* one DDIM update (NS2:1396-1430): audio <- f(audio, model_out, times, times_next).  objective 0 'v', 1 'eps', 2 'x0';
 * schedule 0 sigmoid, 1 cosine, 2 linear (NS2:1133-1148) */
int ns2_ddim_step(const float* audio, const float* model_out, float* out, const float* times, const float* times_next,
                  int B, int64_t per_batch, int objective, int schedule, float scale, void* stream);
/* classifier-free guidance mix (NS2:927) */
int ns2_cfg_mix(const float* cond_out, const float* null_out, float* out, int64_t n, float cond_scale, void* stream);

/* Range guard of precisions 2 and 4 (IEEE-half operands stop at 65504 / 57344; beyond, values are clamped: finite but
 * wrong).  Counts, on the CURRENT device, the conversions that met an out-of-range (or NaN) value since the last reset.
 * Synchronises the device: call it between sampling runs, not per step.  A non-zero count means the model needs
 * precision 3 (bf16 planes: fp32 exponent range). */
int ns2_saturation_count(int reset, int64_t* count);
/* The counters behind that total.  Every source file of the library whose kernels convert to the IEEE-half formats owns one and
 * registers it when the library is loaded: ns2_saturation_counters is how many there are (no GPU needed; -1 if the library was built
 * with more than its registry holds, and the other entry points then fail), ns2_saturation_counter_name(i) the source file of
 * counter i (NULL outside 0 <= i < count). */
int ns2_saturation_counters(void);
const char* ns2_saturation_counter_name(int i);
/* The same counters without a synchronisation: enqueues, on `stream`, one copy per registered counter (cumulative since the last
 * reset) into host[0..n), n = ns2_saturation_counters() -- host memory that stays valid until the stream reaches this point (pinned
 * memory for a truly asynchronous copy).  capacity < n is an argument error and nothing is written.  The order of the words is
 * unspecified: sum them, or compare them with an earlier peek.  The caller records an event behind it and reads the values once
 * the event has completed; the host-side `Model` does so every few forwards, so that calls from ANY wrapper (this package's sampler,
 * the reference's own NaturalSpeech2 / Trainer around compat.HipBackedModel, a bare Model.forward) notice clamped activations, and
 * a training loop under the mixed arithmetic compares a peek before the pass with one after it (an overflowed step). */
int ns2_saturation_peek(unsigned int* host, int capacity, void* stream);

/* ------------------------------------------------------------------ Model (NS2:811-1000) */
typedef struct ns2_model ns2_model;
typedef struct {
  int dim, depth, dim_head, heads, ff_mult, wavenet_layers, wavenet_stacks, dim_cond_mult;   /* NS2:814-823; dim_head 32, 64 or 128 */
  int condition_on_prompt, dim_prompt, num_latents_m, resampler_depth;                       /* NS2:826-831 */
  int precision;               /* 3 = bf16 x3 split "exact", 4 = fp16 + fp8 correction terms "mixed", 2 = fp16 single product
                                  "half", 1 = bf16 single product "fast"; 5 = "hybrid": the per-site plan of this model
                                  only: precision 4 everywhere except the feed-forward causal conv (NS2:1016) and the dilated
                                  convs of the Wavenet blocks (NS2:612), which run as one fp16 product on the same operands.
                                  6 = "hybrid_ff": 5, with the rest of the feed-forward branch (FF-in + GEGLU, NS2:1021, and
                                  FF-out, NS2:1024) as one fp16 product on dense half planes too.
                                  At precisions 2 / 4 / 5 / 6 the step-invariant pass (ns2_model_prepare_cond) computes in
                                  precision 3: its few rows condition every frame of every step */
} ns2_model_config;

int ns2_model_create(const ns2_model_config* cfg, ns2_model** out);
/* register one state_dict entry (reference key names); data = device fp32, contiguous */
int ns2_model_set_param(ns2_model* m, const char* name, const float* data, int ndim, const int64_t* dims);
/* pack all weights (one-time, synchronises); the registered parameter tensors must stay alive afterwards only for
 * the small fp32 vectors the executor reads in place (biases, gammas, sinusoid freqs) */
int ns2_model_finalize(ns2_model* m, void* stream);
int64_t ns2_model_workspace_bytes(const ns2_model* m, int B, int N, int n_prompt, int n_cond);
int64_t ns2_model_cond_bytes(const ns2_model* m, int B, int N, int n_prompt, int n_cond);
/* step-invariant conditioning (NS2:944-992: to_prompt_cond, perceiver_resampler, cond_to_model_dim, null substitutes)
 * -> `cond_state` (caller-owned, ns2_model_cond_bytes).  drop != 0 == cond_drop_prob 1 (the CFG null branch). */
int ns2_model_prepare_cond(ns2_model* m, const float* prompt, int n_prompt, const float* cond, int n_cond, int drop, int B,
                           int N, void* cond_state, void* workspace, int64_t workspace_bytes, void* stream);
/* ns2_model_prepare_cond with a prompt row count per utterance: to_prompt_cond takes the mean over rows [0, prompt_lens[b]), and the
 * perceiver resampler attends to keys [0, Lm + prompt_lens[b]) of cat(latents, prompt) (ns2_attention_fwd_lens's path; the key counts
 * are made on the device).  Prompt rows at or beyond a length may hold NaN.  The drop branch (null substitutes) ignores the lengths.
 * prompt_lens == NULL: the launches of ns2_model_prepare_cond.  Same workspace and cond_state sizes. */
int ns2_model_prepare_cond_lens(ns2_model* m, const float* prompt, int n_prompt, const int* prompt_lens, const float* cond, int n_cond,
                                int drop, int B, int N, void* cond_state, void* workspace, int64_t workspace_bytes, void* stream);
/* Classifier-free guidance as ONE batch (NS2:914-927: cond and null forward of the same x): state_out (ns2_model_cond_bytes for 2 B
 * utterances) = the arrays of state_a (B utterances, e.g. drop = 0) followed by those of state_b (drop = 1).  ns2_model_forward with
 * batch 2 B, x and times repeated, then ns2_cfg_mix of the two halves.  Stream-ordered device copies, no allocation. */
int ns2_model_cond_stack(ns2_model* m, const void* state_a, const void* state_b, int B, int N, int n_cond, void* state_out, void* stream);
/* Model.forward (NS2:929-1000) for x [B, N, dim], times [B] -> out [B, N, dim]; cond_state null iff unconditional;
 * n_cond = the n_cond the cond_state was prepared with */
int ns2_model_forward(ns2_model* m, const float* x, const float* times, const void* cond_state, int n_cond, float* out, int B,
                      int N, void* workspace, int64_t workspace_bytes, void* stream);
/* Step-invariant TIME conditioning.  A sampler knows its times up front and they are shared by the batch
 * (get_sampling_timesteps, NS2:1303-1308), so every time-conditioning projection of the run (to_time_cond NS2:839-843 + the FiLM /
 * adaptive-norm Linears NS2:623, 744) is ONE table: ns2_model_time_table fills table[T, ns2_model_table_cols(m)] for times[T]
 * (device), and ns2_model_forward_row runs Model.forward for the step whose conditioning is `cond_row` = table + i * cols -- no
 * projection is launched inside the step.  Rows are computed with the K split of a batch of plan_B rows (pass the run's batch size):
 * for an unconditional model the step is then BIT-IDENTICAL to ns2_model_forward(times = t_i for every utterance); a conditioned
 * model adds the per-utterance prompt half kept in its cond_state (sum order differs: equal to fp32 rounding). */
int ns2_model_table_cols(const ns2_model* m);
int64_t ns2_model_time_table_workspace_bytes(const ns2_model* m, int plan_B);
int ns2_model_time_table(ns2_model* m, const float* times, int T, int plan_B, float* table, void* workspace, int64_t workspace_bytes,
                         void* stream);
int ns2_model_forward_row(ns2_model* m, const float* x, const float* cond_row, const void* cond_state, int n_cond, float* out, int B, int N,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* ns2_model_forward (times != NULL) / ns2_model_forward_row (cond_row != NULL) with per-utterance frame counts: exactly one of
 * times / cond_row.  In Model the self-attention is the one thing through which a frame sees later frames (the convolutions are
 * causal; norms, FiLM and the cross-attention to the resampled prompt work per frame), so the lengths go to the self-attention kernels
 * (ns2_attention_fwd_lens's path) and to nothing else.  frame_lens == NULL: the same launches as those two entries. */
int ns2_model_forward_lens(ns2_model* m, const float* x, const float* times, const float* cond_row, const int* frame_lens,
                           const void* cond_state, int n_cond, float* out, int B, int N, void* workspace, int64_t workspace_bytes,
                           void* stream);
/* ns2_model_forward_lens with skipping.  frame_lens == NULL is an argument error (ns2_model_forward_lens is the call that allows it).
 * The skipping step runs when the SKIP RULE holds: N % 256 == 0 and no product of the described step is planned on the split-K
 * route; otherwise exactly the launches of ns2_model_forward_lens are issued.  In a skipping step every product and both attention
 * kernels skip hidden row tiles; rows of out at or behind H_i are exact zeros, rows before it have the bits ns2_model_forward_lens
 * gives.  Two utterance chains and a captured step work as there. */
int ns2_model_forward_lens_skip(ns2_model* m, const float* x, const float* times, const float* cond_row, const int* frame_lens,
                                const void* cond_state, int n_cond, float* out, int B, int N, void* workspace, int64_t workspace_bytes,
                                void* stream);
/* Sampled content checksum of every registered parameter (sum and absolute sum of ~2048 evenly spaced elements each), stream-ordered
 * and NON-synchronising: 2 * ns2_model_param_count(m) floats land in host_out (pinned memory) once the stream passes this point.
 * The parameters are read where ns2_model_set_param found them, so a caller that compares two checksums notices parameters
 * rewritten through `.data` (ema_pytorch, NS2:1793-1801) without a device synchronisation -- the host-side Model does, every few forwards. */
int ns2_model_param_count(const ns2_model* m);
int ns2_model_param_checksum(ns2_model* m, float* host_out, int capacity, void* stream);
/* optional intermediate taps for parity tests (fp32 copies made during forward / prepare_cond): "t", "c",
 * "wavenet.init", "wavenet.stack<s>", "wavenet.out", "layer<i>.attn", "layer<i>"; dst = null unregisters */
int ns2_model_debug_tap(ns2_model* m, const char* name, float* dst, int64_t dst_elems);
/* live kernel timing with HIP events on the caller's stream (bench.py roofline): category bits
 * 0 gemm<f32 epilogue> 1 gemm<split epilogue> 2 gemm<qkv> 3 gemm<geglu> 4 gemm<wavenet> 5 attention 6 rmsnorm.
 * _end synchronises on the recorded events and returns the summed kernel time and the number of launches.  A step that ran as two
 * utterance chains (ns2_debug_force_chains) records each product's two parts on their own streams: `launches` counts the product once and
 * `total_ms` adds both parts -- each measured while the other chain's kernels share the chip, so it overstates the product's cost alone. */
int ns2_model_profile_begin(ns2_model* m, unsigned category_mask);
int ns2_model_profile_end(ns2_model* m, double* total_ms, int64_t* launches);
/* test hook, host arithmetic only (no device): the number of chains a forward of B utterances x N frames of a model of this
 * configuration runs where two are wanted (the chain rule alone: not the capture / tap / force conditions) */
int ns2_debug_chain_rule(const ns2_model_config* cfg, int B, int N, int* chains);
/* test hooks.  ns2_debug_skip_rule: the skip rule for a configuration, without a device (pure host arithmetic over the described
 * launches, like ns2_debug_chain_rule): *skips = 1 when a forward of B x N frames would run the skipping step.
 * ns2_debug_skip_last: 1 when the last forward of the process -- through any of the model's forward entries -- ran the skipping step,
 * else 0 (a plain ns2_model_forward resets it). */
int ns2_debug_skip_rule(const ns2_model_config* cfg, int B, int N, int* skips);
int ns2_debug_skip_last(void);
void ns2_model_destroy(ns2_model* m);

#ifdef __cplusplus
}
#endif
#endif /* NS2HIP_H */
