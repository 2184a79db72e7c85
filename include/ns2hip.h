/* libns2hip — C ABI of the MI355X-native NaturalSpeech2 denoising hot path.
 *
 * The reference (lucidrains/naturalspeech2-pytorch) has no FFI/plugin layer: its boundary for this path is the
 * Python class surface.  This header is the C-ABI a host binds instead; each entry point cites the
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

/* RMSNorm.forward (NS2:727-746).  gamma may be null; cond (may be null) holds [gamma_c | beta_c] per batch row */
int ns2_rmsnorm(const float* x, int ldx, int M, int d, int seq_len, const float* gamma, const float* cond, int cond_ld,
                uint16_t* out_hi, uint16_t* out_lo, int ldo, float* out_f32, int ldo_f, int precision, void* stream);

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

/* ------------------------------------------------------------------ DurationPitchPredictor and text-conditioned sampling
 * (NS2:344-527, 87-104, 164-175, 1449-1455, 1476-1483).  The trunk's convolutions are ns2_linear calls (conv_taps = k,
 * pad_left = k / 2), its RMSNorm and attention the entries above; these are the pieces around them.
 * ns2_groupnorm_silu: nn.GroupNorm(groups, C) + SiLU (Block, NS2:346-369) over token-major fp32 rows x [B * n, C], statistics
 * per (utterance, group) over n x C / groups values, eps as given; resid (may be null) [B * n, C] is added after the SiLU (the
 * second Block of a ResnetBlock, NS2:394-398).  Outputs: out_f32 [B * n, C] and / or operand planes (out_hi, out_lo, ldo = C)
 * in the format of `precision`.  C / groups must be a multiple of 4 (and C of 32 for planes); fp32 buffers 16-byte aligned.
 * workspace = ns2_groupnorm_workspace_bytes(B, n, C, groups) bytes of caller-owned scratch: per-chunk (count, mean, M2)
 * partials in fixed slots, combined in a fixed order -- the result is bit-reproducible. */
int64_t ns2_groupnorm_workspace_bytes(int B, int n, int C, int groups);
int ns2_groupnorm_silu(const float* x, int B, int n, int C, int groups, const float* weight, const float* bias, float eps,
                       const float* resid, float* out_f32, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* totals[b] = sum_i int(duration[b, i]) (generate_mask_from_repeats, NS2:87-92; negative durations count as 0 frames):
 * the caller reads max(totals) = n_frames for ns2_length_regulate */
int ns2_length_regulate_totals(const float* duration, int B, int n_ph, int* totals, void* stream);
/* the length regulator of NaturalSpeech2.sample (NS2:1478-1483): frame f < n_frames of utterance b takes the phoneme whose
 * [exclusive, inclusive) prefix of int(duration[b]) holds f (none past the utterance's total: zeros), and
 * out[b, :, f] = enc[b, ph, :] + pitch_table[f0_to_coarse(pitch[b, ph]), :]   (NS2:164-175, 1449-1455)
 * duration / pitch [B, n_ph], enc [B, n_ph, D], pitch_table [>= 256, D], out [B, D, n_frames]; mel_min / mel_max = the fp32
 * constants 1127 log(1 + f0_min / 700) / 1127 log(1 + f0_max / 700) of f0_to_coarse.  n_ph <= 8192. */
int ns2_length_regulate(const float* duration, const float* pitch, const float* enc, const float* pitch_table, int B, int n_ph,
                        int D, int n_frames, float mel_min, float mel_max, float* out, void* stream);
/* out[m] = act(x[m, :K] . w + bias[0]), act = ReLU when relu != 0 (to_pred: Linear(dim, 1) + ReLU, NS2:467-471); bias may be
 * null; K and ldx multiples of 4, x and w 16-byte aligned */
int ns2_row_dot(const float* x, int ldx, int M, int K, const float* w, const float* bias, int relu, float* out, void* stream);

/* ---- Aligner (aligner.py) and the text-conditioned training pass (NS2:1524-1602).  Lengths are int32 [B] on the device,
 * clamped to [0, size] as create_mask (utils.py:28-33) would; nothing here reads device data on the host. */
/* planes [M, ldo] <- ReLU(x [M, N]) in the operand format of `precision`, columns N .. ldo - 1 zero (AlignerNet's ReLUs between
 * its convolutions, aligner.py:30-51); N % 4 == 0, ldo % 32 == 0 */
int ns2_relu_split(const float* x, int M, int N, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
/* AlignerNet attention (aligner.py:72-90): queries [B * T, C], keys [B * n, C] fp32 token-major; aln_log [B, 1, T, n] =
 * the Euclidean distance summed in fp32 (no negation, no temperature), -FLT_MAX at phonemes >= text_lens[b]; aln_soft
 * [B, n, T] = softmax over phonemes, transposed (a fully masked row is uniform).  n <= 1024, C <= 256 */
int ns2_align_attn(const float* queries, const float* keys, const int* text_lens, int B, int T, int n, int C, float* aln_log,
                   float* aln_soft, void* stream);
/* maximum_path (aligner.py:97-130) of value [B, t_x, t_y] fp32 under the prefix masks text_lens x mel_lens: path [B, t_x, t_y]
 * 0/1 fp32, bit for bit the reference's (ties stay, direction 1 outside the mask, backtrack from row text_len - 1), and
 * durations [B, t_x] int32 = its row sums.  t_x <= 1024, t_y <= 8192; workspace = ns2_maximum_path_workspace_bytes bytes
 * (the per-column path rows, plus the direction bits when t_x_pad * t_y / 8 bytes exceed 128 KiB of LDS) */
int64_t ns2_maximum_path_workspace_bytes(int B, int t_x, int t_y);
int ns2_maximum_path(const float* value, const int* text_lens, const int* mel_lens, int B, int t_x, int t_y, float* path,
                     int* durations, void* workspace, int64_t workspace_bytes, void* stream);
/* average_over_durations (utils.py:4-26): pitch [B, T] (the reference's [B, 1, T]), durations [B, n] int32 -> out [B, n] = mean
 * of the non-zero frames of each phoneme from fp32 prefix sums, 0 where none.  T, n <= 8192 */
int ns2_average_over_durations(const float* pitch, const int* durations, int B, int T, int n, float* out, void* stream);
/* backward of expand_encodings with durations (NS2:1449-1455, the forward is ns2_length_regulate): d_cond [B, D, n_frames],
 * duration / pitch [B, n] fp32 -> d_enc [B, n, D] = sum of d_cond over each phoneme's frames, d_table [n_bins, D] (null: skip)
 * = sum over (b, i) in ascending order of the rows of d_enc whose f0_to_coarse(pitch) is the bin.  No atomics: bit-reproducible.
 * workspace = ns2_expand_backward_workspace_bytes(B, n) bytes */
int64_t ns2_expand_backward_workspace_bytes(int B, int n);
int ns2_expand_backward(const float* d_cond, const float* duration, const float* pitch, int B, int n, int D, int n_frames, int n_bins,
                        float mel_min, float mel_max, float* d_enc, float* d_table, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ---- AudioToMel (audio_to_mel.py, NS2:181-224): audio [B, L] fp32 -> out [B, n_mels, T], T = 1 + L / hop_length.  The frames
 * are those of torch.stft(center=True, pad_mode="reflect", onesided=True), power |X|^2, mel = fb^T power summed in ascending
 * bins, and with log_db 10 log10(max(mel, 1e-10)).  Tables (host-built, fp64 rounded to fp32): window [n_fft] (Hann zero-padded
 * centred), twiddle [n_fft] complex (cos, sin)(-2 pi k / n_fft); the filterbank compactly as fb_meta [3][n_mels] int32 = first
 * bin, number of bins, offset into fb_w [n_w], with first + number <= n_bins (the bins read) <= n_fft / 2 + 1.  n_fft a power of
 * two in [256, 2048], 1 <= hop_length <= n_fft, n_mels <= 256, L > n_fft / 2.  No atomics: bit-reproducible per utterance. */
int ns2_audio_to_mel(const float* audio, int B, int64_t L, int n_fft, int hop_length, const float* window, const float* twiddle,
                     const int* fb_meta, const float* fb_w, int n_w, int n_mels, int n_bins, int log_db, float* out, void* stream);

/* one DDIM update (NS2:1396-1430): audio <- f(audio, model_out, times, times_next).  objective 0 'v', 1 'eps', 2 'x0';
 * schedule 0 sigmoid, 1 cosine, 2 linear (NS2:1133-1148) */
int ns2_ddim_step(const float* audio, const float* model_out, float* out, const float* times, const float* times_next,
                  int B, int64_t per_batch, int objective, int schedule, float scale, void* stream);
/* classifier-free guidance mix (NS2:927) */
int ns2_cfg_mix(const float* cond_out, const float* null_out, float* out, int64_t n, float cond_scale, void* stream);

/* ------------------------------------------------------------------ EnCodec SEANet encoder / decoder pieces (HFENC:81-347)
 * The convolutions themselves are ns2_linear calls on channel-last rows (strided / transposed convolutions as 2-tap
 * convolutions over rows regrouped by the stride); these are the pieces around them.
 * ns2_seanet_prep: fp32 x [B, in_prefix + T, C] (row stride ldx, the first in_prefix rows of every utterance skipped;
 *   + optional add [B, T, C]) -> optional ELU (HFENC:285-347) -> operand
 *   planes [B, prefix + T, ldo] whose `prefix` leading rows per utterance hold the mirrored samples (row -j = row j): EnCodec's
 *   reflect padding of causal convolutions (HFENC:142-175).  im2col_k > 0 (C must be 1, prefix 0): output column j of row n is
 *   x_reflect[n - (k - 1) + j], the k taps of the first convolution as a K = k Linear.
 * ns2_seanet_unpad: dst[b][t][:] = src[b][prefix + t][:]  (drop the prefix rows of a convolution output)
 * ns2_lstm_layer: one nn.LSTM layer (HFENC:253-266; gate order i, f, g, o).  xproj [B*T, 4H] = x W_ih^T + b_ih (a GEMM, row
 *   b*T + t), w_hh [4H, H], b_hh [4H]; state = ns2_lstm_state_floats(B, H) floats of caller scratch (at least 3*B*H: with less
 *   than the full amount the recurrence runs as one launch per step instead of one persistent launch per layer);
 *   out[b*T + t, :H] = h_t (+ resid row). */
int ns2_seanet_prep(const float* x, int ldx, int in_prefix, const float* add, int ldadd, int B, int64_t T, int C, int elu, int prefix,
                    int im2col_k, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
/* ns2_seanet_prep2: one pass over fp32 x [B, in_prefix + T, C] for the two operands EnCodec's residual block (HFENC:268-301) needs
 *   of it -- ELU(x) and x -- each (either may be NULL) into the column window [col0, col0 + cols) of a plane buffer of row stride
 *   ld (logical columns; col0 a multiple of 32, cols >= C a multiple of 4, zero filled past C), rows laid out as ns2_seanet_prep
 *   does (`prefix` mirrored rows per utterance).  Lets x and the hidden activation share one operand, so that
 *   conv2(elu(h)) + shortcut(x) is ONE GEMM over the concatenated K. */
int ns2_seanet_prep2(const float* x, int ldx, int in_prefix, int B, int64_t T, int C, int prefix, uint16_t* elu_hi, uint16_t* elu_lo,
                     int elu_ld, int elu_col0, int elu_cols, uint16_t* raw_hi, uint16_t* raw_lo, int raw_ld, int raw_col0, int raw_cols,
                     int precision, void* stream);
/* ns2_seanet_conv_narrow: the two ends of the SEANet stacks as what they are -- the encoder's first convolution (ci = 1 -> co
 *   channels, HFENC:304-327) and the decoder's last (ci -> co = 1, HFENC:330-358): causal, reflect padded (HFENC:142-175), k = 7,
 *   fp32 on the vector ALUs in one pass over the wide side.  x fp32 [B, in_prefix + T, ci] (row stride ldx), optional ELU on the
 *   input, w [co, ci, k] as nn.Conv1d holds it, out fp32 [B * T, co] (row stride ldo).  Returns NS2_UNAVAILABLE (nothing launched)
 *   for any other shape: the caller takes the GEMM path. */
int ns2_seanet_conv_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int ci, int co, int k, int elu, const float* w,
                           const float* bias, float* out, int64_t ldo, void* stream);
/* ns2_seanet_resblock_narrow: EnCodec's residual block (HFENC:268-301) y = shortcut(x) + conv2(elu(conv1(elu(x)))) -- conv1 k = 3
 *   causal, dilation 1, reflect padded, C -> C / 2; conv2 and the shortcut 1 x 1 -- in ONE fp32 pass on the vector ALUs for the narrow
 *   end of the SEANet stacks (C = 32: the blocks that run at the full sample rate), instead of two operand-plane passes + two GEMMs.
 *   x fp32 [B, in_prefix + T, C] (row stride ldx) -> out fp32 [B * T, C] (row stride ldo).  Weights pre-arranged in consumption order:
 *   w1p [3][C][C / 2] = conv1.weight[h][c][t] at (t, c, h); w2p [C / 2][C] = conv2.weight[c][h] at (h, c); wsp [C][C] =
 *   shortcut.weight[o][c] at (c, o); b1 = conv1.bias; b2s = conv2.bias + shortcut.bias.  Returns NS2_UNAVAILABLE (nothing launched)
 *   for any other shape: the caller takes the GEMM path. */
int ns2_seanet_resblock_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int C, const float* w1p, const float* b1,
                               const float* w2p, const float* wsp, const float* b2s, float* out, int64_t ldo, void* stream);
int ns2_seanet_unpad(const float* src, int64_t ld_src, int prefix, float* dst, int64_t ld_dst, int B, int64_t T, int C, void* stream);
int64_t ns2_lstm_state_floats(int B, int H);
int ns2_lstm_layer(const float* xproj, int64_t ld_x, const float* w_hh, const float* b_hh, float* state, int64_t state_floats,
                   const float* resid, int64_t ld_r, float* out, int64_t ld_o, int B, int64_t T, int H, void* stream);

/* ns2_lstm2: BOTH layers of EnCodec's 2-layer nn.LSTM (HFENC:253-266, H = 512) in one launch, layer 2 running one frame behind
 *   layer 1 on its own workgroups and layer 1 forming layer 2's input projections (no GEMM between the layers).  xproj1 [B*T, 4H] =
 *   x W_ih1^T + b_ih1; w_hh1 / w_ih2 / w_hh2 [4H, H]; b_* [4H]; state = ns2_lstm2_state_floats() floats of caller scratch;
 *   out[b*T + t, :H] = h2_t (+ resid row).  Returns NS2_UNAVAILABLE -- nothing launched -- when the device cannot hold all the
 *   workgroups at once, B > 32, or NS2_LSTM_FUSED=0 / NS2_LSTM_PERSISTENT=0: call ns2_lstm_layer per layer instead. */
int64_t ns2_lstm2_state_floats(void);
int ns2_lstm2(const float* xproj1, int64_t ld_x, const float* w_hh1, const float* b_hh1, const float* w_ih2, const float* b_ih2,
              const float* w_hh2, const float* b_hh2, float* state, int64_t state_floats, const float* resid, int64_t ld_r, float* out,
              int64_t ld_o, int B, int64_t T, void* stream);

/* The one-launch LSTM recurrences synchronise their workgroups frame by frame through tagged values in global memory, which needs
 * every workgroup resident.  The launchers take that path only when the occupancy query says the device can hold them; should a
 * wait still time out (CU masking, a device saturated by other processes) the kernel gives up -- its output is then incomplete --
 * and counts the launch here instead of trapping.  Synchronises; call it after a codec run.  NS2_LSTM_PERSISTENT=0 forces the
 * per-step kernel. */
int ns2_lstm_abort_count(int reset, int64_t* count);
/* test hook: set that counter, as if n launches had given up (exercises the caller's fallback from the one-launch recurrences) */
int ns2_debug_lstm_inject_abort(int n);

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

/* EnCodec RVQ (HFENC:364-369, 424-447; reference call sites NS2:1445, NS2:1611, NS2:1496).
 * cb_norm: [Q, C] scratch filled by ns2_rvq_prepare (once per codebook set). codes: [M, Q] int64; emb/residual [M, D] or null */
int ns2_rvq_prepare(const float* codebooks, float* cb_norm, int Q, int C, int D, void* stream);
int ns2_rvq_encode(const float* x, const float* codebooks, const float* cb_norm, int64_t* codes, float* emb,
                   float* residual, int* near_tie_count, int M, int Q, int C, int D, float tie_eps, void* stream);
int ns2_rvq_decode(const int64_t* codes, const float* codebooks, float* emb, int M, int Q, int C, int D, void* stream);

/* RVQ cross-entropy of the training loss (NS2:1668-1684, `codec.rq(x_start, codes)`; csrc/rvq_ce.hip), everything fp32.  For the M rows of
 * x [M, D] and per quantizer q: dist_c = |r_q - E_q[c]|, row_loss[m][q] = log sum_c exp(-dist_c) + dist_target with target =
 * indices[m][q]; r_{q+1} = r_q - (the code nearest to r_q); loss[0] = sum_q mean_m row_loss[m][q], summed in a fixed order.
 * Optional outputs (null = not wanted): quantized_out [M, D] = 0 + E_0[nearest_0] + E_1[nearest_1] + ... in fp32, in stage order;
 * grad [M, D] = d loss / d x (the nearest codes are constants: sum_q d row_loss_q / d r_q, divided by M) -- null skips the second
 * sweep over the codebooks that forms it.  No atomics: loss and grad are bit-reproducible, and the loss does not depend on whether grad is asked for.
 * Defined edge behaviour: an index outside [0, C) (-1 included) makes that row's losses, hence loss[0], and its row of grad NaN -- no
 * error code, no host read; a residual that equals a code (dist = 0) gives the well-defined loss and that code contributes 0 to grad;
 * near-ties of the nearest code are decided by the fp32 scores (ns2_rvq_encode re-decides them in fp64, this one does not).
 * cb_norm: what ns2_rvq_prepare filled.  workspace: ns2_rvq_ce_workspace_bytes(M, Q, quantized_out != null) bytes (0 without
 * quantized_out).  NS2_ERR_ARG for D != 128 or C % 64 != 0, as ns2_rvq_encode. */
int64_t ns2_rvq_ce_workspace_bytes(int M, int Q, int want_quantized);
int ns2_rvq_ce(const float* x, const float* codebooks, const float* cb_norm, const int64_t* indices, float* row_loss, float* loss,
               float* quantized_out, float* grad, int M, int Q, int C, int D, void* workspace, int64_t workspace_bytes, void* stream);

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
void ns2_model_destroy(ns2_model* m);

/* ------------------------------------------------------------------ training: the backward pass
 * What `loss.backward()` runs for the denoiser (NS2:1635 `pred = self.model(...)` under autograd, NS2:1637-1666 the loss,
 * NS2:1886 `accelerator.backward`).  Two training arithmetics, selected per call by `precision`:
 *   3 = bf16 hi / lo planes, three bf16 MFMA products per contraction (the fp32 exponent range: no loss scaling);
 *   4 = "mixed": FMT_H8 lines, one IEEE-half product + both correction terms on the fp8 MFMA (2 MFMA units instead of 3).  IEEE half
 *       stops at 65504 and loses precision below 6e-5, so the caller scales the loss (a power of two; every gradient is linear in
 *       it) -- the reference trains under accelerate's fp16 mixed precision the same way (NS2:1710-1711, 1723-1726).  Values that
 *       leave the half range are counted (ns2_saturation_count, ns2_saturation_peek): an overflowed step is detected, not silently clamped.
 *       The attention products stay bf16 x3 at both precisions (q / k / v / dO planes are bf16 hi / lo: ns2_linear with out_precision = 3).
 * The contractions reuse the forward GEMM family:
 *   dgrad  dX = dY W   : ns2_linear (fp32 output) on a SECOND pack of the weight -- ns2_weight_pack of W^T ([in, out, taps] with the taps
 *                        flipped), conv_taps as in the forward, pad_left = 0 (the gradient of a causal conv looks ahead);
 *   wgrad  dW = dY^T X : ns2_wgrad on TRANSPOSED planes (contraction over the tokens), split over fixed slots + fixed-order sum.
 * Every reduction of this section is slot based and summed in a fixed order: gradients are deterministic, no atomics. */

/* re-pack a weight IN PLACE from new fp32 values (same shape / flags as the ns2_weight_pack call that made it): stream-ordered,
 * no allocation, no synchronisation -- the per-step refresh of an optimizer's weights */
int ns2_weight_update(ns2_weight* w, const float* w_src, const float* extra1x1, void* stream);

/* Every pack of a training pass in ONE launch.  A part = a rectangle of a packed weight (rows [row0, row0 + rows), columns per tap
 * [col0, col0 + cols) of a plain ns2_weight_pack weight: no GEGLU permutation, no extra 1x1 block) and where its fp32 values live:
 * element (r, c, tap) at src[r * sr + c * sc + tap * st], strides in elements and possibly negative -- the parameter's own storage
 * serves the forward pack (sr = C T, sc = T, st = 1), the dgrad pack W^T (sr = T, sc = C T) with flipped taps (st = -1 from src + T - 1)
 * and q | kv concatenations (two parts) without any copy.  ns2_weights_repack_build writes the device table (caller-owned memory of
 * ns2_weights_repack_table_bytes(n) bytes; synchronises once), ns2_weights_repack replays it: stream-ordered, no allocation. */
typedef struct {
  ns2_weight* w; const float* src;
  int64_t sr, sc, st;
  int row0, rows, col0, cols;
} ns2_repack_part;
int64_t ns2_weights_repack_table_bytes(int n);
int ns2_weights_repack_build(const ns2_repack_part* parts, int n, void* table_device, int64_t table_bytes, int64_t* total_blocks, void* stream);
int ns2_weights_repack(const void* table_device, int n, int64_t total_blocks, void* stream);
/* after ns2_weights_repack: rebuild the tiled images (ns2_weight_tile_conv3 / _linear / _wavenet) of those weights that have them --
 * one small launch per such weight, stream-ordered, no allocation.  With it packs that carry images may be part of a repack table. */
int ns2_weights_retile(ns2_weight* const* weights, int n, void* stream);

/* fp32 gradient x [M, C] (row stride ldx) -> any of
 *   row planes [M, ld_row] (zero beyond C)                                  -- the A operand of the dgrad GEMM;
 *   transposed planes T[c][m] with ld_t token columns (ld_t a multiple of 32, zero beyond M) and t_rows rows (zero beyond C; a
 *     W operand of ns2_wgrad needs its rows padded to a multiple of 256)    -- the operands of ns2_wgrad;
 *     per_batch != 0: T[b * t_rows + c][n] per utterance of seq_len tokens   -- the transposed operands of ns2_attention_bwd;
 *     shift: T[c][m] = x[m - shift][c] if m - shift lies in the utterance of m (seq_len tokens each), else 0;
 *   colsum_partial [ns2_grad_prep_slices(M, ld_t)][C]: column sums of 64-row tiles (sum the slots with ns2_reduce_slices:
 *     the bias gradient). */
int64_t ns2_grad_prep_slices(int M, int64_t ld_t);
int ns2_grad_prep(const float* x, int64_t ldx, int M, int C, int seq_len, int shift, uint16_t* row_hi, uint16_t* row_lo, int ld_row,
                  uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, float* colsum_partial, int precision, void* stream);
/* the same transposition for an activation that already exists as operand planes (columns [in_col0, in_col0 + C) of [M, ld_in]):
 * tap t of a causal conv (NS2:583-595) contributes x[n - (k - 1 - t) * dilation], i.e. shift = (k - 1 - t) * dilation */
int ns2_planes_transpose(const uint16_t* in_hi, const uint16_t* in_lo, int ld_in, int in_col0, int M, int C, int seq_len, int shift,
                         uint16_t* t_hi, uint16_t* t_lo, int64_t ld_t, int t_rows, int per_batch, int precision, void* stream);
/* out[o * inner + j] (+)= sum_s partial[(o * S + s) * inner + j], s in increasing order */
int ns2_reduce_slices(const float* partial, int64_t outer, int S, int64_t inner, float* out, int accumulate, void* stream);
/* weight gradient of nn.Linear / CausalConv1d (NS2:583-595, 1021-1024, 1051-1069): dw[r, k, t] = sum_m dY[m, r] * X_t[m, k].
 * dyt: transposed planes of dY, R rows; xt: transposed planes of the T (shifted) inputs stacked along the rows, tap t at rows
 * [t * Kp, t * Kp + K), allocated (zeros) up to the next multiple of 256 rows; both with ld_t token columns.  dw [R, K, T] fp32
 * (the nn.Conv1d layout; T = 1: nn.Linear).  workspace = ns2_wgrad_workspace_bytes(R, T * Kp, ld_t) bytes of caller scratch. */
int64_t ns2_wgrad_workspace_bytes(int R, int ncols, int64_t ld_t);
int ns2_wgrad(const uint16_t* dyt_hi, const uint16_t* dyt_lo, const uint16_t* xt_hi, const uint16_t* xt_lo, int64_t ld_t, int R, int T,
              int Kp, int K, float* dw, void* workspace, int64_t workspace_bytes, int precision, void* stream);

/* The same gradient from the TOKEN-MAJOR operand planes themselves: dy [M, ld_dy] (the row planes ns2_grad_prep writes for the dgrad
 * GEMM), x [M, ld_x] (the operand planes the forward GEMM read).  Tap t of a causal conv's gradient reads x[m - (T - 1 - t) * dil]
 * inside the utterance of m (seq_len tokens, >= 32, M a multiple of it); T = 1: nn.Linear (dil / seq_len ignored).  The kernel forms
 * its MFMA fragments with gfx950's LDS transpose reads, so neither transposed nor shifted copies of the operands exist in memory.
 * Any shape is computed; ns2_wgrad_rows_preferred says whether this route is the faster one (the 256 x 256 kernel must fill the chip:
 * the dim = 128 model's narrow gradients stay on ns2_wgrad, which picks the 128 x 128 kernel).  workspace = ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32)). */
int ns2_wgrad_rows_preferred(int R, int ncols, int64_t M);
int ns2_wgrad_rows(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x, int64_t M,
                   int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes, int precision,
                   void* stream);

/* WavenetResBlock's FiLM + gate (NS2:629-636) for the unfused training forward: out = tanh(z) * sigmoid(z), z = h * gamma_b + beta_b,
 * film[b] = [gamma (d) | beta (d)]; and its backward: dh = dg g'(z) gamma, partial[(b * slices + s)] = [sum dg g'(z) h | sum dg g'(z)]
 * over the s-th group of tokens of utterance b (ns2_film_gate_slices(seq_len) groups; ns2_reduce_slices gives d film [B, 2 d]) */
int ns2_film_gate_fwd(const float* h, int64_t ldh, const float* film, int film_ld, int seq_len, int64_t M, int d, float* out, int64_t ldo,
                      void* stream);
int ns2_film_gate_slices(int seq_len);
int ns2_film_gate_bwd(const float* dg, int64_t lddg, const float* h, int64_t ldh, const float* film, int film_ld, int B, int seq_len, int d,
                      float* dh, int64_t lddh, float* partial, void* stream);
/* GEGLU (NS2:1004-1007) on the saved pre-activation pre [M, ldp] = [x (f) | gate (f)]: planes of gelu(gate) * x, and the backward */
int ns2_geglu_fwd(const float* pre, int64_t ldp, int64_t M, int f, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream);
int ns2_geglu_bwd(const float* dh, int64_t lddh, const float* pre, int64_t ldp, int64_t M, int f, float* dpre, int64_t lddp, void* stream);
/* RMSNorm backward (NS2:727-746): dx = (dx_add ? dx_add : 0) + dL/dx (dx may alias dx_add: the residual stream's gradient);
 * cond_partial [B * slices][2 d] -> the adaptive (gamma_c, beta_c) gradients, gamma_partial [B * slices][d] -> the learned gamma's.
 * d: a multiple of 4, at most 2048; the leading dimensions multiples of 4.  A workgroup keeps 12 d floats in dynamic LDS: beyond
 * d = 1365 that is more than 64 KiB (96 KiB at d = 2048), and the launcher raises the kernel's dynamic-LDS limit before it launches. */
int ns2_rmsnorm_bwd_slices(int seq_len);
int ns2_rmsnorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, const float* cond, int cond_ld, int B,
                    int seq_len, int d, const float* dx_add, float* dx, int64_t lddx, float* cond_partial, float* gamma_partial, void* stream);

/* The training forward is ns2_attention_fwd with `lse` set.
 * delta[b, h, q] = sum_d dO[q, 64 h + d] * O[q, 64 h + d] (O from its operand planes, o_precision 3 or 4) */
int ns2_attention_delta(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H, int Nq,
                        float* delta, int o_precision, void* stream);
/* flash-attention backward, head dim 64: dq = scale * dS k, dk = scale * dS^T q, dv = P^T dO with P recomputed from lse and
 * dS = P (dO v^T - delta).  q / k / v / d_out: row-major planes (head h at columns col0 + 64 h) -- the kernels form K^T, Q^T and
 * dO^T themselves (LDS transpose reads of the row-major tiles: round 4 took per-utterance transposed copies here).  dq == NULL or
 * dk == dv == NULL skips that half (cross-attention to a context that needs no gradient). */
typedef struct {
  const uint16_t* q_hi; const uint16_t* q_lo; int ldq, q_col0;
  const uint16_t* k_hi; const uint16_t* k_lo; int ldk, k_col0;
  const uint16_t* v_hi; const uint16_t* v_lo; int ldv, v_col0;
  const uint16_t* do_hi; const uint16_t* do_lo; int lddo;
  const float* lse; const float* delta;
  float* dq; int lddq, dq_col0;
  float* dk; int lddk, dk_col0;
  float* dv; int lddv, dv_col0;
  int B, H, Nq, Nk; float scale;
  /* round 5: gp_q / gp_kv != 0 -- that half of the gradients leaves the kernel as OPERAND PLANES instead of fp32 (the q | k | v projection's
   * dgrad and wgrad GEMMs are their only consumers): planes [rows, gp_ld] of precision gp_precision (3: bf16 hi / lo lines, 4: FMT_H8),
   * dq at columns dq_col0 + 64 h of row b Nq + q, dk / dv at dk_col0 / dv_col0 + 64 h of row b Nk + k (column offsets multiples of 32) */
  uint16_t* gp_hi; uint16_t* gp_lo; int gp_ld, gp_precision, gp_q, gp_kv;
  /* the mask and the dropout of the forward this is the backward of, as in ns2_attn_args (all zero: neither) */
  const uint8_t* key_mask; float dropout_p; const uint32_t* dropout_seed; unsigned dropout_call;
} ns2_attn_bwd_args;
int ns2_attention_bwd(const ns2_attn_bwd_args* args, void* stream);

/* ---- training of the conditioning encoders (NS2:228-341, 1073-1115; trained jointly with the denoiser: NS2:1538-1543, 1635) ----
 * Transformer's attention has two things Model's has not, a key-padding mask and dropout on the softmax output: the key_mask and
 * dropout_* fields of ns2_attn_args / ns2_attn_bwd_args. */
/* debugging / tests: out [B, H, Nq, Nk] bytes, 1 where the kernels above keep P[b, h, q, k] */
int ns2_dropout_keep_mask(const uint32_t* seed, unsigned call, float dropout_p, int B, int H, int Nq, int Nk, uint8_t* out, void* stream);
/* SiLU of the encoders' k = 9 convolutions (NS2:247, 306-311) on the fp32 pre-activation x [M, ldx], C columns, and its backward
 * dx = dy silu'(x).  Leading dimensions multiples of 4, 16-byte aligned pointers. */
int ns2_silu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream);
int ns2_silu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream);
/* gradient of PhonemeEncoder's token embedding (NS2:281-284): dw [rows, d] = sum of dy [M, lddy] rows per id, negative ids counting as
 * pad_id (an ordinary row of the table, as upstream); summed in ascending token order: bit-reproducible */
int ns2_embedding_bwd(const int64_t* ids, int64_t M, int pad_id, const float* dy, int64_t lddy, int rows, int d, float* dw, void* stream);

/* ---- training of the DurationPitchPredictor (NS2:344-527; its duration / pitch L1 terms, NS2:1578-1589) ----
 * The training FORWARD of GroupNorm + SiLU (+ residual) is ns2_groupnorm_silu with an fp32 output: the caller keeps its workspace, which
 * holds the per-chunk (count, mean, M2) slots.  ns2_groupnorm_silu_bwd takes that buffer as `stats` and combines the slots in the same
 * order with the same code, so it normalises with the forward's mean and rstd bit for bit.  With xh = (x - mean) rstd, z = xh w + b,
 * dz = dy silu'(z):  dweight_dbias [2 C] = (sum dz xh | sum dz) over all rows;  dx = rstd (dz w - s1 / N - xh s2 / N), s1 = sum dz w,
 * s2 = sum dz w xh per (utterance, group), N = n C / groups.  (The residual's gradient is dy itself.)  dy [B n, lddy], x and dx [B n, C].
 * Column sums per 32-row chunk go to fixed slots of the workspace and are added in a fixed order: no atomics, bit-reproducible. */
int64_t ns2_groupnorm_silu_bwd_workspace_bytes(int B, int n, int C);
int ns2_groupnorm_silu_bwd(const float* dy, int64_t lddy, const float* x, int B, int n, int C, int groups, const float* weight,
                           const float* bias, float eps, const void* stats, int64_t stats_bytes, float* dx, float* dweight_dbias,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* backward of out = relu(h . w + b) (ns2_row_dot with relu): g = dout where out > 0 else 0;  dh [M, lddh] = g w;  dw_db [K + 1] =
 * (sum_m g h[m, :] | sum_m g), from per-64-row slots added in a fixed order.  K, ldh, lddh multiples of 4. */
int64_t ns2_row_dot_relu_bwd_workspace_bytes(int64_t M, int K);
int ns2_row_dot_relu_bwd(const float* dout, const float* out, const float* h, int64_t ldh, const float* w, int64_t M, int K, float* dh,
                         int64_t lddh, float* dw_db, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training of the Aligner (aligner.py; the only route that hands it a gradient is the forward-sum / bin loss of NS2:1587-1602) ----
 * Exact arithmetic, fixed summation orders, no atomics: two runs give the same bits.  Lengths are int32 [B] on the device, clamped to
 * [0, size]; nothing here reads device data on the host.  Limits: n <= 1024, T <= 8192, C <= 256. */
/* ReLU between AlignerNet's convolutions (aligner.py:30-51) on the kept fp32 pre-activation x [M, ldx], C columns, and its backward
 * dx = dy where x > 0.  Leading dimensions multiples of 4, 16-byte aligned pointers (as ns2_silu_fwd / ns2_silu_bwd). */
int ns2_relu_fwd(const float* x, int64_t ldx, int64_t M, int C, float* out, int64_t ldo, void* stream);
int ns2_relu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C, float* dx, int64_t lddx, void* stream);
/* backward of ns2_align_attn (aligner.py:72-90: cdist, masked fill, softmax).  queries [B * T, C], keys [B * n, C], aln_log
 * [B, 1, T, n] and aln_soft [B, n, T] as ns2_align_attn wrote them, g_log [B, 1, T, n] and g_soft [B, n, T] the gradients of the two
 * outputs (either may be null).  With G = g_log + soft (g_soft - sum_i soft g_soft) on the live cells (i < text_lens[b]) and
 * w = G / dist, w = 0 where the cell is masked or dist == 0 (torch.cdist's convention: never NaN or inf):
 *   dq [B * T, C]: dq_t = sum_i w (q_t - k_i), phonemes in ascending order;
 *   dk [B * n, C]: dk_i = sum_t w (k_i - q_t), per slice of 256 frames in ascending order, the slices through the fixed-order
 *   slice reducer (ns2_reduce_slices' kernel).  The DIRECT form is summed (rowsum(w) q - w K cancels where q ~ k).
 * workspace = ns2_align_attn_bwd_workspace_bytes bytes: w [B, T, n] fp32 + ceil(T / 256) slots of [B, n, C] fp32; 16-byte aligned. */
int64_t ns2_align_attn_bwd_workspace_bytes(int B, int T, int n, int C);
int ns2_align_attn_bwd(const float* queries, const float* keys, const float* aln_log, const float* aln_soft, const float* g_log,
                       const float* g_soft, const int* text_lens, int B, int T, int n, int C, float* dq, float* dk, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* ForwardSumLoss and BinLoss (aligner.py:132-167, 169-183) on aln_log [B, 1, T, n]; each loss is requested by a non-null output
 * pointer (a device scalar), both share the row statistics.
 * Forward-sum: per frame t < mel_lens[b] the log-softmax over [blank_logprob | aln_log[t, 0 .. L - 1]], L = text_lens[b] (columns
 * > L of the n + 1 wide row are excluded); CTC with blank 0, targets 1 .. L, S = 2 L + 1 states, every skip between labels allowed
 * (they are distinct); zero_infinity (an infeasible utterance gives loss 0, gradient 0); fs_loss = mean_b(nll_b / max(L_b, 1)).
 * One workgroup per utterance runs the alpha recursion over the frames, the states spread over its lanes, and keeps alpha
 * [B, T, 2 n + 1] in the workspace.  Arithmetic: fp64 on probabilities scaled per frame by a power of two (the exponent of the frame
 * before's maximum: exact, and the sum of the exponents gives nll) -- an fp32 log-space recursion leaves the gradient 300 .. 10000 x 2^-24
 * of its largest element off (so does torch's fp32 ctc_loss); emissions below e^-700 count as e^-700.
 * Bin: bin_loss = sum(hard log_softmax(aln_log over the columns <= L)) / B, hard [B, n, T] the 0/1 path (column L is kept, as upstream:
 * it holds the aligner's -FLT_MAX).
 * ns2_align_losses_bwd (same aln_log, hard, lengths, blank_logprob and the workspace the forward filled): d_log [B, 1, T, n] =
 * g_fs (softmax - occupancy) / (max(L, 1) B) on the live cells of the frames t < mel_len (beta recursion, the occupancies of a frame
 * normalised to sum 1 over its states; the blank column's share is dropped) + g_bin (hard - softmax sum_i hard) / B on the columns <= L; exactly 0 elsewhere.  g_fs, g_bin: device scalars, the
 * gradients of the two losses (null = that loss takes no part).
 * workspace = ns2_align_losses_workspace_bytes bytes: 4 floats per frame, B doubles, 2 B T (2 n + 1) floats (alpha, and the backward's
 * alpha + beta: the forward's part is only read, so a backward may be repeated). */
int64_t ns2_align_losses_workspace_bytes(int B, int T, int n);
int ns2_align_losses_fwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, int B, int T, int n,
                         float blank_logprob, float* fs_loss, float* bin_loss, void* workspace, int64_t workspace_bytes, void* stream);
int ns2_align_losses_bwd(const float* aln_log, const float* hard, const int* text_lens, const int* mel_lens, const float* g_fs,
                         const float* g_bin, int B, int T, int n, float blank_logprob, float* d_log, void* workspace,
                         int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NS2HIP_H */
