// extern "C" surface of libns2hip (declared in include/ns2hip.h; the codec and pitch entries in include/ns2hip_audio.h): error plumbing +
// op-level entry points.
// The Model executor entry points live in model_exec.cpp.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <vector>

#include "ns2_host.h"
#include "gemm_route.h"

namespace ns2 {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

// the range-guard counters of the library, one per translation unit that includes ns2_common.h (ns2_sat_registry.h).  Filled by static
// initialisers of OTHER translation units, in no particular order: a function-local static (zero-initialised storage, no allocation, no
// HIP call), so it exists whoever registers first, and the library still loads where there is no GPU.
namespace {
struct SatRegistry { SatCounter c[SAT_COUNTERS_MAX]; int n; bool full; };
SatRegistry& sat_registry() {
  static SatRegistry r;
  return r;
}
}  // namespace
void register_sat_counter(const SatCounter& c) {
  SatRegistry& r = sat_registry();
  if (r.n < SAT_COUNTERS_MAX) r.c[r.n++] = c;
  else r.full = true;
}
const SatCounter* sat_counters(int* n) {
  const SatRegistry& r = sat_registry();
  *n = r.n;
  return r.full ? nullptr : r.c;
}

}  // namespace ns2

using namespace ns2;


static inline int prec_ok(int p) { return p >= 1 && p <= 4; }

extern "C" const char* ns2_last_error(void) { return g_err; }
extern "C" int ns2_version(void) { return 125; }   // 125: the Wavenet tail fold and the wide RMSNorm kernel (include/ns2hip.h): ns2_tail_fold, ns2_debug_force_tail_fold, ns2_debug_force_norm, ns2_debug_norm_last; 124: the feed-forward fold (include/ns2hip.h): ns2_ff_fold, ns2_debug_force_fold, the FF conv kernel writes fp32; 123: the RVQ cross-entropy of the training loss: ns2_rvq_ce (+ _workspace_bytes); 122: training of the Aligner: ns2_relu_fwd / _bwd, ns2_align_attn_bwd (+ _workspace_bytes), ns2_align_losses_fwd / _bwd (+ _workspace_bytes); 121: two utterance chains: ns2_debug_force_chains / _chains_last / _chain_rule, ns2_model_profile_end counts logical products; 120: one argument block per Linear / Conv1d product: ns2_linear(ns2_linear_args) replaces ns2_linear_f32 / _split / _split_as / _geglu / _qkv; 119: one argument block per attention direction: ns2_attention_fwd(ns2_attn_args) replaces ns2_attention / _hd / _lse / _lse_masked, ns2_attn_bwd_args carries the mask and dropout of the removed bwd_masked entry; 118: ns2_debug_force_attention, ns2_debug_attention_fast_launches (attn_fast_kernel.h); 117: the range-guard counters register themselves: ns2_saturation_counters / _counter_name / _peek replace ns2_saturation_peek_async / _peek_train_async; 116: ns2_groupnorm_silu, ns2_length_regulate(_totals), ns2_row_dot (duration_pitch.hip); 115: ns2_weights_retile; 114: ns2_attention_hd (head dims 32 / 64 / 128), ns2_model_create takes dim_head 32 / 128; 113: ns2_weight_tile_conv3 + ns2_conv3_input_ld (the dedicated FF causal conv kernel, ffconv_kernel.h), ns2_weight_tile_linear (gemm3_kernel.h), ns2_weight_tile_wavenet (wavenet3_kernel.h), ns2_debug_force_gemm(4 / 5); 112: ns2_seanet_resblock_narrow; 111: training entry points take a precision (3 = bf16 x3, 4 = mixed on FMT_H8 lines), ns2_linear_split_as; 110: backward pass (capi_train.cpp: ns2_wgrad, ns2_attention_bwd, ...), ns2_weight_update; 109: ns2_seanet_conv_narrow; 108: ns2_seanet_prep2; 107: ns2_lstm2 (two LSTM layers, one launch); 106: ns2_saturation_peek_async; 105: ns2_lstm_layer takes the scratch size (persistent recurrence); 104: model precision 5 (per-site plan); 103: precision 2 / 4 at op level, caller-owned skinny-linear scratch
extern "C" int ns2_debug_force_gemm(int kernel) {
  ARGCHK(kernel >= 0 && kernel <= 5, "ns2_debug_force_gemm: 0 auto, 1 = 128x128 kernel, 2 = 256x256 kernel, 3 = auto without split-K, 4 = auto without the dedicated kernels (FF conv, lean linear, lean Wavenet), 5 = auto without split-K, the dedicated kernels whenever eligible");
  force_gemm_kernel(kernel);
  gemm_hook_changed();
  return NS2_OK;
}

extern "C" int ns2_debug_force_attention(int kernel) {
  ARGCHK(kernel >= 0 && kernel <= 1, "ns2_debug_force_attention: 0 auto, 1 = attn_kernel for every call (never attn_fast_kernel)");
  force_attention_kernel(kernel);
  return NS2_OK;
}
extern "C" int64_t ns2_debug_attention_fast_launches(void) { return attention_fast_launches(); }

extern "C" int ns2_weight_pack(const float* w, int rows, int cols, int taps, int geglu, const float* extra1x1, int precision,
                               ns2_weight** out, void* stream) {
  ARGCHK(w && out && rows > 0 && cols > 0 && taps >= 1 && prec_ok(precision), "ns2_weight_pack: bad arguments");
  ARGCHK(!(geglu && (taps != 1 || extra1x1 || (rows & 1))), "ns2_weight_pack: geglu needs taps=1, no extra, even rows");
  ns2_weight* h = new ns2_weight();
  h->taps = taps; h->geglu = geglu; h->has_extra = extra1x1 != nullptr; h->cols_p = (cols + 31) / 32 * 32;
  int r = pack_weight_public(w, rows, cols, taps, geglu, extra1x1, precision, &h->w, &h->owned, (hipStream_t)stream);
  if (r != NS2_OK) { ns2_weight_free(h); return r; }
  {   // keep the row map on the device: ns2_weight_update (training: the weights change every step) re-packs without allocating
    h->cols = cols;
    const std::vector<int> m = geglu ? geglu_row_map(rows / 2, h->w.rows_p) : [&] {
      std::vector<int> id(h->w.rows_p, -1);
      for (int i = 0; i < rows && i < h->w.rows_p; ++i) id[i] = i;
      return id;
    }();
    if (hipMalloc((void**)&h->d_map, m.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(h->d_map, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("ns2_weight_pack: could not keep the row map");
      ns2_weight_free(h);
      return NS2_ERR_HIP;
    }
    h->owned.push_back(h->d_map);
  }
  *out = h;
  return NS2_OK;
}
// Give a k = 3 conv weight packed for precision 2 (dense IEEE half) the tiled images of the dedicated FF causal conv kernel
// (ffconv_kernel.h).  ns2_linear calls with plane output then take that kernel whenever the call is eligible: dilation 1, causal
// padding, no activation, M and seq_len multiples of 256, activations with rows of ns2_conv3_input_ld(cols) elements, FMT_H8 or dense
// half output.  One-time set-up like ns2_weight_pack (allocates on the first call); ns2_weight_update refreshes the images with the pack.
extern "C" int ns2_weight_tile_conv3(ns2_weight* w, void* stream) {
  ARGCHK(w && w->taps == 3 && !w->geglu && !w->has_extra && w->w.fmt == FMT_F16 && !w->w.lo, "ns2_weight_tile_conv3: a k = 3 conv weight packed for precision 2");
  return build_conv3_tiles(&w->owned, &w->w, (hipStream_t)stream);
}
// Give a linear weight (taps = 1; also the GEGLU packing) packed for precision 4 (FMT_H8 lines) the tiled images of the lean mixed linear
// kernel (gemm3_kernel.h): ns2_linear then takes that kernel, whatever the output, when M % 256 == 0 and K >= 96.  One-time set-up
// (allocates on the first call); ns2_weight_update refreshes the images with the pack; after ns2_weights_repack, ns2_weights_retile does.
extern "C" int ns2_weight_tile_linear(ns2_weight* w, void* stream) {
  ARGCHK(w && w->taps == 1 && !w->has_extra && w->w.fmt == FMT_H8 && w->w.nkt >= 3, "ns2_weight_tile_linear: a linear weight (taps = 1, K >= 96) packed for precision 4");
  return build_lin_tiles(&w->owned, &w->w, (hipStream_t)stream);
}
// Give a WavenetResBlock weight (taps = 3 + the 1x1 res conv, packed for precision 4) the tiled images of the lean block kernel of the
// hybrid plan (wavenet3_kernel.h): ns2_wavenet_block at precision 5 then takes that kernel when channels % 256 == 0 (square), M and
// seq_len are multiples of 256 and dilation <= 128.  Same life-cycle rules as ns2_weight_tile_conv3.
extern "C" int ns2_weight_tile_wavenet(ns2_weight* w, void* stream) {
  ARGCHK(w && w->taps == 3 && w->has_extra && !w->geglu && w->w.fmt == FMT_H8 && (w->cols_p % 128) == 0 && w->w.N == w->cols_p && (w->w.N % 256) == 0,
         "ns2_weight_tile_wavenet: a square WavenetResBlock weight (taps = 3, extra1x1) packed for precision 4, channels a multiple of 256");
  PackedW& W = w->w;
  if (!W.tw1) {
    void *t1 = nullptr, *t2 = nullptr;
    HIPRET(hipMalloc(&t1, wavenet3_tiles_bytes(W.rows_p, w->cols_p, 1, 1))); w->owned.push_back(t1);
    HIPRET(hipMalloc(&t2, wavenet3_tiles_bytes(W.rows_p, w->cols_p, 1, 2))); w->owned.push_back(t2);
    W.tw1 = static_cast<bf16_t*>(t1); W.tw2 = static_cast<bf16_t*>(t2);
  }
  HIPRET(wavenet3_build_tiles(W.hi, W.rows_p, w->cols_p, 1, W.tw1, W.tw2, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_conv3_input_ld(int cols) { return cols > 0 ? ffconv3_lda((cols + 31) / 32 * 32) : 0; }
extern "C" void ns2_weight_free(ns2_weight* w) {
  if (!w) return;
  for (void* p : w->owned) (void)hipFree(p);
  delete w;
}

extern "C" int ns2_split_f32(const float* x, int ldx, int M, int d, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision,
                             void* stream) {
  ARGCHK(x && out_hi && prec_ok(precision), "ns2_split_f32: bad arguments");
  ARGCHK(precision != 2 || !out_lo, "ns2_split_f32: precision 2 (fp16) has no lo plane");
  HIPRET(launch_split(x, ldx, nullptr, 0, 0, 0, out_hi, out_lo, ldo, M, d, 0, (hipStream_t)stream, operand_fmt(precision)));
  return NS2_OK;
}
extern "C" int ns2_join_f32(const uint16_t* hi, const uint16_t* lo, int ld, float* out, int ldo, int64_t M, int d, int precision,
                            void* stream) {
  ARGCHK(hi && out && prec_ok(precision), "ns2_join_f32: bad arguments");
  ARGCHK(precision != 2 || !lo, "ns2_join_f32: precision 2 (fp16) has no lo plane");
  HIPRET(launch_join(hi, lo, ld, out, ldo, (long)M, d, (hipStream_t)stream, operand_fmt(precision)));
  return NS2_OK;
}

// The one translation of a ns2_linear_args block into the kernels' (ns2_kernels.h GemmArgs, built on ns2_host.h gemm_args).  Everything
// ns2_linear refuses, it refuses here, before any HIP call; what needs only the block comes before the first read of *w.
static int linear_args_from(const ns2_linear_args* p, GemmArgs* out) {
  ARGCHK(p != nullptr, "ns2_linear: null argument block");
  ARGCHK(p->w != nullptr, "ns2_linear: w is null");
  ARGCHK(p->a_hi != nullptr, "ns2_linear: a_hi is null");
  ARGCHK(prec_ok(p->precision), "ns2_linear: precision must be 1 .. 4");
  const bool planes = p->out_hi != nullptr, qkv = p->vt_hi != nullptr;
  ARGCHK(planes || p->out_f32, "ns2_linear: no output (neither out_f32 nor out_hi)");
  ARGCHK(!planes || !p->out_f32, "ns2_linear: both out_f32 and out_hi (exactly one output)");
  ARGCHK(planes || !(qkv || p->out_precision), "ns2_linear: vt_hi and out_precision need out_hi, not out_f32");
  ARGCHK(!planes || !p->resid, "ns2_linear: resid needs out_f32, not out_hi");
  ARGCHK(p->pad_left >= -1 && p->pad_left < (p->conv_taps > 0 ? p->conv_taps : 1), "ns2_linear: pad_left must be -1 (causal) or in [0, conv_taps)");
  ARGCHK(p->act >= 0 && p->act <= 2, "ns2_linear: act must be 0 (none), 1 (SiLU) or 2 (ELU)");
  ARGCHK(p->out_precision == 0 || (prec_ok(p->out_precision) && (p->out_precision == 1 || (p->out_precision == 2) == (p->out_lo == nullptr))),
         "ns2_linear: out_precision 0 (= precision) or 1 .. 4, and out_lo must be null for dense IEEE-half output, hi + 32 for interleaved lines");
  ARGCHK(!qkv || !(p->bias || p->act || p->conv_taps || p->out_precision), "ns2_linear: vt_hi (the fused q | k | v) excludes bias, act, conv_taps and out_precision");
  ARGCHK(!qkv || (p->seq_len > 0 && p->M % p->seq_len == 0 && (p->split_col % 32) == 0 && p->vt_ld >= p->seq_len && (p->vt_ld & 7) == 0),
         "ns2_linear: bad q | k | v shapes (seq_len divides M, split_col a multiple of 32, vt_ld >= seq_len and a multiple of 8)");
  ARGCHK(!qkv || p->ldo >= p->split_col, "ns2_linear: ldo smaller than split_col (the q | k rows would overlap)");
  ARGCHK(!qkv || !p->vt_lo || (p->vt_ld & 31) == 0, "ns2_linear: vt_ld must be a multiple of 32 with vt_lo (interleaved lines of 32 keys; the last line of a row would overlap the next row)");
  ARGCHK(!planes || qkv || (p->ldo & 1) == 0, "ns2_linear: ldo must be even");
  const ns2_weight& w = *p->w;
  // the weight's element format must be the one the requested precision multiplies in (fp16 for 2, bf16 planes for 1 / 3)
  ARGCHK(operand_fmt(p->precision) == w.w.fmt, "ns2_linear: w was packed for a different precision");
  ARGCHK(!w.has_extra && (p->conv_taps == 0 ? w.taps == 1 : w.taps == p->conv_taps),
         "ns2_linear: the packing of w does not match conv_taps (a weight with extra1x1 belongs to ns2_wavenet_block)");
  ARGCHK(p->lda >= w.cols_p, "ns2_linear: lda smaller than the padded K of w");
  ARGCHK(!qkv || p->split_col < w.w.N, "ns2_linear: split_col must lie below the rows of w");
  // no route's column tiles reach further (128 columns per tile on the 128 x 128 kernel and the split-K finish): the zeros of [N, ldo) would stay unwritten
  ARGCHK(!planes || qkv || w.geglu || p->ldo <= (w.w.N + 127) / 128 * 128, "ns2_linear: ldo larger than the rows of w rounded up to 128 (the columns beyond would stay unwritten)");
  GemmArgs& g = *out;
  g = gemm_args(w.w, p->a_hi, p->a_lo, p->lda, p->M);
  g.bias = p->bias;
  if (w.geglu) {
    ARGCHK(p->bias && planes && !(p->conv_taps || p->act || qkv || p->out_precision),
           "ns2_linear: a geglu weight needs the packed bias and out_hi, and excludes conv_taps, act, out_f32, vt_hi and out_precision");
    ARGCHK(p->ldo * 2 == w.w.N, "ns2_linear: ldo must be round_up(f, 32) for a geglu weight");
    set_geglu(g, p->out_hi, p->out_lo, p->ldo);
  } else if (qkv) {
    set_qkv(g, p->precision, p->seq_len, p->split_col, p->out_hi, p->out_lo, p->ldo);
    g.vt_hi = p->vt_hi; g.vt_lo = p->vt_lo; g.vt_ld = p->vt_ld;
  } else {
    if (p->conv_taps) set_conv(g, w.w, p->conv_taps, p->dilation, p->seq_len);
    g.pad_left = p->pad_left; g.act = p->act;
    if (planes) {
      set_out_planes(g, EPI_SPLIT, p->out_hi, p->out_lo, p->ldo);
      if (p->out_precision) g.out_fmt = operand_fmt(p->out_precision);
    } else {
      g.resid = p->resid; g.ldr = p->ldr; g.out_f = p->out_f32; g.ldo_f = p->ldo_f;
    }
  }
  return NS2_OK;
}
extern "C" int ns2_linear(const ns2_linear_args* p, void* stream) {
  GemmArgs g;
  if (int rc = linear_args_from(p, &g)) return rc;
  HIPRET(launch_gemm(g, p->precision, (hipStream_t)stream));
  return NS2_OK;
}
// the ragged forms of ns2_linear: what an entry refuses on its own account comes first, under its own name, before any device call
#define SKIP_SHAPE_CHK(name, row_lens, seq_len, M)                                                                                  \
  ARGCHK((row_lens) != nullptr, name ": row_lens is null (the entry without lengths is the call that computes every row)");          \
  ARGCHK((seq_len) > 0 && ((seq_len) & 255) == 0, name ": seq_len must be a positive multiple of 256 (whole skipping granules per utterance)"); \
  ARGCHK((M) > 0 && (M) % (seq_len) == 0, name ": M must be whole utterances of seq_len rows")
extern "C" int ns2_linear_lens(const ns2_linear_args* p, const int* row_lens, int seq_len, void* stream) {
  ARGCHK(p != nullptr, "ns2_linear_lens: null argument block");
  SKIP_SHAPE_CHK("ns2_linear_lens", row_lens, seq_len, p->M);
  ARGCHK(p->seq_len == 0 || p->seq_len == seq_len, "ns2_linear_lens: args->seq_len differs from seq_len");
  GemmArgs g;
  if (int rc = linear_args_from(p, &g)) return rc;
  g.row_lens = row_lens; g.lens_seq = seq_len;
  HIPRET(launch_gemm(g, p->precision, (hipStream_t)stream));
  return NS2_OK;
}
// the same entry under the training rule (zero bits in the hidden tiles of every output), and the
// host counter of the launches that went out with lengths (capi_train.cpp's ns2_wgrad_rows_lens bumps it too)
static std::atomic<long long> g_train_skip_launches{0};
void ns2::note_train_skip_launch() { g_train_skip_launches.fetch_add(1, std::memory_order_relaxed); }
extern "C" int64_t ns2_debug_train_skip_launches(void) { return g_train_skip_launches.load(std::memory_order_relaxed); }
extern "C" int ns2_linear_lens_zero(const ns2_linear_args* p, const int* row_lens, int seq_len, void* stream) {
  ARGCHK(p != nullptr, "ns2_linear_lens_zero: null argument block");
  SKIP_SHAPE_CHK("ns2_linear_lens_zero", row_lens, seq_len, p->M);
  ARGCHK(p->seq_len == 0 || p->seq_len == seq_len, "ns2_linear_lens_zero: args->seq_len differs from seq_len");
  GemmArgs g;
  if (int rc = linear_args_from(p, &g)) return rc;
  g.row_lens = row_lens; g.lens_seq = seq_len; g.zero_hidden = 1;
  const bool with_lens = plan_gemm(g, p->precision).route != GemmRoute::SplitK;      // (split K takes no lengths: every row is computed)
  HIPRET(launch_gemm(g, p->precision, (hipStream_t)stream));
  if (with_lens) note_train_skip_launch();
  return NS2_OK;
}
extern "C" int ns2_geglu_pack_bias(const float* bias, int f, float* packed, int packed_len, void* stream) {
  ARGCHK(bias && packed && f > 0, "ns2_geglu_pack_bias: bad arguments");
  const int rows_p = ((2 * ((f + 31) / 32 * 32)) + 255) / 256 * 256;
  ARGCHK(packed_len >= rows_p, "ns2_geglu_pack_bias: packed_len too small");
  std::vector<float> hb(2 * f), pb(packed_len, 0.f);
  HIPRET(hipMemcpy(hb.data(), bias, 2 * f * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<int> m = geglu_row_map(f, rows_p);
  for (int i = 0; i < rows_p; ++i)
    if (m[i] >= 0) pb[i] = hb[m[i]];
  HIPRET(hipMemcpy(packed, pb.data(), packed_len * sizeof(float), hipMemcpyHostToDevice));
  (void)stream;
  return NS2_OK;
}
extern "C" int ns2_ff_fold(const float* w_out, const float* w_conv, const float* b_conv, const float* b_out, int dim, int f, float* w_fold,
                           float* b_fold, void* stream) {
  ARGCHK(w_out && w_conv && b_conv && w_fold && b_fold && dim > 0 && f > 0, "ns2_ff_fold: bad arguments");
  HIPRET(launch_ff_fold(w_out, w_conv, b_conv, b_out, dim, f, w_fold, b_fold, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_tail_fold(const float* w_final, const float* w_skip, const float* b_skip, const float* b_final, int dim, int layers,
                             float* w_fold, float* b_fold, void* stream) {
  ARGCHK(w_final && w_skip && b_skip && w_fold && b_fold && dim > 0 && layers > 0, "ns2_tail_fold: bad arguments");
  HIPRET(launch_tail_fold(w_final, w_skip, b_skip, b_final, dim, layers, w_fold, b_fold, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_debug_force_norm(int kernel) {
  ARGCHK(kernel == 0 || kernel == 1, "ns2_debug_force_norm: 0 = by shape, 1 = rmsnorm_kernel for every call (never rmsnorm_wide_kernel)");
  force_norm_kernel(kernel);
  return NS2_OK;
}
extern "C" int ns2_debug_norm_last(void) { return norm_kernel_last(); }
static int wavenet_block_impl(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                              int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                              uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, const int* row_lens, void* stream) {
  // precision 5 (this entry point only) = precision 4 operands, the dilated conv as one half product, res_conv with the correction terms
  const int p1_half = precision == 5;
  if (p1_half) precision = 4;
  ARGCHK(w && a_hi && out_hi && conv_bias && res_bias && film && prec_ok(precision), "ns2_wavenet_block: bad arguments");
  ARGCHK(operand_fmt(precision) == w->w.fmt, "ns2_wavenet_block: weight was packed for a different precision");
  ARGCHK(w->taps == 3 && w->has_extra && seq_len > 0, "ns2_wavenet_block: weight must be packed with taps=3 and extra1x1");
  ARGCHK(ldo <= (w->w.N + 127) / 128 * 128, "ns2_wavenet_block: ldo larger than the channels rounded up to 128 (the columns beyond would stay unwritten)");
  GemmArgs g = gemm_args(w->w, a_hi, a_lo, lda, M);
  set_wavenet(g, w->w, dilation, seq_len, precision, p1_half);
  g.bias = conv_bias; g.bias2 = res_bias; g.film = film; g.film_ld = film_ld;
  set_out_planes(g, EPI_WAVENET, out_hi, out_lo, ldo);
  if (row_lens) { g.row_lens = row_lens; g.lens_seq = seq_len; }
  HIPRET(launch_gemm(g, precision, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_wavenet_block(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                                 int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                                 uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream) {
  return wavenet_block_impl(w, a_hi, a_lo, lda, M, seq_len, dilation, conv_bias, res_bias, film, film_ld, out_hi, out_lo, ldo, precision, nullptr, stream);
}
extern "C" int ns2_wavenet_block_lens(const ns2_weight* w, const uint16_t* a_hi, const uint16_t* a_lo, int lda, int M, int seq_len,
                                      int dilation, const float* conv_bias, const float* res_bias, const float* film, int film_ld,
                                      uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, const int* row_lens, void* stream) {
  SKIP_SHAPE_CHK("ns2_wavenet_block_lens", row_lens, seq_len, M);
  return wavenet_block_impl(w, a_hi, a_lo, lda, M, seq_len, dilation, conv_bias, res_bias, film, film_ld, out_hi, out_lo, ldo, precision, row_lens, stream);
}

// The one translation of the C argument block into the kernels' (ns2_kernels.h AttnArgs, whose defaults are "nothing optional").
// Everything ns2_attention_fwd refuses, it refuses here, before any HIP call; launch_attention judges the rest.
int ns2::attn_args_from(const ns2_attn_args* p, AttnArgs* out) {
  ARGCHK(p != nullptr, "ns2_attention_fwd: null argument block");
  ARGCHK(p->q_hi && p->k_hi && p->vt_hi && p->o_hi && prec_ok(p->precision), "ns2_attention_fwd: bad arguments");
  ARGCHK(p->head_dim == 0 || p->head_dim == 32 || p->head_dim == 64 || p->head_dim == 128, "ns2_attention_fwd: head_dim must be 32, 64 or 128 (0 = 64)");
  ARGCHK(p->o_precision == 0 || p->o_precision == 3 || p->o_precision == 4, "ns2_attention_fwd: o_precision 0 (= precision), 3 (bf16 hi / lo) or 4 (FMT_H8)");
  AttnArgs& a = *out;                                  // default-constructed by the caller
  a.D = p->head_dim ? p->head_dim : 64;
  ARGCHK(!p->lse || (p->precision == 3 && a.D == 64), "ns2_attention_fwd: lse needs precision 3 and head_dim 64 (what the backward kernels take)");
  ARGCHK(p->dropout_p == 0.f || p->lse, "ns2_attention_fwd: dropout needs lse (it belongs to the training forward)");
  if (const char* bad = set_attn_dropout(a, p->dropout_p, p->dropout_seed, p->dropout_call)) { set_error("ns2_attention_fwd: %s", bad); return NS2_ERR_ARG; }
  a.q_hi = p->q_hi; a.q_lo = p->q_lo; a.ldq = p->ldq; a.q_col0 = p->q_col0;
  a.k_hi = p->k_hi; a.k_lo = p->k_lo; a.ldk = p->ldk; a.k_col0 = p->k_col0;
  a.vt_hi = p->vt_hi; a.vt_lo = p->vt_lo; a.vt_ld = p->vt_ld;
  a.o_hi = p->o_hi; a.o_lo = p->o_lo; a.ldo = p->ldo;
  if (p->o_precision) a.o_fmt = operand_fmt(p->o_precision);
  a.B = p->B; a.H = p->H; a.Nq = p->Nq; a.Nk = p->Nk; a.scale = p->scale; a.kmask = p->key_mask; a.lse = p->lse;
  return NS2_OK;
}
extern "C" int ns2_attention_fwd(const ns2_attn_args* p, void* stream) {
  AttnArgs a;
  if (int rc = attn_args_from(p, &a)) return rc;
  HIPRET(launch_attention(a, p->precision, (hipStream_t)stream));
  return NS2_OK;
}

// with key counts: what this entry refuses comes first, under its own name; the block itself is ns2_attention_fwd's
extern "C" int ns2_attention_fwd_lens(const ns2_attn_args* p, const int* key_lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_fwd_lens: null argument block");
  ARGCHK(key_lens != nullptr, "ns2_attention_fwd_lens: key_lens is null (ns2_attention_fwd is the call without lengths)");
  ARGCHK(!p->key_mask, "ns2_attention_fwd_lens: key_mask together with key_lens (one way of shortening the keys per call)");
  ARGCHK(!p->lse, "ns2_attention_fwd_lens: lse together with key_lens (the training forward takes no lengths)");
  ARGCHK(p->dropout_p == 0.f, "ns2_attention_fwd_lens: dropout together with key_lens (the training forward takes no lengths)");
  AttnArgs a;
  if (int rc = attn_args_from(p, &a)) return rc;
  a.klens = key_lens;
  HIPRET(launch_attention(a, p->precision, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int64_t ns2_debug_gemm_route_launches(int route) { return gemm_route_launches(route); }
// ... and with query lengths on top (ragged skipping)
extern "C" int ns2_attention_fwd_skip(const ns2_attn_args* p, const int* key_lens, const int* query_lens, void* stream) {
  ARGCHK(p != nullptr, "ns2_attention_fwd_skip: null argument block");
  ARGCHK(query_lens != nullptr, "ns2_attention_fwd_skip: query_lens is null (ns2_attention_fwd / _lens are the calls without them)");
  ARGCHK(p->Nq > 0 && (p->Nq & 255) == 0, "ns2_attention_fwd_skip: Nq must be a positive multiple of 256 (whole skipping granules per utterance)");
  ARGCHK(!p->key_mask && !p->lse && p->dropout_p == 0.f, "ns2_attention_fwd_skip: key_mask, lse and dropout exclude query lengths (the plain inference forward)");
  AttnArgs a;
  if (int rc = attn_args_from(p, &a)) return rc;
  a.klens = key_lens; a.qlens = query_lens;
  HIPRET(launch_attention(a, p->precision, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_rmsnorm(const float* x, int ldx, int M, int d, int seq_len, const float* gamma, const float* cond, int cond_ld,
                           uint16_t* out_hi, uint16_t* out_lo, int ldo, float* out_f32, int ldo_f, int precision, void* stream) {
  ARGCHK(x && (out_hi || out_f32) && prec_ok(precision), "ns2_rmsnorm: bad arguments");
  ARGCHK(precision != 2 || !out_lo, "ns2_rmsnorm: precision 2 (fp16) has no lo plane");
  ARGCHK(!cond || seq_len > 0, "ns2_rmsnorm: adaptive norm needs seq_len");
  NormArgs n;
  n.x = x; n.ldx = ldx; n.gamma = gamma; n.cond = cond; n.cond_ld = cond_ld;
  n.out_hi = out_hi; n.out_lo = out_lo; n.ldo = out_hi ? ldo : d; n.out_f = out_f32; n.ldo_f = ldo_f; n.fmt = operand_fmt(precision);
  n.M = M; n.d = d; n.seq_len = seq_len;
  HIPRET(launch_rmsnorm(n, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int64_t ns2_skinny_linear_workspace_bytes(int B, int K, int J) { return (int64_t)skinny_linear_workspace_bytes(B, K, J); }
extern "C" int ns2_skinny_linear(const float* in, int ld_in, const float* wt, const float* bias, float* out, int ld_out, int B,
                                 int K, int J, int act, void* workspace, int64_t workspace_bytes, void* stream) {
  ARGCHK(in && wt && out, "ns2_skinny_linear: null pointer");
  HIPRET(launch_skinny_linear(in, ld_in, wt, bias, out, ld_out, B, K, J, act, (float*)workspace,
                              workspace ? (size_t)workspace_bytes : 0, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_time_embed(const float* times, const float* freqs, const float* wt, const float* bias, float* feat_ws,
                              float* out, int ld_out, int B, int dim, int dt, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  ARGCHK(times && freqs && wt && feat_ws && out, "ns2_time_embed: null pointer");
  HIPRET(launch_time_embed(times, freqs, wt, bias, feat_ws, out, ld_out, B, dim, dt, (float*)workspace,
                           workspace ? (size_t)workspace_bytes : 0, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_embedding(const int64_t* ids, const float* table, float* out, int64_t n, int dim, int64_t pad_id, void* stream) {
  ARGCHK(ids && table && out && n > 0 && dim > 0, "ns2_embedding: bad arguments");
  HIPRET(launch_embedding(ids, table, out, (long)n, dim, (long)pad_id, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_transpose_f32(const float* in, int batch, int R, int C, float* out, void* stream) {
  ARGCHK(in && out, "ns2_transpose_f32: null pointer");
  HIPRET(launch_transpose_f32(in, batch, R, C, out, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_ddim_step(const float* audio, const float* model_out, float* out, const float* times, const float* times_next,
                             int B, int64_t per_batch, int objective, int schedule, float scale, void* stream) {
  ARGCHK(audio && model_out && out && times && times_next, "ns2_ddim_step: null pointer");
  ARGCHK(objective >= 0 && objective <= 2 && schedule >= 0 && schedule <= 2, "ns2_ddim_step: bad objective/schedule");
  DdimArgs a;
  a.audio = const_cast<float*>(audio); a.model_out = model_out; a.out = out; a.times = times; a.times_next = times_next;
  a.B = B; a.per_batch = (long)per_batch; a.objective = objective; a.schedule = schedule; a.scale = scale;
  HIPRET(launch_ddim(a, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_cfg_mix(const float* cond_out, const float* null_out, float* out, int64_t n, float cond_scale, void* stream) {
  ARGCHK(cond_out && null_out && out, "ns2_cfg_mix: null pointer");
  HIPRET(launch_cfg_mix(cond_out, null_out, out, (long)n, cond_scale, (hipStream_t)stream));
  return NS2_OK;
}

// the pitch extractor (pitch.hip): the checks and the launch of ns2_pitch_yin and ns2_pitch_yin_lens, under the caller's `name`;
// sample_lens = null for the former, device memory for the latter: nothing here reads it
static int pitch_yin(const char* name, const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max,
                     float threshold, float* f0, const int* sample_lens, void* stream) {
  ARGCHK_AS(name, B >= 1 && B <= 65535, "B must be in [1, 65535]");
  ARGCHK_AS(name, L >= 1, "L must be at least 1");
  ARGCHK_AS(name, sample_rate >= 1 && hop_length >= 1, "sample_rate and hop_length must be at least 1");
  ARGCHK_AS(name, tau_min >= 2 && tau_min < tau_max && tau_max <= PITCH_TAU_MAX, "the lags must satisfy 2 <= tau_min < tau_max <= 1024");
  ARGCHK_AS(name, threshold == threshold, "threshold is NaN");
  const int64_t T = 1 + L / hop_length;
  ARGCHK_AS(name, T <= 0x7fffffffLL, "too many frames");
  HIPRET(launch_pitch_yin(audio, B, (long)L, (long)T, sample_rate, hop_length, tau_min, tau_max, threshold, f0, (hipStream_t)stream, sample_lens));
  return NS2_OK;
}
extern "C" int ns2_pitch_yin(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max,
                             float threshold, float* f0, void* stream) {
  ARGCHK(audio && f0, "ns2_pitch_yin: null pointer");
  return pitch_yin("ns2_pitch_yin", audio, B, L, sample_rate, hop_length, tau_min, tau_max, threshold, f0, nullptr, stream);
}
extern "C" int ns2_pitch_yin_lens(const float* audio, int B, int64_t L, int sample_rate, int hop_length, int tau_min, int tau_max,
                                  float threshold, float* f0, const int* sample_lens, void* stream) {
  ARGCHK(audio && f0, "ns2_pitch_yin_lens: null pointer");
  ARGCHK(sample_lens, "ns2_pitch_yin_lens: sample_lens is null (ns2_pitch_yin is the call without lengths)");
  return pitch_yin("ns2_pitch_yin_lens", audio, B, L, sample_rate, hop_length, tau_min, tau_max, threshold, f0, sample_lens, stream);
}

extern "C" int ns2_seanet_prep(const float* x, int ldx, int in_prefix, const float* add, int ldadd, int B, int64_t T, int C, int elu,
                               int prefix, int im2col_k, uint16_t* out_hi, uint16_t* out_lo, int ldo, int precision, void* stream) {
  ARGCHK(x && out_hi && prec_ok(precision), "ns2_seanet_prep: bad arguments");
  HIPRET(launch_seanet_prep(x, ldx, in_prefix, add, ldadd, B, (long)T, C, elu, prefix, im2col_k, out_hi, out_lo, ldo,
                            operand_fmt(precision), (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_seanet_prep2(const float* x, int ldx, int in_prefix, int B, int64_t T, int C, int prefix, uint16_t* elu_hi,
                                uint16_t* elu_lo, int elu_ld, int elu_col0, int elu_cols, uint16_t* raw_hi, uint16_t* raw_lo, int raw_ld,
                                int raw_col0, int raw_cols, int precision, void* stream) {
  ARGCHK(x && (elu_hi || raw_hi) && prec_ok(precision), "ns2_seanet_prep2: bad arguments");
  HIPRET(launch_seanet_prep2(x, ldx, in_prefix, B, (long)T, C, prefix, elu_hi, elu_lo, elu_ld, elu_col0, elu_cols, raw_hi, raw_lo, raw_ld,
                             raw_col0, raw_cols, operand_fmt(precision), (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_seanet_conv_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int ci, int co, int k, int elu,
                                      const float* w, const float* bias, float* out, int64_t ldo, void* stream) {
  ARGCHK(x && w && out && B > 0 && T > 0 && ci > 0 && co > 0 && k > 0 && in_prefix >= 0, "ns2_seanet_conv_narrow: bad arguments");
  const hipError_t e = launch_seanet_conv_narrow(x, (long)ldx, in_prefix, B, (long)T, ci, co, k, elu, w, bias, out, (long)ldo,
                                                 (hipStream_t)stream);
  if (e == hipErrorNotReady) return NS2_UNAVAILABLE;
  HIPRET(e);
  return NS2_OK;
}
extern "C" int ns2_seanet_resblock_narrow(const float* x, int64_t ldx, int in_prefix, int B, int64_t T, int C, const float* w1p,
                                          const float* b1, const float* w2p, const float* wsp, const float* b2s, float* out, int64_t ldo,
                                          void* stream) {
  ARGCHK(x && w1p && b1 && w2p && wsp && b2s && out && B > 0 && T > 0 && C > 0 && in_prefix >= 0, "ns2_seanet_resblock_narrow: bad arguments");
  const hipError_t e = launch_seanet_resblock_narrow(x, (long)ldx, in_prefix, B, (long)T, C, w1p, b1, w2p, wsp, b2s, out, (long)ldo,
                                                     (hipStream_t)stream);
  if (e == hipErrorNotReady) return NS2_UNAVAILABLE;
  HIPRET(e);
  return NS2_OK;
}
extern "C" int ns2_seanet_unpad(const float* src, int64_t ld_src, int prefix, float* dst, int64_t ld_dst, int B, int64_t T, int C,
                                void* stream) {
  ARGCHK(src && dst && B > 0 && T > 0 && C > 0 && prefix >= 0, "ns2_seanet_unpad: bad arguments");
  HIPRET(launch_seanet_unpad(src, (long)ld_src, prefix, dst, (long)ld_dst, B, (long)T, C, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int64_t ns2_lstm_state_floats(int B, int H) { return (B > 0 && H > 0) ? (int64_t)lstm_state_floats(B, H) : 0; }
extern "C" int ns2_lstm_layer(const float* xproj, int64_t ld_x, const float* w_hh, const float* b_hh, float* state, int64_t state_floats,
                              const float* resid, int64_t ld_r, float* out, int64_t ld_o, int B, int64_t T, int H, void* stream) {
  ARGCHK(xproj && w_hh && b_hh && state && out, "ns2_lstm_layer: null pointer");
  ARGCHK(B > 0 && T > 0 && H > 0 && H <= 512 && (H % 4) == 0, "ns2_lstm_layer: hidden size must be a multiple of 4, at most 512");
  ARGCHK(state_floats >= 3 * (int64_t)B * H, "ns2_lstm_layer: state scratch too small (ns2_lstm_state_floats)");
  float* h_a = state;                                  // caller-owned scratch (h ping, h pong, c | h exchange + step barrier)
  float* h_b = state + (size_t)B * H;
  float* c = state + 2 * (size_t)B * H;
  HIPRET(launch_lstm_layer(xproj, (long)ld_x, w_hh, b_hh, h_a, h_b, c, (long)state_floats, resid, (long)ld_r, out, (long)ld_o, B,
                           (long)T, H, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int64_t ns2_lstm2_state_floats(void) { return (int64_t)lstm2_state_floats(); }
extern "C" int ns2_lstm2(const float* xproj1, int64_t ld_x, const float* w_hh1, const float* b_hh1, const float* w_ih2, const float* b_ih2,
                         const float* w_hh2, const float* b_hh2, float* state, int64_t state_floats, const float* resid, int64_t ld_r,
                         float* out, int64_t ld_o, int B, int64_t T, void* stream) {
  ARGCHK(xproj1 && w_hh1 && b_hh1 && w_ih2 && b_ih2 && w_hh2 && b_hh2 && state && out, "ns2_lstm2: null pointer");
  ARGCHK(B > 0 && T > 0, "ns2_lstm2: empty batch or sequence");
  ARGCHK(state_floats >= (int64_t)lstm2_state_floats(), "ns2_lstm2: state scratch too small (ns2_lstm2_state_floats)");
  const hipError_t e = launch_lstm2(xproj1, (long)ld_x, w_hh1, b_hh1, w_ih2, b_ih2, w_hh2, b_hh2, state, (long)state_floats, resid, (long)ld_r,
                                    out, (long)ld_o, B, (long)T, (hipStream_t)stream);
  if (e == hipErrorNotReady) return NS2_UNAVAILABLE;
  HIPRET(e);
  return NS2_OK;
}

// The range guard's entry points loop over the registered counters; a registration that did not fit is an error the caller sees.
#define SAT_FULL_MSG "more translation units registered a range counter than SAT_COUNTERS_MAX holds"
extern "C" int ns2_saturation_count(int reset, int64_t* count) {
  ARGCHK(count != nullptr, "ns2_saturation_count: null pointer");
  int n = 0;
  const SatCounter* regs = sat_counters(&n);
  ARGCHK(regs != nullptr, "ns2_saturation_count: " SAT_FULL_MSG);
  HIPRET(hipDeviceSynchronize());                    // a diagnostic read between sampling runs, never on a launch path
  int64_t tot = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned int p = regs[i].read(reset != 0);
    ARGCHK(p != ~0u, "ns2_saturation_count: could not read the device counter");
    tot += p;
  }
  *count = tot;
  return NS2_OK;
}
extern "C" int ns2_saturation_counters(void) {
  int n = 0;
  return sat_counters(&n) ? n : -1;
}
extern "C" const char* ns2_saturation_counter_name(int i) {
  int n = 0;
  const SatCounter* regs = sat_counters(&n);
  if (!regs || i < 0 || i >= n) return nullptr;
  const char* slash = strrchr(regs[i].file, '/');
  return slash ? slash + 1 : regs[i].file;
}
extern "C" int ns2_saturation_peek(unsigned int* host, int capacity, void* stream) {
  ARGCHK(host != nullptr, "ns2_saturation_peek: null pointer");
  int n = 0;
  const SatCounter* regs = sat_counters(&n);
  ARGCHK(regs != nullptr, "ns2_saturation_peek: " SAT_FULL_MSG);
  ARGCHK(capacity >= n, "ns2_saturation_peek: fewer words than registered counters (ns2_saturation_counters)");
  for (int i = 0; i < n; ++i) HIPRET(regs[i].peek(host + i, (hipStream_t)stream));
  return NS2_OK;
}

extern "C" int ns2_debug_lstm_inject_abort(int n) {
  ARGCHK(n >= 0, "ns2_debug_lstm_inject_abort: negative count");
  HIPRET(hipDeviceSynchronize());
  HIPRET(lstm_abort_inject((unsigned int)n));
  return NS2_OK;
}
extern "C" int ns2_lstm_abort_count(int reset, int64_t* count) {
  ARGCHK(count != nullptr, "ns2_lstm_abort_count: null pointer");
  HIPRET(hipDeviceSynchronize());
  const unsigned int v = lstm_abort_read(reset != 0);
  ARGCHK(v != ~0u, "ns2_lstm_abort_count: could not read the device counter");
  *count = v;
  return NS2_OK;
}

extern "C" int ns2_rvq_prepare(const float* codebooks, float* cb_norm, int Q, int C, int D, void* stream) {
  ARGCHK(codebooks && cb_norm, "ns2_rvq_prepare: null pointer");
  HIPRET(launch_rvq_prepare(codebooks, cb_norm, Q, C, D, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_rvq_encode(const float* x, const float* codebooks, const float* cb_norm, int64_t* codes, float* emb,
                              float* residual, int* near_tie_count, int M, int Q, int C, int D, float tie_eps, void* stream) {
  ARGCHK(x && codebooks && cb_norm && codes, "ns2_rvq_encode: null pointer");
  ARGCHK(D == 128 && C % 64 == 0, "ns2_rvq_encode: needs codebook_dim 128 and codebook_size % 64 == 0 (EnCodec: 128 / 1024)");
  RvqArgs a;
  a.x = x; a.codebooks = codebooks; a.cb_norm = cb_norm; a.codes = codes; a.emb = emb; a.residual = residual;
  a.near_tie_count = near_tie_count; a.M = M; a.Q = Q; a.C = C; a.D = D; a.tie_eps = tie_eps;
  HIPRET(launch_rvq_encode(a, (hipStream_t)stream));
  return NS2_OK;
}
extern "C" int ns2_rvq_decode(const int64_t* codes, const float* codebooks, float* emb, int M, int Q, int C, int D, void* stream) {
  ARGCHK(codes && codebooks && emb, "ns2_rvq_decode: null pointer");
  HIPRET(launch_rvq_decode(codes, codebooks, emb, M, Q, C, D, (hipStream_t)stream));
  return NS2_OK;
}
