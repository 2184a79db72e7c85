// Host-side shared declarations of libns2hip (capi.cpp <-> model_exec.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/ns2hip.h"                // every source that defines entry points sees the whole model-side ABI
#include "../../include/ns2hip_frontend.h"
#include "../../include/ns2hip_audio.h"
#include "../../include/ns2hip_train.h"
#include "ns2_kernels.h"
#include "dropout_keep.h"

namespace ns2 {

void set_error(const char* fmt, ...);
void note_train_skip_launch();  // capi.cpp: a training product went out with lengths (ns2_debug_train_skip_launches)
void gemm_hook_changed();      // model_exec.cpp: ns2_debug_force_gemm was called (a cached verdict of the chain rule is stale)

// how an entry point gives up: a failed HIP call / a refused argument / a failed step -> the last error + the C ABI's code
#define HIPRET(expr)                                                                 \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      ns2::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return NS2_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
#define ARGCHK(cond, msg)            \
  do {                               \
    if (!(cond)) {                   \
      ns2::set_error("%s", msg);     \
      return NS2_ERR_ARG;            \
    }                                \
  } while (0)
// the same refusal from a check list that two entry points share: `name` is the entry's, so each keeps its own message prefix
#define ARGCHK_AS(name, cond, msg)           \
  do {                                       \
    if (!(cond)) {                           \
      ns2::set_error("%s: %s", name, msg);   \
      return NS2_ERR_ARG;                    \
    }                                        \
  } while (0)
#define NSCHK(expr)                  \
  do {                               \
    int _r = (expr);                 \
    if (_r != NS2_OK) return _r;     \
  } while (0)

// The dropout fields of a C argument block (ns2_attn_args / ns2_attn_bwd_args) -> the drop_* fields of the kernels' block (AttnArgs /
// AttnBwdArgs, whose defaults mean "none").  Returns what is wrong with them, or null.  p == 0: the seed is not read (may be null) and
// the kernels without dropout run.
template <class KernelArgs>
inline const char* set_attn_dropout(KernelArgs& a, float p, const uint32_t* seed, unsigned call) {
  if (!(p >= 0.f && p < 1.f)) return "dropout_p in [0, 1)";
  if (p == 0.f) return nullptr;
  if (!seed) return "dropout needs the seed words (device memory)";
  a.drop_seed = seed; a.drop_thr = drop_threshold(p); a.drop_call = call; a.drop_scale = 1.0f / (1.0f - p);
  return nullptr;
}

// capi.cpp: the one translation of ns2_attn_args into the kernels' block (default-constructed by the caller); refuses what
// ns2_attention_fwd refuses, before any HIP call.  Shared with capi_train.cpp (ns2_attention_train_fwd_lens).
int attn_args_from(const ns2_attn_args* p, AttnArgs* out);

struct PackedW {                 // bf16 split-plane weight, rows padded to 256, K contiguous
  bf16_t* hi = nullptr; bf16_t* lo = nullptr;
  int rows_p = 0, ldk = 0, N = 0, nkt = 0, kt_per_tap = 0;
  int fmt = 0;                   // PlaneFmt: bf16 planes (precisions 1 / 3), dense IEEE half (2), FMT_H8 lines (4)
  bf16_t* tl = nullptr;          // FMT_H8 linear weights: the tiled LDS images of the lean mixed linear kernel (gemm3_kernel.h), or null
  bf16_t* tw1 = nullptr; bf16_t* tw2 = nullptr;   // a Wavenet stack's FMT_H8 weights: tiled images of the lean block kernel (wavenet3_kernel.h), or null
  bf16_t* t3 = nullptr;          // k = 3 conv weights in dense IEEE half: the tiled LDS images of the dedicated FF-conv kernel (ffconv_kernel.h), or null
};

// One host path from a packed weight to launch_gemm, shared by capi.cpp and model_exec.cpp.  A caller takes gemm_args(), names the
// fields of ns2_kernels.h GemmArgs it uses (epilogue operands, outputs), and lets the setters below derive what only this layer knows.
// gemm_args: the weight, the activations and this thread's split-K scratch (model_exec.cpp SplitKScope) in an otherwise default block
GemmArgs gemm_args(const PackedW& w, const bf16_t* a_hi, const bf16_t* a_lo, int lda, int M);
inline void set_conv(GemmArgs& g, const PackedW& w, int taps, int dil, int seq_len) {
  g.kt_per_tap = w.kt_per_tap; g.conv_taps = taps; g.dil = dil; g.seq_len = seq_len;
}
inline void set_out_planes(GemmArgs& g, int epi, bf16_t* hi, bf16_t* lo, int ldo) {
  g.epi = epi; g.out_hi = hi; g.out_lo = lo; g.ldo_s = ldo; g.out_ncols = ldo;
}
// EPI_GEGLU: out_ncols = columns written (zeros beyond f); 0 = ldo
inline void set_geglu(GemmArgs& g, bf16_t* hi, bf16_t* lo, int ldo, int out_ncols = 0) {
  set_out_planes(g, EPI_GEGLU, hi, lo, ldo);
  if (out_ncols > 0) g.out_ncols = out_ncols;
}
// EPI_QKV: q | k (columns < split_col) are attention operands -- attention_fmt(prec), or att_fmt for both them and V^T when the
// caller's attention runs in another format; the values fill vt_rows = N - split_col rows per utterance of the transposed planes
inline void set_qkv(GemmArgs& g, int prec, int seq_len, int split_col, bf16_t* hi, bf16_t* lo, int ldo, int att_fmt = -1) {
  set_out_planes(g, EPI_QKV, hi, lo, ldo);
  g.seq_len = seq_len; g.split_col = split_col; g.out_ncols = split_col; g.vt_rows = g.N - split_col;
  g.out_fmt = att_fmt >= 0 ? att_fmt : attention_fmt(prec);
  if (att_fmt >= 0) g.vt_fmt = att_fmt;
}
// EPI_WAVENET: the dilated k = 3 conv, the gate at the K tile where the res conv's tap starts; nz > 1 steps through matrices laid back
// to back.  p1_half (the dilated conv as one half product) exists at precision 4 only.
inline void set_wavenet(GemmArgs& g, const PackedW& w, int dil, int seq_len, int prec, int p1_half) {
  set_conv(g, w, 3, dil, seq_len);
  g.epi = EPI_WAVENET; g.mid_kt = 3 * w.kt_per_tap; g.w_zs = (long)w.rows_p * w.ldk; g.p1_half = (prec == 4) ? p1_half : 0;
}

int pack_weight_public(const float* w, int rows, int cols, int taps, int geglu, const float* extra, int precision, PackedW* out,
                       std::vector<void*>* owned, hipStream_t s);
std::vector<int> geglu_row_map(int f, int rows_p);
int build_conv3_tiles(std::vector<void*>* owned, PackedW* w, hipStream_t s);   // model_exec.cpp: (re)build w->t3 from the row-major pack
int build_lin_tiles(std::vector<void*>* owned, PackedW* w, hipStream_t s);     // model_exec.cpp: (re)build w->tl (FMT_H8 packs; a no-op for other formats)

}  // namespace ns2

struct ns2_weight {
  ns2::PackedW w;
  int taps, geglu, has_extra, cols_p;
  int cols = 0;                  // source columns (per tap)
  int* d_map = nullptr;          // device copy of the row map the weight was packed with (ns2_weight_update re-packs in place)
  std::vector<void*> owned;
};
