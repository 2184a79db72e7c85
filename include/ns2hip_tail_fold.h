/* The Wavenet tail fold and the wide RMSNorm kernel in libns2hip.  Part of the C ABI: listed in _lib.HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).  Status codes and ns2_last_error are those of ns2hip.h, which this header includes.
 *
 * Wavenet ends in `final_conv(sum of the blocks' skip convs)` (NS2:639-640, 685-686, 725): a Conv1d(dim, dim, 1) directly behind a sum of
 * L Conv1d(dim, dim, 1), i.e. a Linear behind a Linear over the L concatenated block outputs.  The pair is one Linear of K = L * dim:
 *   w_fold[n, l * dim + c] = sum_j w_final[n, j] w_skip[l][j, c]        b_fold[n] = sum_j w_final[n, j] (sum_l b_skip[l][j]) + b_final[n]
 * ns2_model_finalize folds once, from the fp32 parameters, and packs w_fold in the model's plan format; ns2_model_forward* then run ONE
 * product from the last stack's planes into the residual stream (like every other update of it: the RMSNorm that follows runs behind it,
 * or inside it where the product splits K), and neither the packed skip / final weights nor the skip sum's planes exist.  Results are a
 * reassociation of the same linear algebra, not the same bits.  The training pass keeps its two products.
 * Profiling (ns2_model_profile_begin): the folded product writes fp32 (gemm<f32 epilogue>) but is timed under category bit 1, where the skip
 * sum was: bench.py credits that category with the skip sum's 2 M dim L dim FLOPs, which are the FLOPs this product multiplies.  With the
 * fold on, category 1 therefore holds one fp32-epilogue launch per step beside the Wavenet's init conv. */
#ifndef NS2HIP_TAIL_FOLD_H
#define NS2HIP_TAIL_FOLD_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fold on the device: w_final [dim, dim], w_skip [layers, dim, dim], b_skip [layers, dim], b_final [dim] or NULL ->
 * w_fold [dim, layers * dim] (ns2_weight_pack(w_fold, dim, layers * dim, 1, ..) packs it), b_fold [dim]; all fp32 device memory.  fp32 FMAs
 * over ascending j (the bias sum over ascending l first), one accumulator per output, no atomics: bit-identical from run to run. */
int ns2_tail_fold(const float* w_final, const float* w_skip, const float* b_skip, const float* b_final, int dim, int layers, float* w_fold,
                  float* b_fold, void* stream);

/* test hook: 1 = fold (the default), 0 = the skip sum and final_conv stay two products -- bit for bit what the library computed before it
 * folded.  Read by ns2_model_finalize (a model keeps what it was finalized with) and by ns2_debug_chain_rule / ns2_debug_skip_rule;
 * process-wide like the hooks of ns2hip.h; NS2_TAIL_FOLD in the environment sets the initial value. */
int ns2_debug_force_tail_fold(int fold);

/* test hook of ns2_rmsnorm and of every RMSNorm a model launches: 0 = by shape (the default): rmsnorm_wide_kernel for the hot case -- d a
 * multiple of 256 up to 1024, ldo == d, FMT_H8 / dense IEEE-half / interleaved bf16 planes, x, gamma, cond and the outputs 16-byte aligned,
 * cond_ld a multiple of 4, and (with cond) seq_len a multiple of 16 -- and rmsnorm_kernel for everything else; 1 = rmsnorm_kernel for every
 * call.  The two kernels give the same bits.  NS2_NORM in the environment sets the initial value.
 * ns2_debug_norm_last: the kernel the last RMSNorm launch of the process took: 1 = rmsnorm_kernel, 2 = rmsnorm_wide_kernel, 0 = none yet. */
int ns2_debug_force_norm(int kernel);
int ns2_debug_norm_last(void);

#ifdef __cplusplus
}
#endif
#endif
