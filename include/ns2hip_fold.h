/* The feed-forward fold in libns2hip.  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  Status codes
 * and ns2_last_error are those of ns2hip.h, which this header includes.
 *
 * FeedForward is Sequential(Linear(dim, 2f), GEGLU(), CausalConv1d(f, f, 3), Linear(f, dim)) (NS2:1009-1025).  Nothing stands between
 * the causal conv and the last Linear and both are linear maps, so the pair is one causal conv of kernel 3 from f to dim channels:
 *   w_fold[n, c, t] = sum_j w_out[n, j] w_conv[j, c, t]          b_fold[n] = sum_j w_out[n, j] b_conv[j] + b_out[n]
 * exactly, the zero frames in front of an utterance included (the padded input is the same).  A step then multiplies 2 M 3f dim
 * instead of 2 M f (3f + dim) per layer and the conv's output never exists.  ns2_model_finalize folds every layer once, from the fp32
 * parameters, and packs w_fold in the format of the conv site of the model's precision plan; ns2_model_forward* run the folded conv
 * (+ bias + residual) in that site's arithmetic.  Results are a reassociation of the same linear algebra, not the same bits. */
#ifndef NS2HIP_FOLD_H
#define NS2HIP_FOLD_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fold of one layer on the device: w_out [dim, f], w_conv [f, f, 3], b_conv [f], b_out [dim] or NULL -> w_fold [dim, f, 3]
 * (Conv1d's layout: ns2_weight_pack(w_fold, dim, f, 3, ..) packs it), b_fold [dim]; all fp32 device memory.  fp32 FMAs over ascending
 * j, one accumulator per output, no atomics: bit-identical from run to run.
 * ns2_linear with such a weight packed at precision 2 and tiled by ns2_weight_tile_conv3 takes the dedicated conv kernel
 * (csrc/ffconv_kernel.h) for an fp32 output as well -- out_f32 and resid 16-byte aligned, ldo_f and ldr multiples of 4, and the
 * conditions ns2hip.h lists for the plane output -- bit-identical to the general kernel. */
int ns2_ff_fold(const float* w_out, const float* w_conv, const float* b_conv, const float* b_out, int dim, int f, float* w_fold,
                float* b_fold, void* stream);

/* test hook: 1 = fold (the default), 0 = the conv and FF-out stay two products -- bit for bit what the library computed before it
 * folded.  Read by ns2_model_finalize (a model keeps what it was finalized with) and by ns2_debug_chain_rule; process-wide like the
 * hooks of ns2hip.h; NS2_FOLD in the environment sets the initial value. */
int ns2_debug_force_fold(int fold);

#ifdef __cplusplus
}
#endif
#endif
