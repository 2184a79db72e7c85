/* Head dims 32 and 128 in the TRAINING pass of libns2hip: the attention forward with its log-sum-exp, the delta reduction and the
 * flash backward for heads of 32, 64 or 128 columns.  Part of the C ABI: listed in _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).
 * Status codes, ns2_last_error, ns2_attn_args and ns2_attn_bwd_args are those of ns2hip.h, which this header includes.
 *
 * The entries of ns2hip.h and ns2hip_ragged_train.h keep their head dim of 64 (ns2_attention_fwd refuses lse at any other).  These take
 * the head dim as an argument: head h lies at columns col0 + head_dim * h of every operand, output and gradient, and `scale` is the
 * caller's (head_dim ** -0.5 for the reference's attention).  With head_dim 64 (or 0) each launches the very kernels of its counterpart:
 * the same bits.  The arithmetic is that of head dim 64 throughout: precision 3 operands (bf16 hi / lo lines, hi*hi + hi*lo + lo*hi), a
 * fixed summation order, no atomics; o and the gradient planes leave in bf16 hi / lo lines or FMT_H8 lines (o_precision / gp_precision).
 *
 * Every refusal below is NS2_ERR_ARG and is made before any device call. */
#ifndef NS2HIP_HEAD_DIM_TRAIN_H
#define NS2HIP_HEAD_DIM_TRAIN_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the training forward (args->lse required, precision 3) at args->head_dim 32, 64 or 128 (0 = 64); lens NULL, or int32 [B] on the
 * device = ns2_attention_train_fwd_lens's contract (then no key_mask / dropout, Nq == Nk) */
int ns2_attention_train_fwd_hd(const ns2_attn_args* args, const int* lens, void* stream);
/* ns2_attention_delta with heads of head_dim columns */
int ns2_attention_delta_hd(const float* d_out, int64_t ld_dout, const uint16_t* o_hi, const uint16_t* o_lo, int ldo, int B, int H, int Nq,
                           int head_dim, float* delta, int o_precision, void* stream);
/* ns2_attention_bwd / ns2_attention_bwd_lens with head h at columns col0 + head_dim * h; scale is the caller's (head_dim ** -0.5) */
int ns2_attention_bwd_hd(const ns2_attn_bwd_args* args, int head_dim, const int* lens, void* stream);

#ifdef __cplusplus
}
#endif
#endif
