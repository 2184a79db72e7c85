/* Ragged batches in libns2hip: skipping the hidden row tiles of a TRAINING batch in the products.  Part of the C ABI: listed in
 * _lib.HEADERS (naturalspeech2_pytorch_amd/_lib.py).  Status codes, ns2_last_error, ns2_linear_args and ns2_weight are those of ns2hip.h, which this
 * header includes.
 *
 * ns2hip_ragged_train.h made a ragged training batch correct: the lengths go to the self-attention in both directions, every other
 * kernel computes every row.  ns2hip_ragged_skip.h skips the hidden row tiles of a SAMPLING step.  Here the lengths go to the three
 * product families of the training pass: the forward products, the dgrads and the weight gradients.  The granule is the one of
 * ns2hip_ragged_skip.h: for a batch [B, N] with N % 256 == 0 and device lengths lens (int32 [B], clamped by the kernels into [1, N])
 *
 *     H_i = min(N, 256 * ceil(lens_i / 256))
 *
 * and row r of utterance i is HIDDEN when r >= H_i.  Lengths are read by the kernels alone (through the scalar cache), never on the
 * host and never written: a launch captured into a HIP graph follows values rewritten between replays.
 *
 * What a hidden tile leaves behind differs from the sampling rule ("keeps what it held"), for two reasons: the buffers of the
 * training pass come uninitialised, and the dgrad of a causal conv is ANTICAUSAL -- the visible row H_i - 1 reads the rows behind it.
 * So A SKIPPING PRODUCT IN TRAINING WRITES ZERO BITS INTO THE HIDDEN TILES OF EVERY OUTPUT IT HAS: an fp32 output with or without a
 * residual, operand planes of either format, the attention's q | k | v lines, V^T.  Nothing in the pass then holds garbage, the
 * kernels that do not skip stay correct unchanged, and every reduction over tokens adds exact zeros where it added exact zeros
 * before (DESIGN section 9 walks the pass). */
#ifndef NS2HIP_RAGGED_SKIP_TRAIN_H
#define NS2HIP_RAGGED_SKIP_TRAIN_H

#include <stdint.h>
#include "ns2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ns2_linear_lens (include/ns2hip_ragged_skip.h) whose hidden row tiles are stored as zero bits in every output of the product;
 * rows before an utterance's computed extent have the bits ns2_linear gives.  Refused as ns2_linear_lens refuses: NS2_ERR_ARG,
 * before any device call, when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0, or when args->seq_len is set
 * and differs; whatever ns2_linear refuses is refused alike.  Every route ns2_linear can take a product down skips (the 128 x 128
 * kernel, the 256 x 256 kernel, the FF conv kernel, the lean linear kernel) except split K, which takes no lengths and computes
 * every row, as in ns2_linear_lens.
 * CONTRACT of an anticausal product (conv_taps > 1 with pad_left in [0, conv_taps - 1): the dgrad of a causal conv): a visible row
 * reads up to (conv_taps - 1 - pad_left) * dilation rows behind it, so the hidden rows of its operand must be ZEROS (what the
 * skipping products of the pass leave there, and what a cotangent holds behind a length).  A causal or plain product reads no hidden
 * row from a visible one: its operand's hidden rows may hold anything. */
int ns2_linear_lens_zero(const ns2_linear_args* args, const int* row_lens, int seq_len, void* stream);

/* ns2_wgrad_rows (include/ns2hip.h) on a ragged batch of M / seq_len utterances: a 32-token K tile whose tokens are all hidden is
 * neither fetched nor multiplied.  With seq_len % 256 == 0 a tile is hidden iff its first token is, and the causal taps of a visible
 * tile (token m - shift) read visible rows only.  The slice plan, the slots and the order of their sum are those of ns2_wgrad_rows
 * for the same M: a slot's sum only loses terms, and where the hidden rows of dY are zeros (the cotangent of a ragged pass) those
 * terms were exact zeros, so dW has the bits of ns2_wgrad_rows.  The hidden rows of dY and X may hold anything: they are not read.
 * Unlike ns2_wgrad_rows, seq_len is required for T = 1 too (it is the utterance stride of the lengths).  Refused (NS2_ERR_ARG, before
 * any device call) when row_lens is null, seq_len <= 0, seq_len % 256 != 0 or M % seq_len != 0; whatever ns2_wgrad_rows refuses is
 * refused alike.  Workspace: ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32)), as there. */
int ns2_wgrad_rows_lens(const uint16_t* dy_hi, const uint16_t* dy_lo, int ld_dy, const uint16_t* x_hi, const uint16_t* x_lo, int ld_x,
                        int64_t M, int R, int T, int Kp, int K, int dil, int seq_len, float* dw, void* workspace, int64_t workspace_bytes,
                        int precision, const int* row_lens, void* stream);

/* Test hook: launches the two entries above have sent WITH lengths so far in this process (a product that ns2_linear_lens_zero routed
 * to split K computed every row and is not counted).  Host arithmetic, no device-side counting: kernels with and without lengths may
 * give the same bits, so the tests read the counter around a pass. */
int64_t ns2_debug_train_skip_launches(void);

#ifdef __cplusplus
}
#endif
#endif
