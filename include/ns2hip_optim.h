/* libns2hip: the optimizer step of the training loop on the device.  Part of the C ABI: listed in _lib.HEADERS
 * (naturalspeech2_pytorch_amd/_lib.py).
 *
 * Reference: what follows `accelerator.backward(loss)` in Trainer.train (NS2:1888-1901) --
 * `clip_grad_norm_(parameters, max_grad_norm)`, `Adam.step()` (weight_decay 0, amsgrad off), `ema.update()` every
 * `update_every` steps -- as three stream-ordered launches with no host read, so the whole loop body can live in one HIP graph.
 *
 * The conventions of ns2hip.h hold (device pointers unless named host_*, caller-owned memory, 0 = ok, ns2_last_error()); this header
 * declares its own entry points, structs and constants only.
 *
 * Memory, all caller-owned:
 *   table   ns2_optim_table_bytes(n, chunks) bytes, 16-byte aligned: the tensors, their cut into chunks of NS2_OPTIM_CHUNK values
 *           (one workgroup each; a chunk never spans two tensors) and one fp32 partial sum of squares per chunk.
 *   state   NS2_OPTIM_STATE_WORDS 32-bit words, 16-byte aligned.  Word indices below; fp32 unless marked (int).  The caller may
 *           rewrite NS2_OPTIM_W_LR and NS2_OPTIM_W_EMA_DECAY between steps (a scheduler, an EMA warm-up: no recapture), and reads the
 *           others in stream order.  Words from NS2_OPTIM_W_PRIVATE on belong to the library (the range-guard snapshot).
 *
 * One step, ns2_optim_step:
 *   norm    every chunk writes the fp32 sum of squares of its gradients into its own slot; one workgroup adds the slots in fp64 in a
 *           fixed order: bit-reproducible, no atomics.  grad_norm = sqrt(sum), clip_coef = min(1, max_grad_norm / (grad_norm + 1e-6))
 *           (exactly 1 below max_grad_norm, and when max_grad_norm <= 0: clipping off).
 *   skip    1 when grad_norm is not finite, or when a range-guard counter (ns2_saturation_*) differs from the snapshot of the last
 *           ns2_optim_mark (never marked: the first test alone).  A skipped step writes nothing but grad_norm, clip_coef and skip:
 *           parameters, moments, EMA and the step count keep their bits.
 *   update  g *= clip_coef; m += (g - m)(1 - beta1); v = beta2 v + (1 - beta2) g^2; p -= step_size m / (sqrt(v) / bc2_sqrt + eps),
 *           step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) evaluated in fp64 for the new step count t; and, when
 *           ema_update_every > 0 and t is a multiple of it, ema += (1 - ema_decay)(p - ema) in the same pass.
 * A tensor whose grad is null takes no part in the norm or in Adam (torch.optim.Adam skips it too) but stays in the EMA.
 * Tensors start at any 4-byte aligned address; where param, grad, exp_avg, exp_avg_sq (and ema) of a tensor do not share their
 * address modulo 16 the tensor takes the 4-byte path, otherwise only its first and last up-to-3 values do. */
#ifndef NS2HIP_OPTIM_H
#define NS2HIP_OPTIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS2_OPTIM_CHUNK 4096
#define NS2_OPTIM_STATE_WORDS 128
#define NS2_OPTIM_W_GRAD_NORM 0
#define NS2_OPTIM_W_CLIP_COEF 1
#define NS2_OPTIM_W_SKIP 2       /* (int) the last step was skipped */
#define NS2_OPTIM_W_STEP 3       /* (int) steps taken */
#define NS2_OPTIM_W_STEP_SIZE 4
#define NS2_OPTIM_W_BC2_SQRT 5
#define NS2_OPTIM_W_EMA_DUE 6    /* (int) */
#define NS2_OPTIM_W_LR 7
#define NS2_OPTIM_W_EMA_DECAY 8
#define NS2_OPTIM_W_EMA_WEIGHT 9 /* 1 - ema_decay, evaluated in fp64 */
#define NS2_OPTIM_W_PRIVATE 10
#define NS2_OPTIM_GRADS_MAX 256  /* pointers per ns2_optim_set_grads call */

typedef struct {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* ema; /* grad, ema: may be null */
  int64_t numel;
} ns2_optim_tensor;

typedef struct {
  double beta1, beta2, eps;
  double max_grad_norm;      /* <= 0: no clipping */
  int ema_update_every;      /* <= 0: no EMA */
} ns2_optim_config;

/* chunks the n tensors of host_tensors are cut into (host arithmetic; negative: a bad argument) */
int64_t ns2_optim_chunks(const ns2_optim_tensor* host_tensors, int n);
int64_t ns2_optim_table_bytes(int n, int64_t chunks);
/* write the device table.  One-time set-up like ns2_weights_repack_build: synchronises, not capturable. */
int ns2_optim_table_build(const ns2_optim_tensor* host_tensors, int n, void* table, int64_t table_bytes, void* stream);
/* replace the grad pointers of tensors [first, first + count), count <= NS2_OPTIM_GRADS_MAX, from the host array: stream-ordered and
 * capturable (the pointers travel as launch arguments), for gradients that a backward pass allocates anew. */
int ns2_optim_set_grads(void* table, int n, int first, int count, const float* const* host_grads, void* stream);
/* initialise the state block: step count, lr, ema_decay, never marked, and the addresses of the current device's range-guard
 * counters.  Synchronises, not capturable. */
int ns2_optim_state_init(void* state, int step, float lr, float ema_decay, void* stream);
/* snapshot the range-guard counters into the state block, device to device: stream-ordered, capturable */
int ns2_optim_mark(void* state, void* stream);
/* norm, finish, update (see above): stream-ordered, capturable, no allocation */
int ns2_optim_step(void* table, int n, int64_t chunks, void* state, const ns2_optim_config* host_config, void* stream);

#ifdef __cplusplus
}
#endif
#endif
