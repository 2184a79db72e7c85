"""Training path of `Model`: forward + backward of the denoiser in the HIP kernels of libns2hip.

Reference call sites: `pred = self.model(noised_audio, times, prompt = prompt, cond = cond)` under autograd (NS2:1635), the
v-target MSE with min-SNR weight (NS2:1637-1666), `accelerator.backward(loss)` (NS2:1886).

How it is cut.  The differentiable graph consists of a handful of coarse `torch.autograd.Function`s whose boundaries are the
fp32 residual-stream tensors [B*N, dim] of the reference's forward (NS2:929-1000):

    GemmFn            nn.Linear / CausalConv1d / 1x1 conv (+ bias, + residual)                 NS2:583-595, 718-725
    WavenetBlockFn    dilated conv -> FiLM -> tanh*sigmoid gate, + res_conv                   NS2:597-642
    AttnFn            adaptive RMSNorm -> q, k, v -> attention -> to_out, + residual         NS2:1029-1069, 727-746, ATT:77-155
    FeedForwardFn     adaptive RMSNorm -> Linear -> GEGLU -> causal conv k3 -> Linear, + res  NS2:1004-1025
    NormLinearFn      RMSNorm(gamma) -> Linear                                                NS2:781-784

Inside a Function everything is a launch of libns2hip (`HipBackend`; C ABI: include/ns2hip.h "training"): activations
travel between the GEMMs as bf16 hi/lo operand planes, the backward contractions are the FORWARD GEMM kernels on re-packed
weights (dgrad) and on transposed planes with a fixed-slot split-K (wgrad), attention backward is a flash kernel that recomputes
P from the forward's log-sum-exp.  Arithmetic: precision 3 ("exact", bf16 x3 products, fp32 accumulate) whatever inference
precision the `Model` was built with -- gradients match the reference's fp32 autograd to ~1e-5.

Rows = batch entries: every conditioning Linear ([B, dim_cond] -> [B, 2 dim] for FiLM / adaptive norms, `to_time_cond.1`,
`to_prompt_cond.1`: NS2:623, 744, 841, 860) is `SkinnyLinearFn` -- the fp32 weight-streaming kernel of the inference path in all
three roles (y = x W^T + b, dx = dy W, dW = dy^T x).  What stays in PyTorch ops are pointwise glue on [B, *] rows (sin / cos of the
time embedding, SiLU, cat, mean-pool, `torch.where` null selects) and `torch.cat` of the
PerceiverResampler's context (NS2:1060-1061).  Autograd chains them with the Functions above; since round 5 the 32-token resampler
of the conditioned model (NS2:532-579) runs on the same Functions (`_resampler`), so no contraction of `Model`'s backward is a torch op.

The conditioning encoders (`Transformer`, `PhonemeEncoder`, `SpeechPromptEncoder` with `train_backend="hip"`; NS2:228-341, 1073-1115,
trained jointly: NS2:1538-1543) run on the same Functions -- `transformer_forward_train`, `phoneme_encoder_forward_train`,
`speech_prompt_encoder_forward_train`: `AttnFn` / `FeedForwardFn` with a learned-gamma RMSNorm in front,
key-padding mask and dropout in the attention forward / backward (csrc/dropout_keep.h), `GemmFn(pad_left=)` for the "same" k = 9
convolutions, `SiluFn`, `EmbeddingFn`; exact arithmetic only.  The `DurationPitchPredictor` (`train_backend="hip"`;
NS2:344-527) adds `GroupNormSiluFn`, `RowDotReluFn` and the `resid` operand of `AttnFn`: `duration_pitch_forward_train`.  The `Aligner`
(`train_backend="hip"`; aligner.py) adds `ReluFn` and `AlignAttnFn`: `aligner_forward_train` (aligner_pass.py); its two losses are
Functions of their own in aligner.py (`ForwardSumLoss` / `BinLoss` with `backend="hip"`).  The RVQ cross-entropy term of the loss
(`codec.rq`, `ResidualVQCrossEntropy(backend="hip")`; NS2:1668-1684) is `RvqCrossEntropyFn`: one launch, fp32 under either arithmetic.

Ragged batches (`Model(ragged_training=True)`, `model_forward_train(..., lens=)`; include/ns2hip_train.h): with
per-utterance frame counts -- int32 [B] on the device, read by kernels alone -- utterance i contributes to the output and to every gradient
what it contributes alone at lens[i] frames.  Rows of x and of the projected cond from a length on are selected to 0 at the entry, every
self-attention `AttnFn` gets `lens` (`HipBackend.attention(..., lens=)` / `attention_bwd(..., lens=)`: the length-aware instantiations of
the training forward and of the backward kernel, which write exact zeros from the length on), and the returned rows from a length on are
selected to 0, which zeroes the cotangent there.  Every gradient row of the padding is then an exact 0, so the weight-gradient GEMMs,
the bias sums and the FiLM partial sums need no lengths.  With `Model(ragged_skip_training=True)` and n % 256 == 0 they get them all the
same (include/ns2hip_train.h): `model_pass.py` hands the lengths down as the trailing optional argument of
`GemmFn`, `WavenetBlockFn`, `AttnFn`, `FeedForwardFn` and `NormLinearFn`, whose products over the b n frame rows pass `row_lens=` to
`HipBackend.gemm_f32` / `gemm_split` / `wgrad_rows`: hidden 256-row tiles are not computed and come back as zero bits, hidden K tiles
of a weight gradient are stepped over -- the same loss, rows and gradients, bit for bit.

Head dims 32 and 128 (`head_dim_training=True` on `Model`, `compat.HipBackedModel`, `Transformer`, the encoders, `DurationPitchPredictor`;
include/ns2hip_train.h): the three `*_unsupported_reason` functions then accept `dim_head` 32 and 128, and the passes
hand `dim_head` to every `AttnFn` (`functions.attn_apply`), which hands it to `HipBackend.attention*` only when it is not 64.  Without the
switch such a module trains on the composite, as before.

`Backend` is the seam the CPU tests use: `tests/emu_backend.py` restates every backend call with plain torch ops on CPU, so the
chain rule, tap flips, shifts and layouts of THIS package are checked against torch autograd without a GPU; the kernels behind
`HipBackend` are checked one by one and end to end on the MI355X (`tests/test_backward_gpu.py`).

Where things are; each module imports only from those before it: packs.py (the packed-weight cache), backend.py (`TPlanes`, `HipBackend`),
passes.py (what "the current pass" is: `training_pass`, `backend()` and its registries, `weights_unchanged`, the loss scale `_Scale`),
functions.py (the autograd Functions), model_pass.py / encoder_pass.py / duration_pitch_pass.py / aligner_pass.py (the `*_forward_train` of `Model`, of the
conditioning encoders, of the predictor and of the aligner), graph.py (`GraphedTrainStep`, on passes.py alone), optim.py (`HipAdam`: clip, Adam and EMA
as one capturable step, csrc/optim.hip; on _lib alone), trainer.py (`Trainer`, the reference's loop over graph.py and optim.py).  The names below are the package's interface; tests and tools take an
underscore name from the module that holds it.
"""
from .aligner_pass import aligner_forward_train, aligner_unsupported_reason
from .backend import HipBackend, TPlanes
from .duration_pitch_pass import duration_pitch_forward_train, duration_pitch_unsupported_reason
from .encoder_pass import (encoder_unsupported_reason, phoneme_encoder_forward_train, speech_prompt_encoder_forward_train,
                           transformer_forward_train)
from .graph import GraphedTrainStep
from .model_pass import available, model_forward_train, rvq_ce_unsupported_reason, unsupported_reason
from .optim import HipAdam
from .passes import TRAIN_PRECISIONS, backend, set_backend, weights_unchanged
from .trainer import Trainer

__all__ = ["HipBackend", "TPlanes", "aligner_forward_train", "aligner_unsupported_reason", "duration_pitch_forward_train", "duration_pitch_unsupported_reason", "encoder_unsupported_reason", "phoneme_encoder_forward_train", "speech_prompt_encoder_forward_train",
           "transformer_forward_train", "GraphedTrainStep", "HipAdam", "Trainer", "available", "model_forward_train", "rvq_ce_unsupported_reason", "unsupported_reason", "TRAIN_PRECISIONS",
           "backend", "set_backend", "weights_unchanged"]
