"""The conditioning encoders under autograd (`Transformer`, `PhonemeEncoder`, `SpeechPromptEncoder` with `train_backend="hip"`) on the
Functions of functions.py.  They train in the exact arithmetic whatever the denoiser next to them uses: the gradient that reaches them
has left its scaled domain (`_ScaleOut` on prompt / cond in model_pass.py)."""
import torch
import torch.nn.functional as F

from .. import ops
from .functions import HEAD_DIMS_TRAIN, attn_apply, train_head_dim, EmbeddingFn, FeedForwardFn, GemmFn, KeepRowsFn, RmsNormFn, SiluFn, _c
from .passes import TRAIN_PRECISIONS, training_pass

_EXACT = TRAIN_PRECISIONS["exact"]


def _key_mask(mask, b, n):
    """bool [b, n] (True = attend) -> uint8 for the kernels.  An utterance with no valid key is rejected (the reference's softmax over a
    fully masked row is NaN); the check reads the mask back, so it is left to the warm passes when a graph is being captured."""
    if mask is None:
        return None
    if mask.dtype != torch.bool or tuple(mask.shape) != (b, n):
        raise ValueError(f"the key-padding mask must be boolean [b, n] = [{b}, {n}], got {mask.dtype} {tuple(mask.shape)}")
    capturing = mask.is_cuda and torch.cuda.is_current_stream_capturing()
    if not capturing and not bool(mask.any(dim=1).all()):
        raise ValueError("the key-padding mask leaves an utterance without a single valid key")
    return mask.to(torch.uint8).contiguous()


def lens_key_mask(lens, n):
    """the byte mask of keys [0, clamp(lens[i], 1, n)) of every utterance, uint8 [b, n], formed on the device from int32 lengths: no host read
    (`_key_mask`'s check has nothing to find: a clamped length always leaves one key), so a captured pass follows lengths rewritten between
    replays"""
    return (torch.arange(n, device=lens.device)[None] < lens.clamp(1, n)[:, None]).to(torch.uint8).contiguous()


def _transformer_train(tr, h, b, n, mask, km=None, row_lens=None):
    """km: a byte mask already made (`lens_key_mask`) instead of `mask`; row_lens: the int32 lengths it was made from -- the rows of h from a
    length on are zeros on entry and are selected to 0 again behind every layer (an attention's output for a padding query and a
    FeedForward's biases are finite but not 0), so every attention sees zero rows where its mask hides keys (`AttnFn` masked_rows_zero)"""
    d = tr.dim
    if km is None:
        km = _key_mask(mask, b, n)
    p = float(tr.dropout) if tr.training else 0.
    seed = None
    if p > 0:
        # one seed per pass, the layer index tells the attentions apart.  Drawn ON THE DEVICE by PyTorch's generator (graph-aware: a replay
        # of a captured pass draws anew) and read there by the kernels.  `tr.dropout_seed` (an int64 tensor of one element) replaces the
        # draw: reproducing a pass; `tr.last_dropout_seed` is what the last pass used.
        seed = getattr(tr, "dropout_seed", None)
        if seed is None:
            seed = torch.empty(1, dtype=torch.int64, device=h.device).random_()
        assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == h.device
        tr.last_dropout_seed = seed
    for li, (norm1, attn, norm2, ff) in enumerate(tr.layers):
        h = attn_apply(_c(h), None, None, attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, n, tr.heads, 0, norm1.gamma, km,
                       (p, seed, li) if p > 0 else None, head_dim=train_head_dim(tr, tr.dim_head), masked_rows_zero=row_lens is not None)
        l1, l2 = getattr(ff, "0"), getattr(ff, "2")
        h = FeedForwardFn.apply(_c(h), None, l1.weight, l1.bias, None, None, l2.weight, l2.bias, n, norm2.gamma)
        if row_lens is not None:
            h = KeepRowsFn.apply(h, n, row_lens)
    if hasattr(tr.norm, "gamma"):
        h = RmsNormFn.apply(_c(h), tr.norm.gamma)
    return h.reshape(b, n, d)


def transformer_forward_train(tr, x, mask=None):
    """`Transformer.forward` (NS2:1073-1115) as a differentiable graph on the Functions of functions.py: per layer RMSNorm(gamma) -> self attention
    (key-padding mask, dropout on P in training mode) + residual, RMSNorm(gamma) -> Linear -> GEGLU -> Linear + residual; final norm"""
    b, n, d = x.shape
    with training_pass(_EXACT, x):
        return _transformer_train(tr, _c(x.float()).reshape(b * n, d), b, n, mask).to(x.dtype)


def speech_prompt_encoder_forward_train(enc, x, lens=None):
    """`SpeechPromptEncoder.forward` (NS2:289-341): the "same" k = 9 convolutions as GEMMs with pad_left = padding, SiLU on the kept fp32
    pre-activation, then the Transformer.
    `lens` (`ragged_conditioning`; include/ns2hip_train.h): prompt rows per utterance, integer [b].  The input and every
    convolution's output are selected to 0 from lens[i] on (`KeepRowsFn`: the same select on the cotangent), so the "same" convolutions read
    what they read behind the end of the utterance alone; the Transformer runs under the key mask arange(n) < lens[:, None] on the existing
    key-mask / dropout kernels; the output rows from lens[i] on are selected to 0.  Nothing reads a device tensor of lengths on the host."""
    b, n, _ = x.shape
    with training_pass(_EXACT, x):
        h = _c(x.float()).reshape(b * n, enc.dim)
        if lens is None:
            for m in enc.conv:
                if isinstance(m, torch.nn.Conv1d):
                    h = SiluFn.apply(_c(GemmFn.apply(_c(h), m.weight, m.bias, None, n, 1, enc.padding)))
            return _transformer_train(enc.transformer, h, b, n, None).to(x.dtype)
        ln = ops._front_lens(lens, b, x.device)
        h = KeepRowsFn.apply(h, n, ln)
        for m in enc.conv:
            if isinstance(m, torch.nn.Conv1d):
                h = KeepRowsFn.apply(SiluFn.apply(_c(GemmFn.apply(_c(h), m.weight, m.bias, None, n, 1, enc.padding))), n, ln)
        out = _transformer_train(enc.transformer, h, b, n, None, km=lens_key_mask(ln, n), row_lens=ln)
        return KeepRowsFn.apply(_c(out).reshape(b * n, -1), n, ln).reshape(b, n, -1).to(x.dtype)


def phoneme_encoder_forward_train(enc, ids, mask=None, lens=None):
    """`PhonemeEncoder.forward` on token ids (NS2:228-287): embedding (padded ids -> pad_id), CausalConv1d k = 9 + SiLU, conv dropout
    (F.dropout on the fp32 activations: pointwise plumbing), then the Transformer under the key-padding mask.
    lens (instead of mask): phonemes per utterance, integer [b] on the device -- the byte mask is formed there (`lens_key_mask`: no host read)"""
    b, n = ids.shape
    with training_pass(_EXACT, ids):
        h = EmbeddingFn.apply(ids, enc.token_emb.weight, enc.pad_id)
        conv = enc.conv[1]
        h = SiluFn.apply(_c(GemmFn.apply(_c(h), conv.weight, conv.bias, None, n, 1)))
        h = F.dropout(h, enc.conv_dropout, enc.training)
        if lens is not None:
            assert mask is None
            ln = ops._front_lens(lens, b, ids.device)
            return _transformer_train(enc.transformer, KeepRowsFn.apply(h, n, ln), b, n, None, km=lens_key_mask(ln, n), row_lens=ln)
        return _transformer_train(enc.transformer, h, b, n, mask)


def encoder_unsupported_reason(module, mask=None):
    """None when the `*_forward_train` functions above can run `module` (a `Transformer`, `PhonemeEncoder` or `SpeechPromptEncoder`) with
    this key mask, else why not -- the counterpart of `unsupported_reason` for `Model`: the caller falls back to the composite"""
    tr = getattr(module, "transformer", module)
    if getattr(tr, "head_dim_training", False):
        if tr.dim_head not in HEAD_DIMS_TRAIN:
            return f"dim_head={tr.dim_head} (the HIP training attention kernels have head dims 32, 64 and 128)"
    elif tr.dim_head != 64:
        return f"dim_head={tr.dim_head} (the HIP attention backward kernels have a head dim of 64)"
    if tr.dim % 32:
        return f"dim={tr.dim} is not a multiple of 32"
    if tr.causal:
        return "causal=True (the training attention kernels are non-causal)"
    for name, p in module.named_parameters():
        if p.dtype != torch.float32:
            return f"parameter {name} is {p.dtype} (fp32 master weights are required)"
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.ndim != 2):
        return "the key-padding mask is not a boolean [b, n] tensor"
    return None
