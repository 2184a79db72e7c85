"""The `Aligner` under autograd (`train_backend="hip"`; aligner.py of the reference: AlignerNet's two conv stacks, the distances and their
softmax, the monotonic alignment search on the detached soft alignment) on the Functions of functions.py, in the exact arithmetic like the
conditioning encoders (encoder_pass.py).  The only route that hands the Aligner a gradient is the forward-sum / bin loss of
`NaturalSpeech2.text_forward_cond(..., return_aux_losses=True)` (NS2:1587-1602)."""
import torch

from .. import ops
from .functions import AlignAttnFn, GemmFn, ReluFn, _c
from .passes import TRAIN_PRECISIONS, training_pass

_EXACT = TRAIN_PRECISIONS["exact"]
MAX_PHONEMES, MAX_FRAMES, MAX_CHANNELS = 1024, 8192, 256          # the limits of ns2_align_attn / ns2_maximum_path / the loss kernels


def _stack(h, convs, seq_len):
    """k = 3 "same" conv (pad_left = 1), then ReLU -> 1 x 1 conv for every further layer (aligner.py:30-51); h [b seq_len, c] fp32"""
    for i, c in enumerate(convs):
        if i:
            h = ReluFn.apply(_c(h))
        h = GemmFn.apply(_c(h), c.weight, c.bias, None, seq_len, 1, c.weight.shape[-1] // 2)    # (a 1 x 1 conv: one tap, no padding)
    return h


def aligner_forward_train(aligner, x, text_lens, y, mel_lens):
    """`Aligner.forward` with int lengths [b] on the device in place of the masks (no host read) as a differentiable graph: x [b, n, dim_hidden]
    phoneme encodings, y [b, dim_in, T] mel -> (aln_hard int32 [b, n], aln_soft [b, n, T], aln_log [b, 1, T, n], aln_mask [b, n, T]), as
    `Aligner.forward_lengths`.  Gradients reach the ten parameters, x, and y when it requires one."""
    net = aligner.aligner
    b, n, _ = x.shape
    T = y.shape[-1]
    text_lens = text_lens.to(device=x.device, dtype=torch.int32)
    mel_lens = mel_lens.to(device=x.device, dtype=torch.int32)
    with training_pass(_EXACT, x):
        keys = _stack(_c(x.float()).reshape(b * n, -1), [net.key_layers[i] for i in (0, 2)], n)
        queries = _stack(_c(y.float().transpose(1, 2)).reshape(b * T, -1), [net.query_layers[i] for i in (0, 2, 4)], T)
        log, soft = AlignAttnFn.apply(_c(queries), _c(keys), text_lens, b)
    if soft.is_cuda:
        path, hard = ops.maximum_path(soft.detach(), text_lens, mel_lens)
    else:                                                # a substitute backend on the CPU (the tests' emulation): the PyTorch search
        from ..aligner import create_mask
        from ..autograd_path import maximum_path_composite
        mask = create_mask(text_lens, n)[:, :, None] & create_mask(mel_lens, T)[:, None, :]
        path = maximum_path_composite(soft.detach(), mask.to(soft.dtype))
        hard = path.sum(-1).int()
    return hard, soft, log, path


def aligner_unsupported_reason(aligner, x=None, y=None, x_mask=None, y_mask=None):
    """None when `aligner_forward_train` can run `aligner` (on these inputs, where given), else why not: the caller falls back to the
    composite, as `Model`, the encoders and the predictor do.  Masks are checked for being prefix masks (one host read each), which is
    why the sync-free callers pass lengths and no masks."""
    for name, p in aligner.named_parameters():
        if p.dtype != torch.float32:
            return f"parameter {name} is {p.dtype} (fp32 master weights are required)"
    if aligner.attn_channels > MAX_CHANNELS:
        return f"attn_channels={aligner.attn_channels} (the distance kernels take at most {MAX_CHANNELS} channels)"
    if x is not None and x.shape[1] > MAX_PHONEMES:
        return f"n={x.shape[1]} phonemes (the alignment kernels take at most {MAX_PHONEMES})"
    if y is not None and y.shape[-1] > MAX_FRAMES:
        return f"T={y.shape[-1]} mel frames (the alignment kernels take at most {MAX_FRAMES})"
    from ..aligner import prefix_lengths
    for name, m in (("x_mask", x_mask), ("y_mask", y_mask)):
        if m is not None and prefix_lengths(m) is None:
            return f"{name} is not a prefix mask (the kernels take lengths)"
    return None
