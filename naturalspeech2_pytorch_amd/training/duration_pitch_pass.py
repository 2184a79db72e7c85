"""The `DurationPitchPredictor` under autograd (`train_backend="hip"`; NS2:344-527, its duration / pitch L1 terms: NS2:1578-1589) on the
Functions of functions.py, in the exact arithmetic like the conditioning encoders (encoder_pass.py)."""
import torch

from .functions import HEAD_DIMS_TRAIN, attn_apply, train_head_dim, EmbeddingFn, GemmFn, GroupNormSiluFn, RmsNormFn, RowDotReluFn, SiluFn, _c
from .passes import TRAIN_PRECISIONS, training_pass

_EXACT = TRAIN_PRECISIONS["exact"]


def _trunk_train(tr, h, prompts, b, n, drop, call0, head_dim=64):
    """one `DurationPitchPredictorTrunk` (NS2:456-466): h [b n, d] fp32, prompts [b, n_p, d] -> [b n].  `drop` = (p, seed) or None;
    the attention of layer i is dropout call `call0 + i`"""
    d, k = tr.dim, tr.kernel_size
    n_p = prompts.shape[1]
    for li, (convs, norm, attn) in enumerate(tr.layers):
        for blk in convs:
            if tr.use_resnet_block:                                   # ResnetBlock: h = Blocks(x); out = h + x (NS2:394-398)
                x_in, last = h, len(blk.blocks) - 1
                for j, bl in enumerate(blk.blocks):
                    h = GemmFn.apply(_c(h), bl.proj.weight, bl.proj.bias, None, n, 1, k // 2)
                    h = GroupNormSiluFn.apply(_c(h), bl.norm.weight, bl.norm.bias, x_in if j == last else None, n, bl.norm.num_groups,
                                              bl.norm.eps)
            else:                                                     # ConvBlock (NS2:402-409)
                h = SiluFn.apply(_c(GemmFn.apply(_c(h), blk[1].weight, blk[1].bias, None, n, 1, k // 2)))
        # attn(norm(x), prompts) + x with keys / values from cat(norm(x), prompts) (NS2:464, 1060-1061).  norm(x) is a tensor of the graph:
        # torch's cat hands the first n rows of the context gradient back to it, the rest to `prompts`
        xn = RmsNormFn.apply(_c(h), norm.gamma)
        ctxt = torch.cat((xn.reshape(b, n, d), prompts), dim=1).reshape(b * (n + n_p), d)
        h = attn_apply(xn, None, ctxt, attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, n, tr.heads, n + n_p, None, None,
                       (drop[0], drop[1], call0 + li) if drop is not None else None, _c(h), head_dim=head_dim)
    head = tr.to_pred[0]
    return RowDotReluFn.apply(_c(h), head.weight, head.bias)


def duration_pitch_forward_train(dp, x, prompts):
    """`DurationPitchPredictor.forward` (NS2:511-527) as a differentiable graph: x = token ids [b, n] or phoneme encodings [b, n, d],
    prompts [b, n_p, d] -> (duration, pitch), each [b, n].  Dropout as in the reference: the trunk hands `dropout` to its Attention only
    (NS2:430-446: the conv blocks keep their own default 0), so in train() mode it acts on the attention probabilities alone -- the stateless
    keep function of csrc/dropout_keep.h under one device-side seed per pass, call index = trunk * depth + layer.  `dp.dropout_seed`
    (an int64 tensor of one element) replaces the draw; `dp.last_dropout_seed` is what the last pass used."""
    trunks = (dp.to_duration_pred, dp.to_pitch_pred)
    with training_pass(_EXACT, prompts):
        if isinstance(dp.phoneme_token_emb, torch.nn.Embedding):
            b, n = x.shape
            h = EmbeddingFn.apply(x, dp.phoneme_token_emb.weight, 0)
            dtype = prompts.dtype
        else:
            b, n, _ = x.shape
            h = _c(x.float()).reshape(b * n, x.shape[-1])
            dtype = x.dtype
        pr = _c(prompts.float())
        p = float(dp.dropout) if dp.training else 0.
        drop = None
        if p > 0:
            seed = getattr(dp, "dropout_seed", None)
            if seed is None:
                seed = torch.empty(1, dtype=torch.int64, device=pr.device).random_()
            assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == pr.device
            dp.last_dropout_seed = seed
            drop = (p, seed)
        depth = len(trunks[0].layers)
        hd = train_head_dim(dp, trunks[0].dim_head)
        return tuple(_trunk_train(tr, h, pr, b, n, drop, ti * depth, hd).reshape(b, n).to(dtype) for ti, tr in enumerate(trunks))


def duration_pitch_unsupported_reason(dp):
    """None when `duration_pitch_forward_train` can run `dp`, else why not: the caller falls back to the composite, as `Model` and the
    encoders do"""
    tr = dp.to_pitch_pred
    if getattr(dp, "head_dim_training", False):
        if tr.dim_head not in HEAD_DIMS_TRAIN:
            return f"dim_head={tr.dim_head} (the HIP training attention kernels have head dims 32, 64 and 128)"
    elif tr.dim_head != 64:
        return f"dim_head={tr.dim_head} (the HIP attention backward kernels have a head dim of 64)"
    if tr.dim % 32:
        return f"dim_hidden={tr.dim} is not a multiple of 32"
    for name, p in dp.named_parameters():
        if p.dtype != torch.float32:
            return f"parameter {name} is {p.dtype} (fp32 master weights are required)"
    return None
