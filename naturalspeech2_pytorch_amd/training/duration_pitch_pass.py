"""The `DurationPitchPredictor` under autograd (`train_backend="hip"`; NS2:344-527, its duration / pitch L1 terms: NS2:1578-1589) on the
Functions of functions.py, in the exact arithmetic like the conditioning encoders (encoder_pass.py)."""
import torch

from .. import ops
from .functions import (HEAD_DIMS_TRAIN, attn_apply, train_head_dim, EmbeddingFn, GemmFn, GroupNormSiluFn, KeepRowsFn, RmsNormFn, RowDotReluFn,
                        SiluFn, _c)
from .passes import TRAIN_PRECISIONS, training_pass

_EXACT = TRAIN_PRECISIONS["exact"]


def _trunk_train(tr, h, prompts, b, n, drop, call0, head_dim=64, text_lens=None, key_mask=None, ctx_order=None):
    """one `DurationPitchPredictorTrunk` (NS2:456-466): h [b n, d] fp32, prompts [b, n_p, d] -> [b n].  `drop` = (p, seed) or None;
    the attention of layer i is dropout call `call0 + i`.
    text_lens: int32 [b] on the device or None -- the rows of h from text_lens[i] on are zeros on entry and after every block: a
    ResnetBlock's GroupNorm takes them as its row counts (statistics and gradient sums of the utterance's own phonemes; it writes zeros
    behind them), a ConvBlock's and the attention's output are selected to 0 there (the k // 2 "same" convs look ahead, and a padding query's
    output is finite but not 0).  key_mask: uint8 [b, n + n_p] or None, the keys of every attention.  ctx_order: int64 [b, n + n_p, d] or
    None -- the rows of cat(norm(x), prompts) every attention gathers its context by (`duration_pitch_forward_train`); key_mask then
    describes the gathered rows"""
    d, k = tr.dim, tr.kernel_size
    n_p = prompts.shape[1]
    gn_tail = () if text_lens is None else (text_lens,)
    for li, (convs, norm, attn) in enumerate(tr.layers):
        for blk in convs:
            if tr.use_resnet_block:                                   # ResnetBlock: h = Blocks(x); out = h + x (NS2:394-398)
                x_in, last = h, len(blk.blocks) - 1
                for j, bl in enumerate(blk.blocks):
                    h = GemmFn.apply(_c(h), bl.proj.weight, bl.proj.bias, None, n, 1, k // 2)
                    h = GroupNormSiluFn.apply(_c(h), bl.norm.weight, bl.norm.bias, x_in if j == last else None, n, bl.norm.num_groups,
                                              bl.norm.eps, *gn_tail)
            else:                                                     # ConvBlock (NS2:402-409)
                h = SiluFn.apply(_c(GemmFn.apply(_c(h), blk[1].weight, blk[1].bias, None, n, 1, k // 2)))
                if text_lens is not None:
                    h = KeepRowsFn.apply(h, n, text_lens)
        # attn(norm(x), prompts) + x with keys / values from cat(norm(x), prompts) (NS2:464, 1060-1061).  norm(x) is a tensor of the graph:
        # torch's cat hands the first n rows of the context gradient back to it, the rest to `prompts`
        xn = RmsNormFn.apply(_c(h), norm.gamma)
        ctxt = torch.cat((xn.reshape(b, n, d), prompts), dim=1)
        if ctx_order is not None:
            ctxt = torch.gather(ctxt, 1, ctx_order)
        ctxt = _c(ctxt).reshape(b * (n + n_p), d)
        h = attn_apply(xn, None, ctxt, attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, n, tr.heads, n + n_p, None, key_mask,
                       (drop[0], drop[1], call0 + li) if drop is not None else None, _c(h), head_dim=head_dim,
                       masked_rows_zero=key_mask is not None)      # (rows of h and of prompts behind their lengths are zeros here)
        if text_lens is not None:
            h = KeepRowsFn.apply(h, n, text_lens)
    head = tr.to_pred[0]
    return RowDotReluFn.apply(_c(h), head.weight, head.bias)


def duration_pitch_forward_train(dp, x, prompts, text_lens=None, prompt_lens=None):
    """`DurationPitchPredictor.forward` (NS2:511-527) as a differentiable graph: x = token ids [b, n] or phoneme encodings [b, n, d],
    prompts [b, n_p, d] -> (duration, pitch), each [b, n].  Dropout as in the reference: the trunk hands `dropout` to its Attention only
    (NS2:430-446: the conv blocks keep their own default 0), so in train() mode it acts on the attention probabilities alone -- the stateless
    keep function of csrc/dropout_keep.h under one device-side seed per pass, call index = trunk * depth + layer.  `dp.dropout_seed`
    (an int64 tensor of one element) replaces the draw; `dp.last_dropout_seed` is what the last pass used.
    text_lens / prompt_lens (`ragged_conditioning`; include/ns2hip_train.h): phonemes / prompt rows per utterance, integer
    [b]; either alone is allowed, the other side then counts as full.  Rows of x and of prompts behind their lengths are selected to 0
    once, ONE byte mask [b, n + n_p] -- keys [0, text_lens[i]) and [n, n + prompt_lens[i]), formed on the device -- serves every layer of
    both trunks on the existing key-mask / dropout attention kernels, and the durations and pitches from text_lens[i] on come back as
    exact 0 with a zero cotangent.  Nothing reads a device tensor of lengths on the host.
    With text_lens the context rows are put in the ORDER THEY HAVE ALONE: a stable sort of the byte mask (on the device, once per pass)
    gives the row order [own text | own prompt | the hidden rows], every attention gathers cat(norm(x), prompts) by it, and the mask
    becomes the prefix [0, text_lens[i] + prompt_lens[i]).  Same keys, same values -- but a prompt key at position n + j of the padded
    context sits at text_lens[i] + j alone, and the attention kernels' sums follow the key position: measured on the MI355X, one row of
    text padding moved the durations by 6.5e-7 and the input gradient by 4.1e-6 against the utterance alone (twice the equal-length
    yardstick: 3e-7), while hidden keys BEHIND the own ones (prompt_lens alone, the prompt encoder) leave every bit where it was."""
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
        tl = km = keep = ctx_order = None
        if text_lens is not None or prompt_lens is not None:
            n_p, dev = pr.shape[1], pr.device
            ones = lambda k: torch.ones(b, k, dtype=torch.bool, device=dev)              # noqa: E731
            prefix = lambda l, k: torch.arange(k, device=dev)[None] < l.clamp(1, k)[:, None]      # noqa: E731
            tm, pm = ones(n), ones(n_p)
            if text_lens is not None:
                tl = ops._front_lens(text_lens, b, dev)
                h = KeepRowsFn.apply(h, n, tl)
                tm = keep = prefix(tl, n)
            if prompt_lens is not None:
                pl = ops._front_lens(prompt_lens, b, dev)
                pr = KeepRowsFn.apply(pr.reshape(b * n_p, -1), n_p, pl).reshape(b, n_p, -1)
                pm = prefix(pl, n_p)
            km = torch.cat((tm, pm), dim=1)
            if text_lens is not None:                                 # hidden text rows lie in front of the prompt's: own rows first
                hidden, order = torch.sort((~km).to(torch.uint8), dim=1, stable=True)
                km, ctx_order = hidden == 0, order[..., None].expand(-1, -1, pr.shape[-1])
            km = km.to(torch.uint8).contiguous()
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
        if km is None:
            return tuple(_trunk_train(tr, h, pr, b, n, drop, ti * depth, hd).reshape(b, n).to(dtype) for ti, tr in enumerate(trunks))
        outs = []
        for ti, tr in enumerate(trunks):
            o = _trunk_train(tr, h, pr, b, n, drop, ti * depth, hd, tl, km, ctx_order).reshape(b, n)
            if keep is not None:                                      # a select: exact 0 behind a length, and a zero cotangent there
                o = torch.where(keep, o, torch.zeros((), dtype=o.dtype, device=o.device))
            outs.append(o.to(dtype))
        return tuple(outs)


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
