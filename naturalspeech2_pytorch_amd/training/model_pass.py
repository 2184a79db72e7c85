"""`Model.forward` under autograd: the denoiser's training pass on the Functions of functions.py"""
import math

import torch
import torch.nn.functional as F

from .functions import HEAD_DIMS_TRAIN, attn_apply, train_head_dim, CondProjectionsFn, FeedForwardFn, GemmFn, NormLinearFn, RmsNormFn, WavenetBlockFn, _c, _lin
from .passes import TRAIN_PRECISIONS, _enter, _ScaleIn, training_pass


def _resampler(pr, prompt, heads, head_dim=64, key_mask=None):
    """PerceiverResampler (NS2:532-579) on the Functions of functions.py: per layer latents += Attention(latents, context = cat(latents,
    proj(prompt))) and latents += FeedForward(latents) (no norms in front, no conv), then RMSNorm * gamma.  Round 4 ran this part of
    the conditioned model's graph as the PyTorch composite (0.2 % of the FLOPs, but the one piece of `Model`'s backward on torch ops).
    key_mask: uint8 [b, Lm + n_p] or None -- the keys [0, Lm + prompt_lens[i]) of cat(latents, prompt) of a ragged prompt batch: every
    attention then runs on the key-mask training kernels (the rows of `prompt` behind a length are zeros: the caller's select)."""
    b, n_p, _ = prompt.shape
    pc = getattr(pr, "proj_context", None)
    px = _c(prompt).reshape(b * n_p, -1)
    if isinstance(pc, torch.nn.Linear):                                      # dim_prompt != dim (NS2:548)
        px = GemmFn.apply(px, pc.weight, pc.bias, None, 0, 1)
    Lm, d = pr.latents.shape
    px = px.reshape(b, n_p, d)
    if key_mask is not None:                                                 # (proj_context's bias: the hidden rows are zeros again -- AttnFn masked_rows_zero)
        px = _keep(px, key_mask[:, -n_p:, None].bool())
    lat = _enter(pr.latents)[None].expand(b, -1, -1).reshape(b * Lm, d)      # (a copy: its gradient sums over the batch into pr.latents)
    for attn, ff in pr.layers:
        context = torch.cat((lat.reshape(b, Lm, d), px), dim=1).reshape(b * (Lm + n_p), d)     # cross_attn_include_queries, NS2:1060-1061
        if key_mask is None:
            lat = attn_apply(_c(lat), None, context, attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, Lm, heads, Lm + n_p, head_dim=head_dim)
        else:
            lat = attn_apply(_c(lat), None, context, attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, Lm, heads, Lm + n_p, None, key_mask,
                             head_dim=head_dim, masked_rows_zero=True)
        l1, l2 = getattr(ff, "0"), getattr(ff, "2")
        lat = FeedForwardFn.apply(_c(lat), None, l1.weight, l1.bias, None, None, l2.weight, l2.bias, Lm)
    return RmsNormFn.apply(_c(lat), pr.norm.gamma).reshape(b, Lm, d)


def _lens_and_mask(lens, b, n, device):
    """`lens` of a ragged batch -> (int32 [b] on the device, what the kernels read; bool [b, n, 1], True on the rows [0, clamp(lens[i], 1, n))).
    An int32 device tensor comes back as it is: no copy and no host read, so a captured pass follows values rewritten between replays."""
    ln = torch.as_tensor(lens).to(device=device, dtype=torch.int32).contiguous()
    assert ln.shape == (b,), f"lens must hold one frame count per utterance: [{b}]"
    return ln, (torch.arange(n, device=device)[None] < ln.clamp(1, n)[:, None])[..., None]


def _keep(t_bnd, mask):
    """rows outside the mask become exactly 0 -- a select, not a product: what lies there may be NaN (its cotangent there becomes 0 too)"""
    return torch.where(mask, t_bnd, torch.zeros((), dtype=t_bnd.dtype, device=t_bnd.device))


def model_forward_train(m, x, times, prompt=None, cond=None, cond_drop_prob=None, lens=None, prompt_lens=None):
    """`Model.forward` (NS2:929-1000) as a differentiable graph whose token-sized arithmetic is HIP (package docstring).
    `m` owns the reference's parameters (this package's `Model` or `compat.HipBackedModel`).  `m.train_precision`: "exact"
    (default: bf16 x3) or "mixed" (IEEE-half product + fp8 correction terms on FMT_H8 operands under a loss scale, `passes._Scale`).
    `lens` (not in the reference): frames per utterance of a ragged batch, integer [b] (include/ns2hip_train.h).  Rows
    of x and of the projected cond from a length on are selected to 0 at the entry, every self-attention stops at the length in both
    directions, and the returned rows from a length on are selected to 0 -- which also zeroes the cotangent there.  No host read.
    `prompt_lens` (not in the reference; `ragged_conditioning`): prompt rows per utterance, integer [b] (include/ns2hip_train.h;
    DESIGN §9).  The prompt rows behind a length are selected to 0 at the entry, the mean of to_prompt_cond is a masked sum over rows
    [0, prompt_lens[i]) divided by the clamped length, and the perceiver resampler's attentions run under the key mask
    [0, Lm + prompt_lens[i]) of cat(latents, prompt), all formed on the device.  With and without `lens`.
    `m.ragged_skip_training` (include/ns2hip_train.h): with `lens` and n % 256 == 0 the products over the b n frame
    rows -- forward, dgrad, row-plane weight gradient -- are handed the lengths and skip the 256-row tiles hidden behind them, writing
    zeros there; decided here, once per pass.  Same loss, rows and gradients, bit for bit."""
    tp = getattr(m, "train_precision", "exact")
    assert tp in TRAIN_PRECISIONS, f"train_precision must be one of {sorted(TRAIN_PRECISIONS)}"
    with training_pass(TRAIN_PRECISIONS[tp], x) as p:
        pl = {}
        if prompt_lens is not None:
            pl = dict(prompt_keep=_lens_and_mask(prompt_lens, x.shape[0], prompt.shape[1], x.device)[1])
        if lens is None:
            out = _forward_train(m, x, times, prompt, cond, cond_drop_prob, **pl)
        else:
            ln, keep = _lens_and_mask(lens, x.shape[0], x.shape[1], x.device)
            if getattr(m, "ragged_skip_training", False) and x.shape[1] % 256 == 0:
                pl["skip"] = ln
            out = _keep(_forward_train(m, x, times, prompt, cond, cond_drop_prob, ln, keep, **pl), keep)
        if p.scale is not None:
            m._last_loss_scale = p.scale             # (inspection / tests: the scale the last backward chose)
            out = _ScaleIn.apply(out, p.scale)
        return out


def _forward_train(m, x, times, prompt, cond, cond_drop_prob, lens=None, keep=None, prompt_keep=None, skip=None):
    """lens / keep: `_lens_and_mask` of a ragged batch, or neither; prompt_keep: the bool [b, n_p, 1] of `_lens_and_mask(prompt_lens)`, or None;
    skip: `lens` again when the products over the b n frame rows skip their hidden row tiles (`ragged_skip_training`), else None -- then
    every call below is the call it was.  The resampler, cond_to_model_dim and the cross attention's k | v are not frame-row products."""
    b, n, d = x.shape
    M = b * n
    p = m.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
    heads = m._hip_cfg["heads"]
    hd = train_head_dim(m, m._hip_cfg["dim_head"])                           # (64 unless `head_dim_training`)
    # ---- rows = batch entries: time embedding and every conditioning projection (PyTorch ops, see the package docstring)
    w = getattr(m.to_time_cond, "0").weights
    tt = times.float()[:, None]
    fr = tt * w[None] * 2 * math.pi
    t = F.silu(_lin(getattr(m.to_time_cond, "1"), torch.cat((tt, fr.sin(), fr.cos()), dim=-1)))
    c = None
    h = _enter((x.float() if keep is None else _keep(x.float(), keep)).reshape(M, d))   # (mixed arithmetic: the token-sized gradients below here are loss-scaled)
    if m.condition_on_prompt:
        assert prompt is not None and cond is not None

        def mask():
            if p == 1:
                return torch.ones(b, dtype=torch.bool, device=x.device)
            if p == 0:
                return torch.zeros(b, dtype=torch.bool, device=x.device)
            return torch.rand(b, device=x.device) < p

        dm = mask()
        res_mask = None
        if prompt_keep is None:
            pmean = prompt.float().mean(dim=1)
        else:
            # [b, d]-sized work on the device: a masked sum over the rows before a length / the clamped length (the mask has that many rows)
            prompt = _keep(prompt.float(), prompt_keep)
            # (sum times the reciprocal, the form of torch's mean: a device tensor of full lengths gives prompt.mean(dim=1))
            pmean = prompt.sum(dim=1) * (1.0 / prompt_keep.sum(dim=1).to(prompt.dtype))
            Lm = m.perceiver_resampler.latents.shape[0]
            res_mask = torch.cat((torch.ones(b, Lm, dtype=torch.bool, device=x.device), prompt_keep[..., 0]), dim=1).to(torch.uint8).contiguous()
        pc = F.silu(_lin(getattr(m.to_prompt_cond, "1"), pmean))
        pc = torch.where(dm[:, None], m.null_prompt_cond, pc)
        t = torch.cat((t, pc), dim=-1)
        # (`prompt` and `cond` come from trainable modules upstream -- the prompt / phoneme encoders, NS2:1635 -- so their gradients
        # leave the scaled domain like x's: ADVICE r5)
        c = torch.where(dm[:, None, None], _enter(m.null_prompt_tokens), _resampler(m.perceiver_resampler, _enter(prompt.float()), heads, hd, res_mask))   # [b, Lm, d]
        # cond_to_model_dim: 1x1 conv over channel-first cond (NS2:978) = a Linear over the frames
        n_c = cond.shape[-1]
        if keep is not None:
            # (the frames of cond itself first: a NaN there would reach the projection's weight gradient as 0 * NaN)
            cond = _keep(cond.float().transpose(1, 2), torch.arange(n_c, device=x.device)[None, :, None] < lens.clamp(1, n)[:, None, None]).transpose(1, 2)
        cm = GemmFn.apply(_enter(_c(cond.float().transpose(1, 2)).reshape(b * n_c, -1)), m.cond_to_model_dim.weight, m.cond_to_model_dim.bias, None,
                          n_c, 1)
        cm = cm.reshape(b, n_c, d)
        cm = torch.where(mask()[:, None, None], _enter(m.null_cond).t()[None], cm)
        if n_c > n:
            cm = cm[:, :n]
        elif n_c < n:
            cm = F.pad(cm, (0, 0, 0, n - n_c))
        if keep is not None:
            cm = _keep(cm, keep)
        h = h + _c(cm).reshape(M, d)
        c2 = _c(c.float()).reshape(b * c.shape[1], d)
    t = _c(t)
    # every conditioning projection of the pass at once (CondProjectionsFn), in the order the graph below consumes them
    lins = [blk.to_time_cond for st in m.wavenet.stacks for blk in st.blocks]
    for layer in m.transformer.layers:
        lins += [getattr(layer, str(i)).to_gamma_beta for i in ((0, 2, 4) if m.condition_on_prompt else (0, 4))]
    if all(l.bias is not None for l in lins):
        films = dict(zip(map(id, lins), CondProjectionsFn.apply(t, *[q for l in lins for q in (l.weight, l.bias)])))
    else:                                                                    # (the reference's Linears all carry a bias)
        films = {}

    def film_of(lin):
        f = films.get(id(lin))
        return f if f is not None else _lin(lin, t)

    sk = () if skip is None else (skip,)                                     # the trailing `lens` of the Functions, only when present
    wn = m.wavenet
    h0 = GemmFn.apply(h, wn.init_conv.weight, wn.init_conv.bias, None, n, 1, *((-1,) + sk if sk else ()))
    cols = [h0] * m._hip_cfg["wavenet_layers"]
    acc = None
    for st in wn.stacks:
        nxt = []
        for i, blk in enumerate(st.blocks):
            z = WavenetBlockFn.apply(_c(cols[i]), film_of(blk.to_time_cond), blk.conv.weight, blk.conv.bias, blk.res_conv.weight,
                                     blk.res_conv.bias, n, 2 ** i, *sk)
            nxt.append(z)
            if blk.skip_conv is not None:                                    # sum of the skip convs (NS2:685-686, 725) as a chain of residuals
                acc = GemmFn.apply(_c(z), blk.skip_conv.weight, blk.skip_conv.bias, acc if acc is None else _c(acc), n, 1, *((-1,) + sk if sk else ()))
        cols = nxt
    h = GemmFn.apply(_c(acc), wn.final_conv.weight, wn.final_conv.bias, None, n, 1, *((-1,) + sk if sk else ()))
    for layer in m.transformer.layers:
        a1 = getattr(layer, "1")
        if lens is None:
            h = attn_apply(_c(h), film_of(getattr(layer, "0").to_gamma_beta), None, a1.to_q.weight, a1.to_kv.weight, a1.to_out.weight, n, heads, 0,
                           head_dim=hd)
        else:
            h = attn_apply(_c(h), film_of(getattr(layer, "0").to_gamma_beta), None, a1.to_q.weight, a1.to_kv.weight, a1.to_out.weight, n, heads, 0,
                           None, None, None, None, lens, head_dim=hd, row_lens=skip)
        if m.condition_on_prompt:
            a3 = getattr(layer, "3")
            h = attn_apply(_c(h), film_of(getattr(layer, "2").to_gamma_beta), c2, a3.to_q.weight, a3.to_kv.weight, a3.to_out.weight, n,
                           heads, c.shape[1], head_dim=hd, row_lens=skip)
        ff = getattr(layer, "5")
        l1, cv, l2 = getattr(ff, "0"), getattr(getattr(ff, "2"), "1"), getattr(ff, "3")
        h = FeedForwardFn.apply(_c(h), film_of(getattr(layer, "4").to_gamma_beta), l1.weight, l1.bias, cv.weight, cv.bias, l2.weight, l2.bias, n,
                                *((None,) + sk if sk else ()))
    tp = m.transformer.to_pred
    out = NormLinearFn.apply(_c(h), getattr(tp, "0").gamma, getattr(tp, "1").weight, n, *sk)
    return out.reshape(b, n, d).to(x.dtype)


def available(device):
    """the HIP training path needs the library and parameters on an MI355X"""
    return device.type == "cuda" and torch.cuda.is_available()


def unsupported_reason(m):
    """None when `model_forward_train` can run `m`, else why not.  The Functions are written for what the inference executor
    accepts (ns2_model_create): heads of 64 (q / k / v column offsets, the attention kernels' head dim, scale 1/8), dim a multiple
    of 32 (whole 32-column lines per operand row), fp32 parameters (the packs and the returned gradients are fp32).  Anything else
    must not reach the kernels (a `dim_head=32` model would read past its packed qkv planes).  A model with
    `head_dim_training = True` trains at dim_head 32 and 128 too (include/ns2hip_train.h: the passes hand dim_head to AttnFn)."""
    cfg = m._hip_cfg
    if getattr(m, "head_dim_training", False):
        if cfg["dim_head"] not in HEAD_DIMS_TRAIN:
            return f"dim_head={cfg['dim_head']} (the HIP training attention kernels have head dims 32, 64 and 128)"
    elif cfg["dim_head"] != 64:
        return f"dim_head={cfg['dim_head']} (the HIP attention backward has a head dim of 64 unless the model is built with head_dim_training=True)"
    if cfg["dim"] % 32:
        return f"dim={cfg['dim']} is not a multiple of 32"
    for name, p in m.named_parameters():
        if p.dtype != torch.float32:
            return f"parameter {name} is {p.dtype} (fp32 master weights are required)"
    return None


def rvq_ce_unsupported_reason(rq, x, indices):
    """None when `codec.rq` with `backend="hip"` (codec.py `ResidualVQCrossEntropy`) can run these tensors on ns2_rvq_ce, else why not: the
    caller falls back to the composite, as `Model`, the encoders, the predictor and the aligner do.  Checks metadata only: no host read."""
    if not (x.is_cuda and indices.is_cuda):
        return "CPU tensors (the kernel runs on the GPU)"
    if x.dtype != torch.float32:
        return f"x is {x.dtype} (the kernel is fp32)"
    if indices.dtype != torch.int64:
        return f"indices are {indices.dtype} (the kernel reads int64 codes, what the codec returns)"
    from .. import _lib
    try:
        _lib.load()
    except (_lib.Ns2Error, OSError) as e:
        return f"no library ({e})"
    return None
