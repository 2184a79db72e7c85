"""Differentiable PyTorch composite of `Model.forward`: fp32 torch ops on the module's own parameters.

Since round 4 training has HIP kernels of its own (the `training/` package: forward AND backward in libns2hip, `train_backend="hip"`, the
default of this package's `Model` on an MI355X; NS2:1635, NS2:1886).  This composite is what is left for the cases those kernels do
not take -- CPU tensors (the CPU test-suite), `train_backend="composite"`, a model `training.unsupported_reason` rejects (a head
dimension other than 64 in the backward kernels, non-fp32 parameters) -- and the yardstick bench.py times beside the HIP training
step (`side.train_step.*.pytorch_composite_ms_per_step`).  Inference (`torch.no_grad()` -- `NaturalSpeech2.sample`,
`forward_with_cond_scale` in the sampling loop, bench.py's timed region) never reaches this file.
"""
import math

import torch
import torch.nn.functional as F


def _causal_conv(x_bnc, conv, dilation=1):
    k = conv.weight.shape[-1]
    x = F.pad(x_bnc.transpose(1, 2), (dilation * (k - 1), 0))
    return F.conv1d(x, conv.weight, conv.bias, dilation=dilation).transpose(1, 2)


def _rmsnorm(x, norm, t=None):
    out = F.normalize(x, dim=-1) * math.sqrt(x.shape[-1])
    if norm.gamma is not None:
        out = out * norm.gamma
    if norm.to_gamma_beta is None:
        return out
    g, b = norm.to_gamma_beta(t).chunk(2, dim=-1)
    return out * g[:, None] + b[:, None]


def _attention(x, attn, heads, context=None, include_queries=False, key_mask=None, dropout_p=0.):
    ctx = x if context is None else (torch.cat((x, context), dim=1) if include_queries else context)
    q = attn.to_q(x)
    k, v = attn.to_kv(ctx).chunk(2, dim=-1)
    b, n, _ = q.shape

    def sp(t):
        return t.reshape(b, t.shape[1], heads, -1).transpose(1, 2)

    am = None if key_mask is None else key_mask[:, None, None, :].bool()          # ATT:92-94: key-padding mask, True = attend
    o = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=am, dropout_p=dropout_p)
    return attn.to_out(o.transpose(1, 2).reshape(b, n, -1))


def _feedforward(x, ff, causal_conv):
    h = getattr(ff, "0")(x)
    a, gate = h.chunk(2, dim=-1)
    h = F.gelu(gate) * a
    if causal_conv:
        h = _causal_conv(h, getattr(getattr(ff, "2"), "1"))
        return getattr(ff, "3")(h)
    return getattr(ff, "2")(h)


def _prefix_mask(lens, b, n, device):
    """[b, n] bool, True on the rows [0, lens[i]) of utterance i; lengths clamped into [1, n] as the kernels do (include/ns2hip.h)"""
    ln = torch.as_tensor(lens, device=device).long().clamp(1, n)
    assert ln.shape == (b,), f"lengths must hold one count per utterance: [{b}]"
    return torch.arange(n, device=device)[None] < ln[:, None]


def _keep_rows(x_bnc, mask):
    """rows outside the mask become exactly 0 -- a select, not a product: what lies there may be NaN"""
    return x_bnc if mask is None else torch.where(mask[..., None], x_bnc, torch.zeros((), dtype=x_bnc.dtype, device=x_bnc.device))


def model_forward_autograd(m, x, times, prompt=None, cond=None, cond_drop_prob=None, lens=None, prompt_lens=None):
    """`prompt_lens` (not in the reference; Model.forward's): prompt rows per utterance, integer [b].  The prompt is seen in two places,
    the mean of to_prompt_cond and the keys of the perceiver resampler: the mean runs over rows [0, prompt_lens[i]) and the resampler's
    keys cat(latents, prompt) get the mask [all latents | those rows] (include/ns2hip_frontend.h).
    `lens` (not in the reference; Model.forward's): frames per utterance of a ragged batch, integer [b].  The self-attention is the
    one place where a frame sees later frames, so it alone gets the key mask arange(n) < lens[:, None]: out[i, :lens[i]] is what
    utterance i gives alone.  The restatement of the HIP kernels' rule (include/ns2hip.h), lengths clamped into [1, n] as there."""
    b, n, _ = x.shape
    self_mask = None
    if lens is not None:
        ln = torch.as_tensor(lens, device=x.device).long().clamp(1, n)
        assert ln.shape == (b,), f"lens must hold one frame count per utterance: [{b}]"
        self_mask = torch.arange(n, device=x.device)[None] < ln[:, None]
    p = m.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
    w = getattr(m.to_time_cond, "0").weights
    tt = times[:, None]
    fr = tt * w[None] * 2 * math.pi
    t = F.silu(getattr(m.to_time_cond, "1")(torch.cat((tt, fr.sin(), fr.cos()), dim=-1)))
    c = None
    h = x
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
        if prompt_lens is not None:
            pm = _prefix_mask(prompt_lens, b, prompt.shape[1], x.device)
            prompt = _keep_rows(prompt, pm)
            pmean = prompt.sum(dim=1) / pm.sum(dim=1, keepdim=True).to(prompt.dtype)
            res_mask = torch.cat((torch.ones(b, m.perceiver_resampler.latents.shape[0], dtype=torch.bool, device=x.device), pm), dim=1)
        else:
            pmean = prompt.mean(dim=1)
        pc = F.silu(getattr(m.to_prompt_cond, "1")(pmean))
        pc = torch.where(dm[:, None], m.null_prompt_cond, pc)
        t = torch.cat((t, pc), dim=-1)
        pr = m.perceiver_resampler
        px = pr.proj_context(prompt) if hasattr(pr, "proj_context") else prompt
        lat = pr.latents[None].expand(b, -1, -1)
        for attn, ff in pr.layers:
            lat = _attention(lat, attn, m.heads, context=px, include_queries=True, key_mask=res_mask) + lat
            lat = _feedforward(lat, ff, False) + lat
        c = torch.where(dm[:, None, None], m.null_prompt_tokens, _rmsnorm(lat, pr.norm))
        cm = F.conv1d(cond, m.cond_to_model_dim.weight, m.cond_to_model_dim.bias)
        cm = torch.where(mask()[:, None, None], m.null_cond, cm)
        if cm.shape[-1] > n:
            cm = cm[..., :n]
        elif cm.shape[-1] < n:
            cm = F.pad(cm, (0, n - cm.shape[-1]))
        h = h + cm.transpose(1, 2)
    wn = m.wavenet
    h0 = _causal_conv(h, wn.init_conv)
    cols = [h0] * m.wavenet_layers
    skips = []
    for s, st in enumerate(wn.stacks):
        nxt = []
        for i, blk in enumerate(st.blocks):
            u = cols[i]
            g, be = blk.to_time_cond(t).chunk(2, dim=-1)
            z = _causal_conv(u, blk.conv, 2 ** i) * g[:, None] + be[:, None]
            z = z.tanh() * z.sigmoid() + _causal_conv(u, blk.res_conv)
            nxt.append(z)
            if blk.skip_conv is not None:
                skips.append(_causal_conv(z, blk.skip_conv))
        cols = nxt
    h = _causal_conv(torch.stack(skips).sum(0), wn.final_conv)
    for layer in m.transformer.layers:
        h = _attention(_rmsnorm(h, getattr(layer, "0"), t), getattr(layer, "1"), m.heads, key_mask=self_mask) + h
        if m.condition_on_prompt:
            h = _attention(_rmsnorm(h, getattr(layer, "2"), t), getattr(layer, "3"), m.heads, context=c) + h
        h = _feedforward(_rmsnorm(h, getattr(layer, "4"), t), getattr(layer, "5"), True) + h
    tp = m.transformer.to_pred
    return getattr(tp, "1")(_rmsnorm(h, getattr(tp, "0")))


def model_forward_autograd_ragged(m, x, times, lens, prompt=None, cond=None, cond_drop_prob=None, prompt_lens=None):
    """`model_forward_autograd` with `lens` as the TRAINING pass of a ragged batch runs it (Model.forward under autograd with
    `ragged_training`; the restatement of training/model_pass.py's rule, include/ns2hip_train.h): frames of x and cond from a
    length on are selected to 0 at the entry (NaN may lie there, and a masked key's 0 * NaN would reach the rows before it), and the
    returned rows from a length on are selected to 0, which zeroes their cotangent: utterance i contributes to the output and to
    every gradient what it contributes alone at lens[i] frames.  Lengths may be a device tensor: nothing here reads them on the host."""
    b, n, _ = x.shape
    mask = _prefix_mask(lens, b, n, x.device)
    if cond is not None:
        cond = _keep_rows(cond.transpose(1, 2), _prefix_mask(lens, b, cond.shape[-1], x.device)).transpose(1, 2)
    return _keep_rows(model_forward_autograd(m, _keep_rows(x, mask), times, prompt=prompt, cond=cond, cond_drop_prob=cond_drop_prob, lens=lens,
                                             prompt_lens=prompt_lens), mask)


# ---- the plain Transformer and the two conditioning encoders under autograd (NS2:1073-1115, 228-341): joint training of
# prompt_enc / phoneme_enc with the denoiser (NS2:1538-1543) needs gradients through them.  The default (`train_backend="composite"`), the
# CPU path, and the fall-back of `train_backend="hip"` (training/encoder_pass.py: `*_forward_train`) for what `training.encoder_unsupported_reason` names.
def transformer_forward_autograd(tr, x, mask=None):
    p = tr.dropout if tr.training else 0.
    for norm1, attn, norm2, ff in tr.layers:
        x = _attention(_rmsnorm(x, norm1), attn, tr.heads, key_mask=mask, dropout_p=p) + x
        x = _feedforward(_rmsnorm(x, norm2), ff, False) + x
    return _rmsnorm(x, tr.norm) if hasattr(tr.norm, "gamma") else x


def speech_prompt_encoder_autograd(enc, x, lens=None):
    """lens (not in the reference): prompt rows per utterance, integer [b].  The "same" convolutions read zeros behind a length (the input
    and every convolution's output are zeroed there, as behind the end of an utterance alone), the Transformer's keys stop at it, and the
    output rows from lens[i] on are 0: rows [0, lens[i]) are what utterance i gives alone (include/ns2hip_frontend.h)."""
    mask = None if lens is None else _prefix_mask(lens, x.shape[0], x.shape[1], x.device)
    h = _keep_rows(x, mask).transpose(1, 2)
    for m in enc.conv:
        if isinstance(m, torch.nn.Conv1d):
            h = _keep_rows(F.silu(F.conv1d(h, m.weight, m.bias, padding=enc.padding)).transpose(1, 2), mask).transpose(1, 2)
    return _keep_rows(transformer_forward_autograd(enc.transformer, h.transpose(1, 2), mask=mask), mask)


def phoneme_encoder_autograd(enc, ids, mask=None):
    ids = ids.masked_fill(ids < 0, enc.pad_id)
    h = F.embedding(ids, enc.token_emb.weight)
    h = F.silu(_causal_conv(h, enc.conv[1]))
    h = F.dropout(h, enc.conv_dropout, enc.training)
    return transformer_forward_autograd(enc.transformer, h, mask=mask)


# ---- DurationPitchPredictor (NS2:344-527) and the length regulator of text-conditioned sampling (NS2:87-104, 164-175, 1449-1455)
def _group_norm_rows(h_bcn, norm, mask):
    """nn.GroupNorm whose statistics of utterance i run over the rows inside mask[i] (biased variance, as F.group_norm)"""
    if mask is None:
        return F.group_norm(h_bcn, norm.num_groups, norm.weight, norm.bias, norm.eps)
    b, c, n = h_bcn.shape
    g = norm.num_groups
    hg = h_bcn.reshape(b, g, c // g, n)
    mm = mask[:, None, None, :]
    zero = torch.zeros((), dtype=hg.dtype, device=hg.device)
    cnt = (mask.sum(dim=1) * (c // g)).to(hg.dtype)[:, None, None, None]
    mean = torch.where(mm, hg, zero).sum(dim=(2, 3), keepdim=True) / cnt
    var = torch.where(mm, (hg - mean) ** 2, zero).sum(dim=(2, 3), keepdim=True) / cnt
    out = ((hg - mean) * torch.rsqrt(var + norm.eps)).reshape(b, c, n)
    return out * norm.weight[None, :, None] + norm.bias[None, :, None]


def _dp_trunk_autograd(tr, x, prompts, training, text_mask=None, key_mask=None):
    # the trunk hands `dropout` to its Attention only; Block / ConvBlock keep their own default 0 (NS2:430-446): no dropout after the convolutions
    p = tr.dropout if training else 0.
    k = tr.kernel_size
    for convs, norm, attn in tr.layers:
        for blk in convs:
            if tr.use_resnet_block:                                   # ResnetBlock: h = Blocks(x); out = h + x (NS2:394-398)
                h = x.transpose(1, 2)
                for b in blk.blocks:
                    h = F.conv1d(h, b.proj.weight, b.proj.bias, padding=k // 2)
                    h = _keep_rows(F.silu(_group_norm_rows(h, b.norm, text_mask)).transpose(1, 2), text_mask).transpose(1, 2)
                x = _keep_rows((h + x.transpose(1, 2)).transpose(1, 2), text_mask)
            else:                                                     # ConvBlock (NS2:402-409)
                x = _keep_rows(F.silu(F.conv1d(x.transpose(1, 2), blk[1].weight, blk[1].bias, padding=k // 2)).transpose(1, 2), text_mask)
        x = _keep_rows(_attention(_rmsnorm(x, norm), attn, tr.heads, context=prompts, include_queries=True, key_mask=key_mask, dropout_p=p) + x,
                       text_mask)
    head = tr.to_pred[0]
    out = F.relu(F.linear(x, head.weight, head.bias)[..., 0])
    return out if text_mask is None else torch.where(text_mask, out, torch.zeros((), dtype=out.dtype, device=out.device))


def duration_pitch_autograd(dp, x, prompts, text_lens=None, prompt_lens=None):
    """text_lens / prompt_lens (not in the reference): phonemes / prompt rows per utterance, integer [b]; either alone is allowed, the
    other side then counts as full.  Rows behind a length are zeros for the "same" convolutions, the GroupNorm statistics of utterance i
    run over its own phonemes, the attention keys cat(norm(x), prompts) are [0, text_lens[i]) and [n, n + prompt_lens[i]), and the
    durations and pitches from text_lens[i] on come back 0 (include/ns2hip_frontend.h)."""
    if isinstance(dp.phoneme_token_emb, torch.nn.Embedding):
        x = dp.phoneme_token_emb(x)
    text_mask = key_mask = None
    if text_lens is not None or prompt_lens is not None:
        b, n, n_p = x.shape[0], x.shape[1], prompts.shape[1]
        text_mask = None if text_lens is None else _prefix_mask(text_lens, b, n, x.device)
        pm = None if prompt_lens is None else _prefix_mask(prompt_lens, b, n_p, x.device)
        x, prompts = _keep_rows(x, text_mask), _keep_rows(prompts, pm)
        ones = lambda k: torch.ones(b, k, dtype=torch.bool, device=x.device)          # noqa: E731
        key_mask = torch.cat((ones(n) if text_mask is None else text_mask, ones(n_p) if pm is None else pm), dim=1)
    return tuple(_dp_trunk_autograd(tr, x, prompts, dp.training, text_mask, key_mask) for tr in (dp.to_duration_pred, dp.to_pitch_pred))


def f0_to_coarse(f0, f0_bin=256, f0_max=1100.0, f0_min=50.0):
    """NS2:164-175 in the same fp32 operations"""
    f0_mel_max = 1127 * torch.log(1 + torch.tensor(f0_max) / 700)
    f0_mel_min = 1127 * torch.log(1 + torch.tensor(f0_min) / 700)
    f0_mel = 1127 * (1 + f0 / 700).log()
    pos = f0_mel > 0
    f0_mel = torch.where(pos, (f0_mel - f0_mel_min.to(f0.device)) * (f0_bin - 2) / (f0_mel_max - f0_mel_min).to(f0.device) + 1, f0_mel)
    f0_mel = f0_mel.masked_fill(f0_mel <= 1, 1.)
    f0_mel = f0_mel.masked_fill(f0_mel > f0_bin - 1, f0_bin - 1)
    return (f0_mel + 0.5).int()


def length_regulate(duration, pitch, enc, pitch_table, return_totals=False):
    """generate_mask_from_repeats + expand_encodings (NS2:87-104, 1449-1455) as a gather: frame f of utterance b takes the
    phoneme whose [exclusive, inclusive) prefix of int(duration) holds f, zeros past the utterance's total.  The reference's 0/1
    mask einsum sums one product x * 1 with zeros, so enc[ph] + pitch_table[coarse[ph]] is bit-identical to it.  Negative
    durations (the predictor's ReLU never makes one) count as 0 frames.  -> [B, D, n_frames]; return_totals: (that, the utterances' own
    frame totals [B])"""
    reps = duration.int().clamp(min=0)
    cum = reps.cumsum(dim=-1)
    totals = cum[:, -1]
    n_frames = int(totals.max().item())
    frames = torch.arange(n_frames, device=duration.device)
    ph = torch.searchsorted(cum.contiguous(), frames[None].expand(cum.shape[0], -1).contiguous().to(cum.dtype), right=True)
    valid = frames[None] < totals[:, None]
    ph = ph.clamp(max=cum.shape[1] - 1)
    e = torch.gather(enc, 1, ph[..., None].expand(-1, -1, enc.shape[-1]))
    pe = F.embedding(f0_to_coarse(pitch).long(), pitch_table)
    pe = torch.gather(pe, 1, ph[..., None].expand(-1, -1, pe.shape[-1]))
    out = torch.where(valid[..., None], e + pe, torch.zeros((), dtype=e.dtype, device=e.device))
    return (out.transpose(1, 2), totals) if return_totals else out.transpose(1, 2)


# ---- Aligner (aligner.py of the reference) and the text-conditioned training pass (utils.py:4-26, NS2:1449-1455)
def aligner_net_autograd(net, queries, keys, mask=None):
    """AlignerNet.forward (aligner.py:62-90): (attn [b, 1, T, n], attn_logp [b, 1, T, n]); attn_logp is the plain distance"""
    k = F.conv1d(keys, net.key_layers[0].weight, net.key_layers[0].bias, padding=1).relu()
    k = F.conv1d(k, net.key_layers[2].weight, net.key_layers[2].bias)
    q = F.conv1d(queries, net.query_layers[0].weight, net.query_layers[0].bias, padding=1).relu()
    q = F.conv1d(q, net.query_layers[2].weight, net.query_layers[2].bias).relu()
    q = F.conv1d(q, net.query_layers[4].weight, net.query_layers[4].bias)
    logp = torch.cdist(q.transpose(1, 2), k.transpose(1, 2))[:, None]
    if mask is not None:
        logp = logp.masked_fill(~mask.bool()[..., None, :], -torch.finfo(logp.dtype).max)
    return logp.softmax(dim=-1), logp


def maximum_path_composite(value, mask, const=None):
    """maximum_path (aligner.py:97-130) as a PyTorch loop: the DP over columns from v = 0 (ties stay), directions forced to 1
    outside the mask, the backtrack from row mask[:, :, 0].sum() - 1 with Python's negative indexing, the path times the mask"""
    dev = value.device
    neg = torch.tensor(float("-inf"), device=dev) if const is None else const
    value = value * mask
    b, t_x, t_y = value.shape
    v = torch.zeros(b, t_x, dtype=torch.float32, device=dev)
    rows = torch.arange(t_x, device=dev)
    stay = torch.empty(b, t_x, t_y, dtype=torch.bool, device=dev)
    for j in range(t_y):
        above = torch.cat((neg.expand(b, 1).to(v.dtype), v[:, :-1]), dim=1)
        s = v >= above
        stay[:, :, j] = s
        v = torch.where(rows[None] <= j, torch.where(s, v, above) + value[:, :, j], neg.to(v.dtype))
    stay = stay | ~mask.bool()
    idx = mask[:, :, 0].sum(1).long() - 1
    path = torch.zeros(b, t_x, t_y, dtype=torch.float32, device=dev)
    bi = torch.arange(b, device=dev)
    for j in range(t_y - 1, -1, -1):
        path[bi, idx, j] = 1
        idx = idx + stay[bi, idx, j].long() - 1
    return (path * mask.float()).to(value.dtype)


def average_over_durations_composite(values, durs):
    """utils.py:4-26: differences of fp32 prefix sums of the values and of their non-zero count at the phonemes' frame ends"""
    ends = torch.cumsum(durs, dim=1).long()
    starts = F.pad(ends[:, :-1], (1, 0))
    nz = F.pad(torch.cumsum(values != 0.0, dim=2), (1, 0))
    cs = F.pad(torch.cumsum(values, dim=2), (1, 0))
    f = values.shape[1]
    e, s = ends[:, None].expand(-1, f, -1), starts[:, None].expand(-1, f, -1)
    sums = (torch.gather(cs, 2, e) - torch.gather(cs, 2, s)).to(values.dtype)
    cnt = (torch.gather(nz, 2, e) - torch.gather(nz, 2, s)).to(values.dtype)
    return torch.where(cnt == 0.0, cnt, sums / cnt).to(values.dtype)


def expand_with_path(enc, path, pitch, table):
    """expand_encodings (NS2:1449-1455): enc [b, n, D], path [b, n, T] 0/1, pitch [b, n] -> [b, D, T], the reference's two
    0/1 einsums (each frame sums one product x * 1 with zeros)"""
    pe = F.embedding(f0_to_coarse(pitch).long(), table)
    return torch.einsum("bnt,bnd->bdt", path, enc) + torch.einsum("bnt,bnd->bdt", path, pe)
