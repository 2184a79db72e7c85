"""`DurationPitchPredictor` (NS2:344-527) and the length regulator of text-conditioned sampling (NS2:87-104, 164-175,
1449-1455, 1476-1483).

Each of the two trunks (`to_duration_pred`, `to_pitch_pred`) runs `depth` layers of [conv stack -> RMSNorm -> attention whose
keys / values are cat(norm(x), encoded prompts) (cross_attn_include_queries) -> residual], then Linear(dim, 1) + ReLU.  On the
HIP path the "same"-padded convolutions are the shifted-row GEMMs (conv_taps = k, pad_left = k // 2), a `ConvBlock` takes its
SiLU in the GEMM epilogue, a `ResnetBlock`'s GroupNorm + SiLU (+ residual) is csrc/duration_pitch.hip, RMSNorm / attention are
the hot path's kernels and the heads are a row dot product.  Under autograd (or on the CPU) the differentiable composite of
autograd_path.py runs instead (`train_backend="composite"`, the default), or with `train_backend="hip"` on the GPU
`training.duration_pitch_forward_train`: forward and backward on the HIP kernels.  Same constructor keywords and state_dict keys as
the reference classes.
"""
import torch
from torch import nn

from . import ops
from ._cache import PackedCache
from .model import _Attention, _NoParams, _RMSNorm, _PRECISIONS
from .transformer import TRAIN_BACKENDS, host_full_lens, needs_autograd


class _Block(nn.Module):                        # Block (NS2:346-369): Conv1d -> GroupNorm -> SiLU -> Dropout
    def __init__(self, dim, dim_out, kernel, groups=8):
        super().__init__()
        self.proj = nn.Conv1d(dim, dim_out, kernel, padding=kernel // 2)
        self.norm = nn.GroupNorm(groups, dim_out)


class _ResnetBlock(nn.Module):                  # ResnetBlock (NS2:371-400) with dim == dim_out: res_conv is the identity
    def __init__(self, dim, kernel, num_convs=2):
        super().__init__()
        self.blocks = nn.Sequential(*[_Block(dim, dim, kernel) for _ in range(num_convs)])
        self.res_conv = nn.Identity()


def _conv_block(dim, kernel):                   # ConvBlock (NS2:402-409): Rearrange, Conv1d, SiLU, Dropout, Rearrange
    return nn.Sequential(_NoParams(), nn.Conv1d(dim, dim, kernel, padding=kernel // 2), _NoParams(), _NoParams(), _NoParams())


class DurationPitchPredictorTrunk(nn.Module):   # NS2:411-481
    def __init__(self, dim=512, depth=10, kernel_size=3, dim_context=None, heads=8, dim_head=64, dropout=0.2,
                 use_resnet_block=True, num_convs_per_resnet_block=2, num_convolutions_per_block=3, use_flash_attn=False):
        super().__init__()
        self.dim, self.kernel_size, self.heads, self.dim_head, self.dropout = dim, kernel_size, heads, dim_head, dropout
        self.use_resnet_block = use_resnet_block
        conv = (lambda: _ResnetBlock(dim, kernel_size, num_convs_per_resnet_block)) if use_resnet_block else \
            (lambda: _conv_block(dim, kernel_size))
        self.layers = nn.ModuleList([
            nn.ModuleList([nn.Sequential(*[conv() for _ in range(num_convolutions_per_block)]), _RMSNorm(dim),
                           _Attention(dim, dim_head, heads, dim_context=dim_context)])
            for _ in range(depth)])
        self.to_pred = nn.Sequential(nn.Linear(dim, 1), _NoParams(), _NoParams())


class DurationPitchPredictor(nn.Module):
    def __init__(self, *, dim, num_phoneme_tokens=None, tokenizer=None, dim_encoded_prompts=None, num_convolutions_per_block=3,
                 use_resnet_block=True, num_convs_per_resnet_block=2, depth=10, kernel_size=3, heads=8, dim_head=64,
                 dim_hidden=512, dropout=0.2, use_flash_attn=False, precision="exact", train_backend="composite", head_dim_training=False,
                 ragged_conditioning=False):
        super().__init__()
        assert train_backend in TRAIN_BACKENDS, f"train_backend must be one of {TRAIN_BACKENDS}"
        self.train_backend = train_backend
        self.ragged_conditioning = ragged_conditioning      # True: forward(text_lens=, prompt_lens=) runs under autograd too (else it raises, as before)
        self.head_dim_training = head_dim_training      # True: train_backend="hip" takes dim_head 32 / 128 too (else: the composite, as before)
        self.dropout_seed = None                # train_backend="hip": an int64 tensor [1] replaces the per-pass draw of the attention dropout seed
        if kernel_size % 2 == 0:
            raise ValueError(f"kernel_size must be odd: Conv1d(padding=k // 2) with an even k ({kernel_size}) changes the length")
        if dim_hidden % 32 != 0:
            raise ValueError(f"dim_hidden must be a multiple of 32 (GroupNorm groups of 4-column vectors, 32-column operand lines), got {dim_hidden}")
        assert precision in _PRECISIONS, f"precision must be one of {sorted(_PRECISIONS)}"
        assert dim_head in (32, 64, 128), "the HIP attention kernel is built for head dims 32, 64 and 128"
        self.tokenizer = tokenizer
        if num_phoneme_tokens is None and tokenizer is not None:
            num_phoneme_tokens = tokenizer.vocab_size
        dim_encoded_prompts = dim if dim_encoded_prompts is None else dim_encoded_prompts
        self.phoneme_token_emb = nn.Embedding(num_phoneme_tokens, dim) if num_phoneme_tokens is not None else nn.Identity()
        kw = dict(dim=dim_hidden, depth=depth, kernel_size=kernel_size, dim_context=dim_encoded_prompts, heads=heads,
                  dim_head=dim_head, dropout=dropout, use_resnet_block=use_resnet_block,
                  num_convs_per_resnet_block=num_convs_per_resnet_block, num_convolutions_per_block=num_convolutions_per_block,
                  use_flash_attn=use_flash_attn)
        self.to_pitch_pred = DurationPitchPredictorTrunk(**kw)
        self.to_duration_pred = DurationPitchPredictorTrunk(**kw)
        self.to_duration_pred.load_state_dict(self.to_pitch_pred.state_dict())      # copy.deepcopy upstream (NS2:509)
        self.precision, self.dim_hidden, self.dropout = precision, dim_hidden, dropout
        self._cache = PackedCache(fingerprint_every=1)      # once per utterance: check the content on every call (EMA copies)

    def forward(self, x, encoded_prompts, prompt_mask=None, *, text_lens=None, prompt_lens=None):
        """x: token ids [b, n] (with num_phoneme_tokens) or phoneme encodings [b, n, dim_hidden]; encoded_prompts [b, n_p,
        dim_hidden].  Returns (duration, pitch), each [b, n].

        text_lens / prompt_lens (not in the reference): phonemes / prompt rows per utterance of a padded batch, integer
        [b], read on the device and clamped into [1, n] / [1, n_p]; either alone is allowed, the other side then counts as full.  The
        durations and pitches [0, text_lens[i]) are what utterance i gives alone with its text and prompt cut to its lengths, whatever
        lies behind them (NaN included); from text_lens[i] on they are exactly 0.  Under autograd they need `ragged_conditioning=True`
        (training/duration_pitch_pass.py with lengths, or the composite with the same lengths: the gradients are those of the utterances
        alone too); without the switch they raise, as before."""
        if not torch.is_tensor(x):
            raise NotImplementedError("List[str] input needs the tokenizer / espeak front-end (out of scope); pass token ids or "
                                      "phoneme encodings")
        if prompt_mask is not None:
            raise NotImplementedError("prompt_mask is not supported: the reference's Attend applies it to keys = cat(queries, "
                                      "prompts), which a [b, n_p] mask does not cover (NS2:1060-1066)")
        if text_lens is not None or prompt_lens is not None:
            if needs_autograd(self, x if x.is_floating_point() else None) and getattr(self, "ragged_conditioning", False):
                b = x.shape[0]                                         # full on the host: that side takes the call without its lengths, same bits
                text_lens = None if host_full_lens(text_lens, x.shape[1], b) else text_lens
                prompt_lens = None if host_full_lens(prompt_lens, encoded_prompts.shape[1], b) else prompt_lens
                if text_lens is None and prompt_lens is None:
                    return self.forward(x, encoded_prompts)
                if self.train_backend == "hip" and x.is_cuda:
                    from . import training
                    if training.available(x.device) and training.duration_pitch_unsupported_reason(self) is None:
                        return training.duration_pitch_forward_train(self, x, encoded_prompts, text_lens=text_lens, prompt_lens=prompt_lens)
                from .autograd_path import duration_pitch_autograd
                return duration_pitch_autograd(self, x, encoded_prompts, text_lens=text_lens, prompt_lens=prompt_lens)
            if needs_autograd(self, x if x.is_floating_point() else None):
                raise NotImplementedError(f"{'text_lens' if text_lens is not None else 'prompt_lens'}: per-utterance lengths are a sampling "
                                          f"feature (torch.no_grad()); the training passes take equal-length batches")
            if not x.is_cuda:
                from .autograd_path import duration_pitch_autograd
                with torch.no_grad():
                    return duration_pitch_autograd(self, x, encoded_prompts, text_lens=text_lens, prompt_lens=prompt_lens)
            return self._forward_hip(x, encoded_prompts, text_lens, prompt_lens)
        if needs_autograd(self, x if x.is_floating_point() else None) or not x.is_cuda:
            if self.train_backend == "hip" and x.is_cuda:          # (on the GPU this branch is entered under autograd only)
                from . import training
                if training.available(x.device) and training.duration_pitch_unsupported_reason(self) is None:
                    return training.duration_pitch_forward_train(self, x, encoded_prompts)
            from .autograd_path import duration_pitch_autograd
            return duration_pitch_autograd(self, x, encoded_prompts)
        return self._forward_hip(x, encoded_prompts)

    def refresh_weights(self):
        self._cache.refresh(self.parameters())

    # ------------------------------------------------------------------ HIP path
    def _build_packed(self):
        prec = _PRECISIONS[self.precision]

        def f32(t):
            return t.detach().float().contiguous()

        trunks = []
        for tr in (self.to_duration_pred, self.to_pitch_pred):
            layers = []
            for convs, norm, attn in tr.layers:
                if tr.use_resnet_block:
                    cs = [[(ops.PackedWeight(f32(b.proj.weight), precision=prec), f32(b.proj.bias), f32(b.norm.weight),
                            f32(b.norm.bias), b.norm.num_groups, b.norm.eps) for b in rb.blocks] for rb in convs]
                else:
                    cs = [(ops.PackedWeight(f32(cb[1].weight), precision=prec), f32(cb[1].bias)) for cb in convs]
                layers.append(dict(convs=cs, gamma=f32(norm.gamma), q=ops.PackedWeight(f32(attn.to_q.weight), precision=prec),
                                   kv=ops.PackedWeight(f32(attn.to_kv.weight), precision=prec),
                                   out=ops.PackedWeight(f32(attn.to_out.weight), precision=prec)))
            head = tr.to_pred[0]
            trunks.append(dict(layers=layers, w_pred=f32(head.weight).reshape(-1), b_pred=f32(head.bias)))
        return trunks

    @torch.no_grad()
    def _forward_hip(self, x, encoded_prompts, text_lens=None, prompt_lens=None):
        if self.training and self.dropout > 0:
            raise NotImplementedError("dropout is a training-time feature; the HIP path is inference-only (call .eval(), or run "
                                      "under autograd for the composite)")
        if isinstance(self.phoneme_token_emb, nn.Embedding):
            V = self.phoneme_token_emb.num_embeddings
            if x.is_floating_point() or int(x.min()) < 0 or int(x.max()) >= V:
                raise IndexError(f"phoneme token ids must be integers in [0, {V})")
            x = ops.embedding(x, self.phoneme_token_emb.weight.detach().float().contiguous(), 0)
        b, n, d = x.shape
        np_ = encoded_prompts.shape[1]
        if d != self.dim_hidden or encoded_prompts.shape[-1] != self.dim_hidden or encoded_prompts.shape[0] != b:
            raise ValueError(f"phoneme encodings and encoded prompts must both be [b, *, {self.dim_hidden}] "
                             f"(keys are cat(queries, prompts), NS2:1060-1061); got {tuple(x.shape)} and {tuple(encoded_prompts.shape)}")
        prec = _PRECISIONS[self.precision]
        packed = self._cache.get(self.parameters(), self._build_packed, extra=(self.precision,))
        h0 = x.reshape(b * n, d).float().contiguous()
        p0 = encoded_prompts.reshape(b * np_, d).float().contiguous()
        key_mask = None
        if text_lens is not None or prompt_lens is not None:
            # rows behind a length become zeros once, in copies (the callers' tensors are not written): the "same" convolutions then
            # read what they read behind the end of the utterance alone, and every context row the key mask hides is finite.  ONE byte
            # mask [b, n + n_p] for all layers of both trunks: keys [0, text_lens[i]) and [n, n + prompt_lens[i]), made on the device
            def side(lens_, rows, k):
                if lens_ is None:
                    return rows, torch.ones(b, k, dtype=torch.bool, device=x.device)
                l = ops._front_lens(lens_, b, x.device)
                return ops.zero_rows(rows.clone(), b, k, l), torch.arange(k, device=x.device)[None] < l.clamp(1, k)[:, None]

            (h0, tm), (p0, pm) = side(text_lens, h0, n), side(prompt_lens, p0, np_)
            parts = [tm, pm]
            key_mask = torch.cat(parts, dim=1).to(torch.uint8).contiguous()
            text_lens = None if text_lens is None else ops._front_lens(text_lens, b, x.device)
        # the prompt rows of every attention context, split once: context planes [b, n + n_p] = [norm(x) rows | prompt rows]
        pp = ops.split(p0, precision=prec)
        ctx = ops._out_planes(b * (n + np_), d, x.device, prec)
        ctx.buf.view(b, n + np_, -1)[:, n:].copy_(pp.buf.view(b, np_, -1))
        outs = [self._trunk_hip(tr, h0, b, n, np_, ctx, prec, text_lens, key_mask) for tr in packed]
        if text_lens is not None:
            pad = torch.arange(n, device=x.device)[None] >= text_lens.clamp(1, n)[:, None]
            outs = [o.reshape(b, n).masked_fill(pad, 0.) for o in outs]
        return outs[0].reshape(b, n).to(x.dtype), outs[1].reshape(b, n).to(x.dtype)

    def _trunk_hip(self, tr, h, b, n, np_, ctx, prec, text_lens=None, key_mask=None):
        """text_lens: int32 [b] on the device or None -- rows of h from text_lens[i] on are zeros on entry and after every layer;
        key_mask: uint8 [b, n + np_] or None, the keys of every attention"""
        gn_kw = {} if text_lens is None else dict(lens=text_lens)
        att_kw = {} if key_mask is None else dict(key_mask=key_mask)
        k = self.to_pitch_pred.kernel_size
        H, dh = self.to_pitch_pred.heads, self.to_pitch_pred.dim_head
        conv_kw = dict(conv_taps=k, dilation=1, seq_len=n, pad_left=k // 2, precision=prec)
        for L in tr["layers"]:
            a = ops.split(h, precision=prec)
            if self.to_pitch_pred.use_resnet_block:
                for rb in L["convs"]:                # ResnetBlock: out = silu(gn(conv(... silu(gn(conv(x)))))) + x
                    xin, last = h, len(rb) - 1
                    for j, (pw, cb, gw, gb, groups, eps) in enumerate(rb):
                        y = ops.linear_f32(pw, a, bias=cb, **conv_kw)
                        if j < last:
                            a = ops.groupnorm_silu(y, b, gw, gb, groups, eps, want_f32=False, precision=prec, **gn_kw)
                        else:
                            h, a = ops.groupnorm_silu(y, b, gw, gb, groups, eps, resid=xin, precision=prec, **gn_kw)
            else:
                for i, (pw, cb) in enumerate(L["convs"]):   # ConvBlock: conv + SiLU in the GEMM epilogue
                    if i + 1 < len(L["convs"]):
                        a = ops.linear_split(pw, a, bias=cb, act=1, **conv_kw)
                        if text_lens is not None:            # no GroupNorm here to zero the rows behind the end
                            ops.zero_rows(a, b, n, text_lens)
                    else:
                        h = ops.linear_f32(pw, a, bias=cb, act=1, **conv_kw)
                        if text_lens is not None:
                            ops.zero_rows(h, b, n, text_lens)
            xn = ops.rmsnorm(h, gamma=L["gamma"], precision=prec)
            ctx.buf.view(b, n + np_, -1)[:, :n].copy_(xn.buf.view(b, n, -1))
            inner = H * dh
            q = ops.linear_split(L["q"], xn, precision=prec, out_precision=2 if prec == 4 else None)   # attention operand format
            kk, vt = ops.linear_qkv(L["kv"], ctx, seq_len=n + np_, split_col=inner, precision=prec)
            o = ops.attention(q, kk, vt, b, H, n, n + np_, precision=prec, head_dim=dh, **att_kw)
            h = ops.linear_f32(L["out"], o, resid=h, precision=prec)
            if text_lens is not None:                        # a padding query's output is finite but not 0: the next convolution reads it
                ops.zero_rows(h, b, n, text_lens)
        return ops.row_dot(h, tr["w_pred"], tr["b_pred"], relu=True)
