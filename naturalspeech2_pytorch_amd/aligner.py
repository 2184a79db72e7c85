"""`Aligner` (aligner.py of the reference: AlignerNet, maximum_path, ForwardSumLoss, BinLoss, Aligner) and the pieces of the
text-conditioned training pass around it (utils.py:4-33, NS2:1449-1455, 1524-1602).

With no gradient wanted and CUDA tensors (`transformer.needs_autograd`), `Aligner` runs csrc/aligner.hip: the convolutions are
the shifted-row GEMMs (conv_taps = 3, pad_left = 1, and plain 1x1 products) with a ReLU + split kernel between them, then one
kernel for the distances + mask + softmax and the monotonic alignment search `ns2_maximum_path`.  Otherwise the PyTorch
composite of autograd_path.py runs; its alignment search is HIP on CUDA and a PyTorch loop on the CPU.  The HIP path takes
prefix masks (what `create_mask` builds): masks passed to the public module are reduced to lengths once (one host read) and
any other mask goes to the composite.  Same constructor keywords, forward signatures, outputs and state_dict keys as the reference.

Training.  By default (`train_backend="composite"`, `backend="composite"` of the two losses) the Aligner under autograd is the PyTorch
composite and the losses are PyTorch (CTC is torch's).  With `train_backend="hip"` on the GPU `training.aligner_forward_train` runs forward
and backward on the HIP kernels, and `ForwardSumLoss` / `BinLoss` with `backend="hip"` are autograd Functions over
ns2_align_losses_fwd / _bwd: int lengths on the device, no host read anywhere.
"""
import torch
from torch import nn
import torch.nn.functional as F

from . import ops
from ._cache import PackedCache
from .model import _PRECISIONS
from .transformer import needs_autograd


def create_mask(lengths, max_len):
    """utils.py:28-33: [b] lengths -> [b, max_len] prefix mask"""
    return torch.arange(max_len, dtype=lengths.dtype, device=lengths.device)[None] < lengths[:, None]


def prefix_lengths(mask):
    """lengths [b] int32 of a prefix mask [b, t] (or [b, 1, t]), or None when the mask is not a prefix mask (one host read)"""
    m = mask.reshape(mask.shape[0], mask.shape[-1]).bool()
    lens = m.sum(-1).to(torch.int32)
    return lens if bool((create_mask(lens, m.shape[-1]) == m).all()) else None


def _product_lengths(mask):
    """(text_lens, mel_lens) of attn_mask = x_mask * y_mask [b, t_x, t_y] built from prefix masks, or None"""
    m = mask.bool()
    tl = m.any(2).sum(1).to(torch.int32)
    ml = m.any(1).sum(1).to(torch.int32)
    ref = create_mask(tl, m.shape[1])[:, :, None] & create_mask(ml, m.shape[2])[:, None, :]
    return (tl, ml) if bool((ref == m).all()) else None


def maximum_path(value, mask, const=None):
    """aligner.py:97-130: the monotonic alignment path [b, t_x, t_y] of `value` under `mask`.  fp32 CUDA input with a mask made
    of prefix masks: `ns2_maximum_path`, bit for bit the reference's; otherwise the PyTorch loop of autograd_path.py."""
    if value.is_cuda and const is None and value.dtype == torch.float32:
        lens = _product_lengths(mask)
        if lens is not None:
            return ops.maximum_path(value.contiguous(), *lens)[0]
    from .autograd_path import maximum_path_composite
    return maximum_path_composite(value, mask, const)


class AlignerNet(nn.Module):
    """alignment model (aligner.py:17-60); `forward` is the differentiable composite"""

    def __init__(self, dim_in=80, dim_hidden=512, attn_channels=80, temperature=0.0005):
        super().__init__()
        self.temperature = temperature
        self.key_layers = nn.ModuleList([
            nn.Conv1d(dim_hidden, dim_hidden * 2, kernel_size=3, padding=1, bias=True),
            nn.ReLU(inplace=True),
            nn.Conv1d(dim_hidden * 2, attn_channels, kernel_size=1, padding=0, bias=True)])
        self.query_layers = nn.ModuleList([
            nn.Conv1d(dim_in, dim_in * 2, kernel_size=3, padding=1, bias=True),
            nn.ReLU(inplace=True),
            nn.Conv1d(dim_in * 2, dim_in, kernel_size=1, padding=0, bias=True),
            nn.ReLU(inplace=True),
            nn.Conv1d(dim_in, attn_channels, kernel_size=1, padding=0, bias=True)])

    def forward(self, queries, keys, mask=None):
        from .autograd_path import aligner_net_autograd
        return aligner_net_autograd(self, queries, keys, mask)


TRAIN_BACKENDS = ("composite", "hip")


def _i32(lens, device):
    return lens.to(device=device, dtype=torch.int32).contiguous()


class _ForwardSumFn(torch.autograd.Function):
    """the forward-sum loss on ns2_align_losses_fwd / _bwd: aln_log [b, 1, T, n], int32 lengths on the device -> a 0-dim loss"""

    @staticmethod
    def forward(ctx, logp, key_lens, query_lens, blank):
        from .training import backend
        ctx.bk = bk = backend()
        x = logp.detach().float().contiguous()
        loss, _, ws = bk.align_losses_fwd(x, key_lens, query_lens, blank, want_fs=True)
        ctx.save_for_backward(x, key_lens, query_lens, ws)
        ctx.blank, ctx.dtype = blank, logp.dtype
        return loss.to(logp.dtype)

    @staticmethod
    def backward(ctx, g):
        x, key_lens, query_lens, ws = ctx.saved_tensors
        d = ctx.bk.align_losses_bwd(x, key_lens, query_lens, ctx.blank, ws, g_fs=g.detach().float().reshape(1).contiguous())
        return d.to(ctx.dtype), None, None, None


class _BinFn(torch.autograd.Function):
    """the bin loss on the same kernels: hard [b, n, T] 0/1, aln_log [b, 1, T, n] -> a 0-dim loss (no gradient for `hard`: it is a path)"""

    @staticmethod
    def forward(ctx, hard, logp, key_lens):
        from .training import backend
        ctx.bk = bk = backend()
        x, h = logp.detach().float().contiguous(), hard.detach().float().contiguous()
        _, loss, ws = bk.align_losses_fwd(x, key_lens, None, 0., hard=h, want_fs=False, want_bin=True)
        ctx.save_for_backward(x, h, key_lens, ws)
        ctx.dtype = logp.dtype
        return loss.to(logp.dtype)

    @staticmethod
    def backward(ctx, g):
        x, h, key_lens, ws = ctx.saved_tensors
        d = ctx.bk.align_losses_bwd(x, key_lens, None, 0., ws, hard=h, g_bin=g.detach().float().reshape(1).contiguous())
        return None, d.to(ctx.dtype), None


def _hip_loss_ok(logp):
    return logp.is_cuda and logp.shape[-1] <= 1024 and logp.shape[-2] <= 8192


class ForwardSumLoss(nn.Module):
    """aligner.py:132-167: CTC over the alignment log-probabilities, blank = a constant column in front.  `backend="hip"` (not in the
    reference): CUDA tensors take the kernels of csrc/aligner.hip (no host read of the lengths); CPU tensors always take the composite"""

    def __init__(self, blank_logprob=-1, backend="composite"):
        super().__init__()
        assert backend in TRAIN_BACKENDS, f"backend must be one of {TRAIN_BACKENDS}"
        self.blank_logprob, self.backend = blank_logprob, backend
        self.ctc_loss = nn.CTCLoss(blank=0, zero_infinity=True)

    def forward(self, attn_logprob, key_lens, query_lens):
        if self.backend == "hip" and _hip_loss_ok(attn_logprob):
            dev = attn_logprob.device
            return _ForwardSumFn.apply(attn_logprob, _i32(key_lens, dev), _i32(query_lens, dev), float(self.blank_logprob))
        n = attn_logprob.shape[-1]
        lp = F.pad(attn_logprob[:, 0].permute(1, 0, 2), (1, 0), value=self.blank_logprob)      # [T, b, n + 1]
        cols = torch.arange(n + 1, device=lp.device)
        lp = lp.masked_fill(cols[None, None] > key_lens[None, :, None], -torch.finfo(lp.dtype).max).log_softmax(-1)
        targets = torch.arange(1, n + 1, device=lp.device)[None].expand(key_lens.numel(), n)
        return self.ctc_loss(lp, targets, query_lens, key_lens)


class BinLoss(nn.Module):
    """aligner.py:169-183 (the reference fills the caller's attn_logprob in place; this one works on a copy).  `backend`: as ForwardSumLoss"""

    def __init__(self, backend="composite"):
        super().__init__()
        assert backend in TRAIN_BACKENDS, f"backend must be one of {TRAIN_BACKENDS}"
        self.backend = backend

    def forward(self, attn_hard, attn_logprob, key_lens):
        if self.backend == "hip" and _hip_loss_ok(attn_logprob):
            return _BinFn.apply(attn_hard, attn_logprob, _i32(key_lens, attn_logprob.device))
        b, n = attn_logprob.shape[0], attn_logprob.shape[-1]
        lp = attn_logprob[:, 0].permute(1, 0, 2)                                                # [T, b, n]
        cols = torch.arange(n, device=lp.device)
        lp = lp.masked_fill(cols[None, None] > key_lens[None, :, None], -torch.finfo(lp.dtype).max).log_softmax(-1)
        return (attn_hard.permute(2, 0, 1) * lp).sum() / b


class Aligner(nn.Module):
    """aligner.py:185-229.  forward(x [b, n, dim_hidden] phoneme encodings, x_mask [b, 1, n], y [b, dim_in, T] mel,
    y_mask [b, 1, T]) -> (aln_hard int32 [b, n], aln_soft [b, n, T], aln_log [b, 1, T, n], aln_mask [b, n, T])"""

    def __init__(self, dim_in, dim_hidden, attn_channels=80, temperature=0.0005, precision="exact", train_backend="composite"):
        super().__init__()
        assert precision in _PRECISIONS, f"precision must be one of {sorted(_PRECISIONS)}"
        assert train_backend in TRAIN_BACKENDS, f"train_backend must be one of {TRAIN_BACKENDS}"
        self.train_backend = train_backend  # not in the reference: "hip" = forward and backward on the HIP kernels (training/aligner_pass.py)
        self.dim_in, self.dim_hidden, self.attn_channels, self.temperature = dim_in, dim_hidden, attn_channels, temperature
        self.precision = precision          # not in the reference: arithmetic of the HIP convolutions
        self.aligner = AlignerNet(dim_in=dim_in, dim_hidden=dim_hidden, attn_channels=attn_channels, temperature=temperature)
        self._cache = PackedCache(fingerprint_every=1)

    def forward(self, x, x_mask, y, y_mask):
        if not needs_autograd(self, x) and x.is_cuda:
            tl, ml = prefix_lengths(x_mask), prefix_lengths(y_mask)
            if tl is not None and ml is not None:
                return self.forward_lengths(x, tl, y, ml)
        elif self.train_backend == "hip" and x.is_cuda:            # (on the GPU this branch is entered under autograd only)
            if self.train_ready(x, y):
                tl, ml = prefix_lengths(x_mask), prefix_lengths(y_mask)
                if tl is not None and ml is not None:
                    return self.forward_lengths_train(x, tl, y, ml)
        return self._forward_composite(x, x_mask, y, y_mask)

    def train_ready(self, x, y):
        """does the HIP training pass take these inputs (`train_backend="hip"`, CUDA, nothing `aligner_unsupported_reason` names)"""
        if self.train_backend != "hip" or not x.is_cuda:
            return False
        from . import training
        return training.available(x.device) and training.aligner_unsupported_reason(self, x, y) is None

    def forward_lengths_train(self, x, text_lens, y, mel_lens):
        """the differentiable HIP path with int lengths [b] on the device in place of the masks (no host read).  -> as forward"""
        if x.shape[-1] != self.dim_hidden or y.shape[1] != self.dim_in or x.shape[0] != y.shape[0]:
            raise ValueError(f"expected phoneme encodings [b, n, {self.dim_hidden}] and mel [b, {self.dim_in}, T]; got "
                             f"{tuple(x.shape)} and {tuple(y.shape)}")
        from . import training
        return training.aligner_forward_train(self, x, text_lens, y, mel_lens)

    def _forward_composite(self, x, x_mask, y, y_mask):
        soft, logp = self.aligner(y, x.transpose(1, 2), x_mask)
        attn_mask = (x_mask[..., :, None] * y_mask[..., None, :])[:, 0]
        soft = soft[:, 0].transpose(1, 2)
        path = maximum_path(soft.detach() if soft.is_cuda else soft, attn_mask)
        return path.sum(-1).int(), soft, logp, path

    def refresh_weights(self):
        self._cache.refresh(self.parameters())

    def _build_packed(self):
        prec = _PRECISIONS[self.precision]

        def f32(t):
            return t.detach().float().contiguous()

        def conv(c):
            w = f32(c.weight)
            return ops.PackedWeight(w if w.shape[-1] > 1 else w[..., 0].contiguous(), precision=prec), f32(c.bias)

        net = self.aligner
        return dict(keys=[conv(net.key_layers[i]) for i in (0, 2)], queries=[conv(net.query_layers[i]) for i in (0, 2, 4)])

    @torch.no_grad()
    def forward_lengths(self, x, text_lens, y, mel_lens):
        """the HIP path with int lengths [b] on the device in place of the masks (no host read).  -> as forward"""
        if x.shape[-1] != self.dim_hidden or y.shape[1] != self.dim_in or x.shape[0] != y.shape[0]:
            raise ValueError(f"expected phoneme encodings [b, n, {self.dim_hidden}] and mel [b, {self.dim_in}, T]; got "
                             f"{tuple(x.shape)} and {tuple(y.shape)}")
        prec = _PRECISIONS[self.precision]
        packed = self._cache.get(self.parameters(), self._build_packed, extra=(self.precision,))
        b, n, _ = x.shape
        T = y.shape[-1]
        text_lens = text_lens.to(device=x.device, dtype=torch.int32)
        mel_lens = mel_lens.to(device=x.device, dtype=torch.int32)

        def stack(h, layers, seq_len):
            a = ops.split(h, precision=prec)
            for i, (pw, bias) in enumerate(layers):
                kw = dict(conv_taps=3, dilation=1, seq_len=seq_len, pad_left=1) if i == 0 else {}
                h = ops.linear_f32(pw, a, bias=bias, precision=prec, **kw)
                if i + 1 < len(layers):
                    a = ops.relu_split(h, precision=prec)
            return h

        keys = stack(x.reshape(b * n, -1).float().contiguous(), packed["keys"], n)
        queries = stack(y.transpose(1, 2).reshape(b * T, -1).float().contiguous(), packed["queries"], T)
        log, soft = ops.align_attn(queries, keys, text_lens, b)
        path, hard = ops.maximum_path(soft, text_lens, mel_lens)
        return hard, soft, log, path


def average_over_durations(values, durs):
    """utils.py:4-26: values [b, 1, T], durs [b, n] -> [b, 1, n], the mean of the non-zero frames of each phoneme (0 where
    there is none), from fp32 prefix sums.  HIP (ns2_average_over_durations) on CUDA for one formant."""
    if values.is_cuda and values.shape[1] == 1 and values.dtype == torch.float32:
        return ops.average_over_durations(values[:, 0].contiguous(), durs)[:, None]
    from .autograd_path import average_over_durations_composite
    return average_over_durations_composite(values, durs)


class _Expand(torch.autograd.Function):
    """expand_encodings (NS2:1449-1455) with the hard alignment as durations: ns2_length_regulate forward, ns2_expand_backward
    backward (fixed-order sums, no atomics)"""

    @staticmethod
    def forward(ctx, enc, table, duration, pitch, n_frames):
        ctx.save_for_backward(duration, pitch)
        ctx.n_bins = table.shape[0]
        return ops.expand_frames(duration, pitch, enc.detach().float().contiguous(), table.detach().float().contiguous(), n_frames)

    @staticmethod
    def backward(ctx, g):
        duration, pitch = ctx.saved_tensors
        d_enc, d_table = ops.expand_backward(g.float().contiguous(), duration, pitch,
                                             ctx.n_bins if ctx.needs_input_grad[1] else None)
        return (d_enc if ctx.needs_input_grad[0] else None), d_table, None, None, None


def expand_encodings(phoneme_enc, aln_hard, aln_mask, pitch, pitch_table):
    """cond [b, D, T_mel] = the frames of each phoneme's encoding + pitch embedding (NS2:1449-1455).  phoneme_enc [b, n, D],
    aln_hard [b, n] int, aln_mask [b, n, T_mel] (the 0/1 path), pitch [b, n] (averaged).  On CUDA the length regulator and
    its backward kernel; on the CPU the reference's 0/1 einsum."""
    if phoneme_enc.is_cuda:
        return _Expand.apply(phoneme_enc, pitch_table, aln_hard.float().contiguous(), pitch.float().contiguous(), aln_mask.shape[-1])
    from .autograd_path import expand_with_path
    return expand_with_path(phoneme_enc, aln_mask, pitch, pitch_table)
