"""RVQ side of the codec boundary (`EncodecWrapper`, SURVEY §8b "Codec surface") with the residual-VQ encode and
decode running in the HIP kernels of csrc/rvq.hip.

Surface kept for `NaturalSpeech2` (reference call sites in brackets):
    codec.target_sample_hz, .seq_len_multiple_of [NS2:1213-1214], .codebook_dim [NS2:1244], .eval() [NS2:1444, 1610]
    codec(x, return_encoded=True, curtail_from_left=...) -> (emb [b,n,128], codes [b,n,Q] int64, None)   [NS2:1445, 1611]
    codec.decode(emb [b,n,128]) -> waveform [b,1,T]                                                        [NS2:1496-1499]
    codec.rq(x_start, codes) -> (quantized, ce_loss)                                                       [NS2:1682]

The SEANet conv/LSTM encoder and decoder of EnCodec are callables (`encoder`, `decoder`): `from_hf` takes them from a HF
`transformers.EncodecModel` (the in-container stand-in for the un-vendored `encodec` package), by default wrapped
in `seanet.SEANetEncoderHIP / SEANetDecoderHIP` so that waveform <-> latents also runs on the HIP kernels, and
copies its codebooks.  With `encoder=None` the wrapper accepts latents [b, n, 128] directly.
"""
from typing import Callable, Optional

import torch
from torch import nn
import torch.nn.functional as F

from . import ops
from ._cache import PackedCache
from .resample import Resample


RQ_BACKENDS = ("composite", "hip")           # of `codec.rq`, the RVQ cross-entropy term of the training loss


class HipRVQ(nn.Module):
    """EnCodec residual vector quantizer (HFENC:424-447) over `codebooks` [Q, C, 128]."""

    def __init__(self, codebooks: torch.Tensor, tie_eps: float = 1e-4):
        super().__init__()
        assert codebooks.ndim == 3 and codebooks.shape[-1] == 128 and codebooks.shape[1] % 64 == 0
        self.register_buffer("codebooks", codebooks.float().contiguous())
        self.tie_eps = tie_eps
        self._norm = PackedCache()

    def _cb_norm(self):
        return self._norm.get([self.codebooks], lambda: ops.rvq_prepare(self.codebooks))

    @torch.no_grad()
    def encode(self, latents: torch.Tensor):
        """latents [b, n, 128] -> codes [b, n, Q] int64, emb [b, n, 128] (sum of the selected code vectors)."""
        b, n, d = latents.shape
        x = latents.reshape(b * n, d).float().contiguous()
        codes, emb = ops.rvq_encode(x, self.codebooks, self._cb_norm(), tie_eps=self.tie_eps)
        return codes.reshape(b, n, -1), emb.reshape(b, n, d)

    @torch.no_grad()
    def decode(self, codes: torch.Tensor):
        b, n, q = codes.shape
        return ops.rvq_decode(codes.reshape(b * n, q).contiguous(), self.codebooks).reshape(b, n, -1)


class ResidualVQCrossEntropy(nn.Module):
    """`codec.rq(x, indices) -> (quantized_out, ce_loss)`: the training-time cross-entropy of the diffusion model's predicted
    x_start against the codec's own code indices (NS2:1670-1684, off by default: rvq_cross_entropy_loss_weight = 0).

    PARITY UNPINNED: upstream this is `vector_quantize_pytorch.ResidualVQ.forward(x, indices=...)` (setup.py pins only
    `>=1.4.1`, no lock file; not vendored, not installed here).  Restated from its published algorithm: per quantizer the
    logits are the NEGATIVE EUCLIDEAN distances (with the square root) of the running residual to every code, the loss is
    `F.cross_entropy(logits, indices[..., q])`, the residual is reduced by the nearest code (detached), and the layer losses
    are summed.  Differentiable in `x`.

    `backend` (settable; not in the reference): "composite" (default) is the autograd composite below; "hip" runs the term on the fused
    kernel of csrc/rvq_ce.hip through `training.RvqCrossEntropyFn` -- one launch for the loss and its unit gradient, nothing of size
    [b, n, C] kept, no host read (capturable by `training.GraphedTrainStep`), fp32.  It falls back to the composite for what
    `training.rvq_ce_unsupported_reason` names (CPU tensors, non-fp32 `x`, indices that are not int64, no library).  Where the kernel differs:
      * an index outside [0, C) -- the -1 of a dropped-out quantizer included, which the composite asserts against after reading the device
        -- makes the loss NaN (and that row's gradient): loud, without a synchronisation;
      * a residual that equals a code (distance 0) gives the well-defined loss and that code adds 0 to the gradient, where the composite's
        gradient of sqrt at 0 is not finite;
      * the nearest code of a stage is decided by the fp32 scores r.e - |e|^2/2; on a near-tie either code is a valid stage result.

    `forward(x [b, n, d], indices [b, n, Q], lens=)` (not in the reference) is the ragged batch: frames per utterance, integer [b], clamped
    into [1, n].  The loss is the mean over the utterances of each utterance's OWN loss (its cross-entropies averaged over its own
    frames [0, lens[i])), so utterance i adds to it, and to the gradient, what it adds alone divided by b.  What x and indices hold at or
    behind a length -- NaN, -1 -- reaches neither; quantized_out and the gradient are exact zeros there.  backend="hip" runs
    ns2_rvq_ce_lens (include/ns2hip_train.h; no host read, capturable); the composite selects x and indices to 0 behind the lengths
    before use and masks the per-frame cross-entropies with a select."""

    def __init__(self, owner: HipRVQ, backend: str = "composite"):
        super().__init__()
        assert backend in RQ_BACKENDS, f"backend must be one of {RQ_BACKENDS}"
        self._owner = [owner]              # not registered: the codebooks stay owned (and moved) by the HipRVQ
        self.backend = backend

    def forward(self, x, indices, lens=None):
        assert self.backend in RQ_BACKENDS, f"backend must be one of {RQ_BACKENDS}"
        if lens is not None:
            lens = torch.as_tensor(lens)
            if x.ndim != 3 or lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != (x.shape[0],):
                raise ValueError(f"rq(lens=) takes x [b, n, d] and one integer frame count per utterance [b], got {list(x.shape)} and "
                                 f"{lens.dtype} {list(lens.shape)}")
            lens = lens.to(x.device)
        if self.backend == "hip":
            from . import training
            if training.rvq_ce_unsupported_reason(self, x, indices) is None:
                return self._forward_hip(x, indices, lens)
        if lens is not None:
            return self._forward_composite_lens(x, indices, lens)
        return self._forward_composite(x, indices)

    def _forward_hip(self, x, indices, lens=None):
        from .training.functions import RvqCrossEntropyFn
        owner = self._owner[0]
        assert indices.shape[:-1] == x.shape[:-1] and indices.shape[-1] == owner.codebooks.shape[0]
        d = x.shape[-1]
        xr = x.reshape(-1, d)
        extra = () if lens is None else (lens.to(torch.int32).contiguous(),)
        loss, quant = RvqCrossEntropyFn.apply(xr if xr.is_contiguous() else xr.contiguous(), owner.codebooks, owner._cb_norm(),
                                              indices.reshape(-1, indices.shape[-1]), *extra)
        return quant.reshape(x.shape), loss

    def _forward_composite_lens(self, x, indices, lens):
        cb = self._owner[0].codebooks.to(x.dtype)
        assert indices.shape[:-1] == x.shape[:-1] and indices.shape[-1] == cb.shape[0]
        b, n = x.shape[:2]
        ln = lens.long().clamp(1, n)                                             # as the kernel clamps
        keep = torch.arange(n, device=x.device)[None] < ln[:, None]             # [b, n]
        # selects, not products: NaN and -1 may lie behind a length
        x = torch.where(keep[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
        indices = torch.where(keep[..., None], indices, torch.zeros((), dtype=indices.dtype, device=x.device))
        assert not torch.any(indices == -1), "some of the residual vq indices were dropped out"
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        residual, out, ce = x, torch.zeros_like(x), 0.
        for q in range(cb.shape[0]):
            e = cb[q]
            d2 = residual.pow(2).sum(-1, keepdim=True) - 2 * residual @ e.t() + e.pow(2).sum(-1)
            logits = -d2.clamp(min=0).sqrt()                                     # [b, n, C]
            rows = F.cross_entropy(logits.transpose(1, 2), indices[..., q], reduction="none")    # [b, n]
            ce = ce + (torch.where(keep, rows, zero).sum(-1) / ln.to(x.dtype)).mean()            # own frames, then the mean over b
            quantized = F.embedding(logits.argmax(dim=-1), e)
            residual = residual - quantized.detach()
            out = out + quantized
        return torch.where(keep[..., None], out, zero), ce

    def _forward_composite(self, x, indices):
        cb = self._owner[0].codebooks.to(x.dtype)
        assert indices.shape[:-1] == x.shape[:-1] and indices.shape[-1] == cb.shape[0]
        assert not torch.any(indices == -1), "some of the residual vq indices were dropped out"
        residual, out, ce = x, torch.zeros_like(x), 0.
        for q in range(cb.shape[0]):
            e = cb[q]
            d2 = residual.pow(2).sum(-1, keepdim=True) - 2 * residual @ e.t() + e.pow(2).sum(-1)
            logits = -d2.clamp(min=0).sqrt()                                     # [b, n, C]
            ce = ce + F.cross_entropy(logits.transpose(1, 2), indices[..., q], ignore_index=-1)
            quantized = F.embedding(logits.argmax(dim=-1), e)
            residual = residual - quantized.detach()
            out = out + quantized
        return out, ce


class EncodecWrapperHIP(nn.Module):
    target_sample_hz = 24000
    seq_len_multiple_of = 320          # strides 2*4*5*8
    codebook_dim = 128
    # The SEANet encoder is causal, but its reflect padding mirrors the first rows of an utterance: the last convolution (k = 7, at the
    # frame rate) reads frames 1 .. 6 for its prefix.  A prompt of a padded batch keeps its padding out of its frames only from this
    # many frames on (NaturalSpeech2.sample(prompt_lens=) with a raw-audio prompt checks it); the HIP encoder takes no shorter input.
    min_causal_prompt_frames = 7

    def __init__(self, codebooks: torch.Tensor, encoder: Optional[Callable] = None, decoder: Optional[Callable] = None,
                 rq_backend: str = "composite"):
        """rq_backend (not in the reference): the backend of `self.rq`, the RVQ cross-entropy term (`ResidualVQCrossEntropy`)"""
        super().__init__()
        self._hip_codec_init(codebooks, encoder, decoder, rq_backend)

    def _hip_codec_init(self, codebooks, encoder=None, decoder=None, rq_backend="composite"):
        """everything but nn.Module's own set-up: compat.hip_backed_codec_class builds a subclass of the REFERENCE's codec class whose
        own __init__ (it fetches pretrained EnCodec weights) must not run"""
        self.rvq = HipRVQ(codebooks)
        self.rq = ResidualVQCrossEntropy(self.rvq, backend=rq_backend)
        self.encoder, self.decoder = encoder, decoder

    @classmethod
    def from_hf(cls, hf_model, num_quantizers: int = 8, hip_seanet: bool = True, precision: str = "exact", rq_backend: str = "composite"):
        """wire a `transformers.EncodecModel`'s SEANet encoder / decoder and its first `num_quantizers` codebooks (6 kbps at
        24 kHz = 8, what audiolm's EncodecWrapper uses).  hip_seanet=True (default): the SEANet stacks run on the HIP kernels
        (seanet.py) with the model's own (weight-normalised) parameters; False: HF's PyTorch modules are called as they are."""
        layers = list(hf_model.quantizer.layers)[:num_quantizers]
        cbs = torch.stack([l.codebook.embed.detach().float() for l in layers])
        enc, dec = hf_model.encoder, hf_model.decoder
        if hip_seanet:
            from .seanet import SEANetDecoderHIP, SEANetEncoderHIP
            enc, dec = SEANetEncoderHIP(enc, precision=precision), SEANetDecoderHIP(dec, precision=precision)
        return cls(cbs, encoder=enc, decoder=dec, rq_backend=rq_backend)

    @property
    def num_quantizers(self):
        return self.rvq.codebooks.shape[0]

    def refresh_weights(self):
        """run-boundary content check of everything this wrapper packed (SEANet stacks, codebook norms): an EMA copy of the whole
        `NaturalSpeech2` (NS2:1793) rewrites these through `.data`"""
        for m in (self.encoder, self.decoder):
            if hasattr(m, "refresh_weights"):
                m.refresh_weights()
        self.rvq._norm.refresh([self.rvq.codebooks])

    @torch.no_grad()
    def forward(self, x, return_encoded=True, curtail_from_left=False, input_sample_hz=None, **kwargs):
        """x: raw audio [b, t] (needs `encoder`) or latents [b, n, 128] -> (emb [b,n,128], codes [b,n,Q], None).
        input_sample_hz (audiolm_pytorch's keyword): the rate of the raw audio; another rate than `target_sample_hz` is resampled
        (resample.py) before the audio is curtailed.  Latents have no rate: with them a foreign rate is a ValueError."""
        foreign = input_sample_hz is not None and int(input_sample_hz) != int(self.target_sample_hz)
        if foreign and x.ndim != 2:
            raise ValueError(f"input_sample_hz={input_sample_hz} with latents {list(x.shape)}: only raw audio [b, t] has a sample rate to "
                             f"convert to {self.target_sample_hz}")
        if x.ndim == 2:
            if self.encoder is None:
                raise RuntimeError("raw audio needs the SEANet encoder (out of scope of the HIP path): pass encoder=")
            if foreign:
                x = Resample(int(input_sample_hz), int(self.target_sample_hz))(x)
            t = x.shape[-1] // self.seq_len_multiple_of * self.seq_len_multiple_of
            if t == 0:
                raise ValueError(f"audio shorter than one codec frame ({self.seq_len_multiple_of} samples)")   # x[..., -0:] would keep everything
            x = x[..., -t:] if curtail_from_left else x[..., :t]
            latents = self.encoder(x[:, None]).transpose(1, 2)       # [b, 128, n] -> [b, n, 128]
        else:
            latents = x
        codes, emb = self.rvq.encode(latents)
        return emb, codes, None

    @torch.no_grad()
    def decode(self, emb):
        if self.decoder is None:
            raise RuntimeError("waveform decode needs the SEANet decoder (out of scope of the HIP path): pass decoder=")
        return self.decoder(emb.transpose(1, 2))
