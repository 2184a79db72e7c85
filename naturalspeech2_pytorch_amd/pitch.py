"""PitchExtractor: raw audio -> F0 per mel frame, the input `forward(text=...)` needs as `pitch`.

The reference calls pyworld (dio + stonemask) on the CPU, one utterance at a time, inside every training forward (NS2:132-162,
1546-1559); its alternative, torchaudio's compute_kaldi_pitch, is no longer shipped.  This module is NOT a port of either: it is
an estimator of its own, YIN (de Cheveigne & Kawahara, "YIN, a fundamental frequency estimator for speech and music", JASA 2002,
steps 1-5), and no parity with pyworld or Kaldi is claimed or testable.  What it keeps is the contract of the rest of `forward`:
one value per AudioToMel frame (T = 1 + L // hop_length), in Hz, 0 for unvoiced frames (what `f0_to_coarse` and
`average_over_durations` expect).

The formula, for audio x[0 .. L) in fp32, with

    tau_min = floor(sample_rate / f0_ceil)    tau_max = ceil(sample_rate / f0_floor)    W = 2 tau_max    S = 3 tau_max

    frame i reads the S samples from s_i = i hop_length - S // 2; samples outside [0, L) are 0
    d(tau)  = sum_{j=0}^{W-1} (x[s_i + j] - x[s_i + j + tau])^2,  tau = 1 .. tau_max      (direct form: the autocorrelation identity cancels)
    c(tau)  = sum_{k=1}^{tau} d(k)
    d'(tau) = d(tau) * tau / c(tau) where c(tau) > 0, else 1
    tau     = the first of tau_min .. tau_max with d'(tau) < threshold; none: the frame is unvoiced, f0 = 0.  Otherwise, while
              tau < tau_max and d'(tau + 1) < d'(tau), advance tau
    den     = y0 - 2 y1 + y2 with y0, y1, y2 = d'(tau - 1), d'(tau), d'(tau + 1)
    delta   = clamp(0.5 (y0 - y2) / den, -1, 1) if tau + 1 <= tau_max and den > 0, else 0
    f0      = sample_rate / (tau + delta)

Consequences: the first and last few frames of an utterance see the zero padding and come out unvoiced, and audio shorter than
about one span (S samples, 42 ms at the defaults) is all unvoiced.

On a GPU, `forward` runs one HIP kernel (csrc/pitch.hip: ns2_pitch_yin) when 2 <= tau_min < tau_max <= 1024.  Any other
configuration, the CPU, and audio that requires grad take the vectorised PyTorch composite of the same formula below.  The output
never carries a gradient (the reference's pitch does not either).  The composite is a fallback and a yardstick, not a path for
training batches: it materialises every (frame, lag, sample) difference, about 32 MiB per pass of a Python loop (36 frames at the
defaults, some 1800 passes for 32 utterances of 13.6 s).  The module has no parameters and no buffers, and `forward`
reads nothing back from the device.

`forward(audio, lens=)` is the ragged batch: sample counts per utterance, integer [b].  Frame t of utterance i reads zeros outside
[0, lens[i]), so frames t < T_i = 1 + lens[i] // hop_length are those of the module on `audio[i, :lens[i]]` alone, and frames from T_i
on are exactly 0 (unvoiced).  On a GPU that is ns2_pitch_yin_lens (include/ns2hip_audio.h): the lengths stay on the device and a
value outside [1, L] is clamped into it.  The composite does the same per utterance (slice, compute, zero-fill) and reads the lengths.
"""
import math

import torch
from torch import nn
import torch.nn.functional as F

from . import ops

TAU_MAX_HIP = 1024          # csrc/ns2_kernels.h PITCH_TAU_MAX


def yin_lags(sample_rate: int, f0_floor: float, f0_ceil: float):
    """(tau_min, tau_max) of the search"""
    return int(math.floor(sample_rate / f0_ceil)), int(math.ceil(sample_rate / f0_floor))


def yin_frames(x: torch.Tensor, hop_length: int, tau_max: int) -> torch.Tensor:
    """x [N, L] -> the zero-padded spans [N, 1 + L // hop_length, 3 tau_max] (a view of one padded copy)"""
    L, S = x.shape[-1], 3 * tau_max
    T = 1 + L // hop_length
    right = max(0, (T - 1) * hop_length - S // 2 + S - L)
    return F.pad(x, (S // 2, right)).unfold(-1, S, hop_length)[:, :T]


def yin_composite(x: torch.Tensor, sample_rate: int, hop_length: int, tau_min: int, tau_max: int, threshold: float):
    """the module docstring's formula on x [N, L] fp32 in plain tensor operations -> (f0 [N, T] fp32, tau [N, T] int64, 0 unvoiced)"""
    assert x.ndim == 2 and x.shape[-1] >= 1 and 2 <= tau_min < tau_max
    W = 2 * tau_max
    frames = yin_frames(x, hop_length, tau_max)
    N, T, S = frames.shape
    frames = frames.reshape(N * T, S)
    step = max(1, (1 << 23) // (tau_max * W))                    # frames per pass: the [n, tau_max, W] differences stay near 32 MiB
    d = []
    for n0 in range(0, N * T, step):
        win = frames[n0:n0 + step].unfold(-1, W, 1)              # [n, tau_max + 1, W]: window tau starts at sample tau
        diff = win[:, :1] - win[:, 1:]
        d.append((diff * diff).sum(-1))
    d = torch.cat(d)                                             # [N T, tau_max]: column k is tau = k + 1
    taus = torch.arange(1, tau_max + 1, device=x.device)
    c = torch.cumsum(d, -1)
    dp = torch.where(c > 0, d * taus.to(d.dtype) / c, torch.ones_like(d))
    below = (dp < threshold) & (taus >= tau_min)
    voiced = below.any(-1)
    first = below.to(torch.int32).argmax(-1)                     # the first True (0 where there is none: masked by `voiced`)
    lower_next = torch.cat((dp[:, 1:] < dp[:, :-1], torch.zeros_like(below[:, :1])), -1)
    k = (~lower_next & (taus - 1 >= first[:, None])).to(torch.int32).argmax(-1)
    y0 = dp.gather(-1, (k - 1).clamp(min=0)[:, None])[:, 0]
    y1 = dp.gather(-1, k[:, None])[:, 0]
    y2 = dp.gather(-1, (k + 1).clamp(max=tau_max - 1)[:, None])[:, 0]
    den = y0 - 2 * y1 + y2
    ok = (k + 1 <= tau_max - 1) & (den > 0)
    delta = torch.where(ok, (0.5 * (y0 - y2) / den).clamp(-1, 1), torch.zeros_like(den))
    tau = k + 1
    f0 = torch.where(voiced, float(sample_rate) / (tau.to(d.dtype) + delta), torch.zeros_like(den))
    return f0.reshape(N, T), torch.where(voiced, tau, torch.zeros_like(tau)).reshape(N, T)


class PitchExtractor(nn.Module):
    def __init__(self, *, sample_rate=24000, hop_length=160, f0_floor=71., f0_ceil=640., threshold=0.1):
        super().__init__()
        assert sample_rate >= 1 and hop_length >= 1 and 0 < f0_floor < f0_ceil
        self.sample_rate = sample_rate
        self.hop_length = hop_length
        self.f0_floor = f0_floor
        self.f0_ceil = f0_ceil
        self.threshold = threshold
        self.tau_min, self.tau_max = yin_lags(sample_rate, f0_floor, f0_ceil)
        assert 2 <= self.tau_min < self.tau_max, f"the lags must satisfy 2 <= tau_min < tau_max, got {self.tau_min}, {self.tau_max}"

    def hip_supported(self) -> bool:
        return self.tau_max <= TAU_MAX_HIP

    def forward(self, audio: torch.Tensor, lens=None) -> torch.Tensor:
        """audio [..., L] -> f0 [..., 1 + L // hop_length] fp32, Hz, 0 where unvoiced; never carries a gradient.
        lens: sample counts [b] of a ragged batch [b, L] (module docstring)"""
        grad = audio.requires_grad and torch.is_grad_enabled()    # under autograd: the composite, as AudioToMel does
        if lens is not None:
            lens = torch.as_tensor(lens)
            if audio.ndim != 2 or lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != (audio.shape[0],):
                raise ValueError(f"PitchExtractor(lens=) takes audio [b, L] and one integer sample count per utterance [b], got "
                                 f"{list(audio.shape)} and {lens.dtype} {list(lens.shape)}")
        with torch.no_grad():
            return self._forward(audio.detach().float(), grad, lens)

    def _forward(self, audio, grad, lens=None):
        shape = audio.shape
        if shape[-1] < 1:
            raise ValueError("PitchExtractor needs at least one sample")
        x = audio.reshape(-1, shape[-1])
        T = 1 + shape[-1] // self.hop_length
        if x.shape[0] == 0:
            return audio.new_zeros(shape[:-1] + (T,))
        args = (self.sample_rate, self.hop_length, self.tau_min, self.tau_max, self.threshold)
        if lens is not None and x.is_cuda and not grad and self.hip_supported():
            f0 = ops.pitch_yin(x.contiguous(), *args, lens=lens.to(x.device))
        elif lens is not None:                                    # per utterance: slice, the composite, zero-fill (reads the lengths)
            f0 = x.new_zeros(x.shape[0], T)
            for i, s in enumerate(lens.tolist()):
                s = min(max(int(s), 1), shape[-1])                # as the kernel clamps
                f0[i, :1 + s // self.hop_length] = yin_composite(x[i:i + 1, :s], *args)[0][0]
        elif x.is_cuda and not grad and self.hip_supported():
            f0 = ops.pitch_yin(x.contiguous(), *args)
        else:
            f0 = yin_composite(x, *args)[0]
        return f0.reshape(shape[:-1] + (T,))
