"""AudioToMel: raw audio -> mel frames, the reference's `AudioToMel` (NS2:181-224) without torchaudio.

The reference builds `T.Spectrogram`, `T.MelScale` and `T.AmplitudeToDB` inside every `forward`, on the CPU.  The same
arithmetic, written out:

    X     = torch.stft(audio, n_fft, hop_length, win_length, window=hann_window(win_length), center=True, pad_mode="reflect",
                       onesided=True, normalized=False)          the window zero-padded centred to n_fft
    power = |X|^2
    mel   = fb^T @ power                                         fb = mel_filterbank(...): melscale_fbanks(f_min=0, norm=None, "htk")
    out   = 10 log10(clamp(mel, min=1e-10))                      if log (AmplitudeToDB(stype="power", top_db=None), ref 1)

On a GPU, `forward` runs one HIP kernel (csrc/audio_to_mel.hip: ns2_audio_to_mel) when n_fft is a power of two in
[256, 2048], win_length <= n_fft, hop_length <= n_fft and n_mels <= 256.  Any other configuration, the CPU, and audio that
requires grad (under autograd) take the PyTorch composite above.  The module has no parameters and no buffers: the kernel's
tables (window, twiddles, compact filterbank) are cached per device and configuration, so `forward` makes no device -> host
synchronisation after the first call on a device.

`forward(audio, lens=)` (not in the reference) is the ragged batch: sample counts per utterance, integer [b].  Utterance i's frames
t < T_i = 1 + lens[i] // hop_length are those of the module on `audio[i, :lens[i]]` alone -- the reflect padding mirrors about the
utterance's own last sample, not about the end of the batch -- and frames from T_i on are exactly 0 (padding, not the -100 dB of
silence).  On a GPU that is ns2_audio_to_mel_lens (include/ns2hip_audio.h): the lengths stay on the device, nothing reads them on
the host, and a value outside [n_fft // 2 + 1, L] is clamped into it.  Elsewhere a composite does the same per utterance (slice, today's
composite, zero-fill), which reads the lengths.
"""
import math

import torch
from torch import nn

from . import ops


def mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, dtype=torch.float32) -> torch.Tensor:
    """[n_freqs, n_mels]: torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None,
    mel_scale="htk"), built as torchaudio builds it (bin frequencies and mel points by linspace, triangular slopes).  The one
    table of this module: the composite uses it as it is, the HIP plan stores it compactly."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))


def padded_hann(win_length: int, n_fft: int, dtype=torch.float64) -> torch.Tensor:
    """the periodic Hann window of torch.hann_window(win_length), zero-padded centred to n_fft as torch.stft pads it"""
    n = torch.arange(win_length, dtype=torch.float64)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / win_length)
    left = (n_fft - win_length) // 2
    return torch.nn.functional.pad(w, (left, n_fft - win_length - left)).to(dtype)


def _hip_supported(n_fft, win_length, hop_length, n_mels) -> bool:
    return n_fft & (n_fft - 1) == 0 and 256 <= n_fft <= 2048 and 1 <= win_length <= n_fft and 1 <= hop_length <= n_fft \
        and 1 <= n_mels <= 256


_PLANS = {}


def _plan(device, n_fft, win_length, n_mels, sampling_rate, f_max):
    """device tables of ns2_audio_to_mel, built once per (device, configuration): copied from pinned memory without a sync"""
    key = (device, n_fft, win_length, n_mels, sampling_rate, f_max)
    plan = _PLANS.get(key)
    if plan is None:
        fb = mel_filterbank(n_fft // 2 + 1, 0., f_max, n_mels, sampling_rate)      # [n_freqs, n_mels]
        meta, weights, n_bins = [[], [], []], [], 1
        for m in range(n_mels):
            nz = torch.nonzero(fb[:, m]).flatten()
            first, count = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.numel() else (0, 0)
            meta[0].append(first)
            meta[1].append(count)
            meta[2].append(len(weights))
            weights += fb[first:first + count, m].tolist()
            n_bins = max(n_bins, first + count)
        k = torch.arange(n_fft, dtype=torch.float64) * (-2 * math.pi / n_fft)
        host = dict(window=padded_hann(win_length, n_fft, torch.float32),
                    twiddle=torch.stack((torch.cos(k), torch.sin(k)), -1).float(),
                    meta=torch.tensor(meta, dtype=torch.int32),
                    weights=torch.tensor(weights or [0.], dtype=torch.float32))
        plan = {name: t.pin_memory().to(device, non_blocking=True) for name, t in host.items()}
        plan.update(n_w=len(weights), n_bins=n_bins, host=host)     # host: pinned sources kept alive with the plan
        _PLANS[key] = plan
    return plan


class AudioToMel(nn.Module):
    def __init__(self, *, n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, win_length=640, hop_length=160, log=True):
        super().__init__()
        self.log = log
        self.n_mels = n_mels
        self.n_fft = n_fft
        self.f_max = f_max
        self.win_length = win_length
        self.hop_length = hop_length
        self.sampling_rate = sampling_rate

    def hip_supported(self) -> bool:
        return _hip_supported(self.n_fft, self.win_length, self.hop_length, self.n_mels)

    def forward(self, audio: torch.Tensor, lens=None) -> torch.Tensor:
        """audio [..., L] -> [..., n_mels, 1 + L // hop_length] fp32; lens: sample counts [b] of a ragged batch [b, L] (module docstring)"""
        audio = audio.float()
        L = audio.shape[-1]
        if L <= self.n_fft // 2:
            raise ValueError(f"AudioToMel needs more than n_fft // 2 = {self.n_fft // 2} samples for the reflect padding, got {L}")
        grad = audio.requires_grad and torch.is_grad_enabled()
        if lens is not None:
            lens = torch.as_tensor(lens)
            if audio.ndim != 2 or lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != (audio.shape[0],):
                raise ValueError(f"AudioToMel(lens=) takes audio [b, L] and one integer sample count per utterance [b], got "
                                 f"{list(audio.shape)} and {lens.dtype} {list(lens.shape)}")
            if not (audio.is_cuda and not grad and self.hip_supported()):
                return self._forward_composite_lens(audio, lens)
            return self._forward_hip(audio, lens.to(audio.device))
        if audio.is_cuda and not grad and self.hip_supported():
            return self._forward_hip(audio)
        return self._forward_composite(audio)

    def _forward_composite_lens(self, audio, lens):
        """per utterance: slice, the composite, zero-fill (reads the lengths on the host)"""
        L = audio.shape[-1]
        out = audio.new_zeros(audio.shape[0], self.n_mels, 1 + L // self.hop_length)
        for i, s in enumerate(lens.tolist()):
            s = min(max(int(s), self.n_fft // 2 + 1), L)                # as the kernel clamps
            mel = self._forward_composite(audio[i:i + 1, :s])
            out[i, :, :mel.shape[-1]] = mel[0]
        return out

    def _forward_composite(self, audio):
        shape = audio.shape
        x = audio.reshape(-1, shape[-1])
        window = torch.hann_window(self.win_length, device=x.device)
        spec = torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=window, center=True,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        power = spec.abs().pow(2.0)                                                   # [b, n_freqs, T]
        fb = mel_filterbank(self.n_fft // 2 + 1, 0., self.f_max, self.n_mels, self.sampling_rate).to(x.device)
        mel = torch.matmul(power.transpose(-1, -2), fb).transpose(-1, -2)            # [b, n_mels, T]
        if self.log:
            mel = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
        return mel.reshape(shape[:-1] + mel.shape[-2:])

    def _forward_hip(self, audio, lens=None):
        shape = audio.shape
        x = audio.reshape(-1, shape[-1]).contiguous()
        T = 1 + shape[-1] // self.hop_length
        if x.shape[0] == 0:
            return audio.new_empty(shape[:-1] + (self.n_mels, T))
        p = _plan(x.device, self.n_fft, self.win_length, self.n_mels, self.sampling_rate, self.f_max)
        mel = ops.audio_to_mel(x, self.n_fft, self.hop_length, self.n_mels, self.log, p, **({} if lens is None else dict(lens=lens)))
        return mel.reshape(shape[:-1] + (self.n_mels, T))
