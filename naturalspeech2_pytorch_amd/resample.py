"""Resample: raw audio at any sample rate -> the codec's rate, on the device.

Upstream resamples on the CPU inside its dataset (audiolm_pytorch's SoundDataset, torchaudio.functional.resample), and its
`EncodecWrapper.forward(x, input_sample_hz=)` does the same per call.  torchaudio is not a dependency here.  This module restates that
function's arithmetic at its DEFAULTS -- resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99 -- and nothing else
of it (no Kaiser window); no parity with torchaudio itself was tested, only with the formula below.

With g = gcd(orig_hz, new_hz), down = orig_hz / g, up = new_hz / g, lpw = lowpass_filter_width:

    base  = min(down, up) * rolloff
    w     = ceil(lpw * down / base)                      the "width"
    T     = 2 w + down                                   taps per phase
    for p in [0, up), i in [0, T):
        t       = clamp((-p / up + (i - w) / down) * base, -lpw, lpw)
        k[p][i] = (1 if t == 0 else sin(pi t) / (pi t)) * cos(pi t / (2 lpw))**2 * base / down
    out[b, f up + p] = sum_{i = 0 .. T-1} k[p][i] x[b, f down + i - w]          x = 0 outside [0, L)
    L_out = ceil(up L / down); only q = f up + p < L_out is stored

The table is built on the host in fp64 and rounded once to fp32 (`resample_table`).  On a GPU, `forward` runs one HIP kernel
(csrc/resample.hip: ns2_resample, include/ns2hip_audio.h) when up, down <= 640 and T <= 1024 -- every pair among 8, 16, 22.05, 24, 32,
44.1 and 48 kHz.  There each output is one fp32 fma chain in ascending i: bit-reproducible, and a row does not depend on the rest of the
batch.  Any other pair, the CPU, and audio that requires grad take `resample_composite` (pad, conv1d with stride `down`, transpose,
crop), which is differentiable.  The module has no parameters and no buffers: its tables are cached per (device, rates, parameters)
and copied from pinned memory, so `forward` makes no device -> host synchronisation after the first call on a device and can be
captured into a graph.

`forward(audio, lens=)` is the ragged batch: sample counts per utterance, integer [b], clamped into [0, L].  Utterance i reads zeros at
and behind lens[i] (a select: NaN there reaches nothing), so its outputs before `out_lens(lens)[i]` = ceil(up lens[i] / down) are those
of the module on `audio[i, :lens[i]]` alone, and exact 0 from there on.  On a GPU that is ns2_resample_lens: the lengths stay on the
device.  The composite does the same per utterance (slice, compute, zero-fill) and reads the lengths.
"""
import math

import torch
from torch import nn
import torch.nn.functional as F

from . import _lib, ops


def resample_ratio(orig_hz: int, new_hz: int):
    """(up, down): the rates divided by their gcd"""
    orig_hz, new_hz = int(orig_hz), int(new_hz)
    assert orig_hz >= 1 and new_hz >= 1, "sample rates are positive integers"
    g = math.gcd(orig_hz, new_hz)
    return new_hz // g, orig_hz // g


def resample_table(orig_hz: int, new_hz: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(up, down, w, k): the module docstring's table k [up, T] in fp64, T = 2 w + down"""
    up, down = resample_ratio(orig_hz, new_hz)
    lpw = int(lowpass_filter_width)
    assert lpw >= 1 and 0. < rolloff <= 1., "lowpass_filter_width >= 1 and rolloff in (0, 1]"
    base = min(down, up) * float(rolloff)
    w = int(math.ceil(lpw * down / base))
    i = torch.arange(-w, w + down, dtype=torch.float64)[None] / down
    p = torch.arange(0, -up, -1, dtype=torch.float64)[:, None] / up
    t = ((p + i) * base).clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    pt = t * math.pi
    sinc = torch.where(pt == 0, torch.ones_like(pt), torch.sin(pt) / torch.where(pt == 0, torch.ones_like(pt), pt))
    return up, down, w, sinc * window * (base / down)


_PLANS = {}


def _plan(device, orig_hz, new_hz, lpw, rolloff):
    """tables of one (device, rates, parameters), built once: `kernel` [up, 1, T] for the composite, and on a GPU `taps`, the transposed
    table [T, up] of ns2_resample, both copied from pinned memory without a sync"""
    key = (device, orig_hz, new_hz, lpw, rolloff)
    plan = _PLANS.get(key)
    if plan is None:
        up, down, w, k = resample_table(orig_hz, new_hz, lpw, rolloff)
        k = k.float()                                               # the one rounding
        host = dict(kernel=k[:, None].contiguous())
        if device.type == "cuda":
            host["taps"] = k.t().contiguous()
            plan = {name: t.pin_memory().to(device, non_blocking=True) for name, t in host.items()}
        else:
            plan = {name: t.to(device) for name, t in host.items()}
        plan.update(up=up, down=down, w=w, host=host)               # host: pinned sources kept alive with the plan
        _PLANS[key] = plan
    return plan


def _composite(x, plan):
    """x [N, L] fp32 -> [N, ceil(up L / down)]: the formula as one strided convolution"""
    up, down, w = plan["up"], plan["down"], plan["w"]
    L = x.shape[-1]
    y = F.conv1d(F.pad(x, (w, w + down))[:, None], plan["kernel"], stride=down)      # [N, up, 1 + L // down]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :(L * up + down - 1) // down]


def resample_composite(audio: torch.Tensor, orig_hz: int, new_hz: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                       lens=None) -> torch.Tensor:
    """the module docstring's formula in plain tensor operations (differentiable): audio [..., L] -> [..., ceil(up L / down)] fp32.
    lens [b] with audio [b, L]: per utterance -- slice, compute, zero-fill (reads the lengths on the host)"""
    audio = audio.float()
    shape = audio.shape
    plan = _plan(audio.device, int(orig_hz), int(new_hz), int(lowpass_filter_width), float(rolloff))
    L = shape[-1]
    L_out = (L * plan["up"] + plan["down"] - 1) // plan["down"]
    x = audio.reshape(-1, L)
    if lens is None:
        return _composite(x, plan).reshape(shape[:-1] + (L_out,))
    rows = []
    for i, s in enumerate(torch.as_tensor(lens).tolist()):
        s = min(max(int(s), 0), L)                                  # as the kernel clamps
        y = _composite(x[i:i + 1, :s], plan) if s > 0 else x.new_zeros(1, 0)
        rows.append(F.pad(y, (0, L_out - y.shape[-1])))
    return torch.cat(rows).reshape(shape[:-1] + (L_out,))


class Resample(nn.Module):
    def __init__(self, orig_hz: int, new_hz: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        super().__init__()
        self.orig_hz, self.new_hz = int(orig_hz), int(new_hz)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        self.up, self.down = resample_ratio(self.orig_hz, self.new_hz)
        assert self.lowpass_filter_width >= 1 and 0. < self.rolloff <= 1., "lowpass_filter_width >= 1 and rolloff in (0, 1]"
        self.width = int(math.ceil(self.lowpass_filter_width * self.down / (min(self.down, self.up) * self.rolloff)))

    def hip_supported(self) -> bool:
        """whether the kernel takes the shape (host arithmetic of the library, no device)"""
        return _lib.load().ns2_resample_frames_per_block(self.up, self.down, self.width) > 0

    def out_len(self, L: int) -> int:
        return (int(L) * self.up + self.down - 1) // self.down

    def out_lens(self, lens) -> torch.Tensor:
        """sample counts -> the counts after resampling, ceil(up lens / down), where `lens` lives (no host read)"""
        lens = torch.as_tensor(lens)
        return (lens.long() * self.up + (self.down - 1)) // self.down

    def forward(self, audio: torch.Tensor, lens=None) -> torch.Tensor:
        """audio [..., L] -> [..., ceil(up L / down)] fp32; lens: sample counts [b] of a ragged batch [b, L] (module docstring).
        Equal rates: the input, unchanged."""
        if self.up == self.down:
            return audio
        audio = audio.float()
        shape = audio.shape
        if shape[-1] < 1:
            raise ValueError("Resample needs at least one sample")
        if lens is not None:
            lens = torch.as_tensor(lens)
            if audio.ndim != 2 or lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != (shape[0],):
                raise ValueError(f"Resample(lens=) takes audio [b, L] and one integer sample count per utterance [b], got "
                                 f"{list(shape)} and {lens.dtype} {list(lens.shape)}")
        grad = audio.requires_grad and torch.is_grad_enabled()
        if not audio.is_cuda or grad or not self.hip_supported():
            return resample_composite(audio, self.orig_hz, self.new_hz, self.lowpass_filter_width, self.rolloff, lens=lens)
        L_out = self.out_len(shape[-1])
        x = audio.reshape(-1, shape[-1])
        if x.shape[0] == 0:
            return audio.new_empty(shape[:-1] + (L_out,))
        p = _plan(x.device, self.orig_hz, self.new_hz, self.lowpass_filter_width, self.rolloff)
        out = ops.resample(x.contiguous(), self.up, self.down, self.width, p["taps"],
                           **({} if lens is None else dict(lens=lens.to(x.device))))
        return out.reshape(shape[:-1] + (L_out,))
