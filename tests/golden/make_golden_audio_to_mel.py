"""Golden fixtures of AudioToMel (the reference's AudioToMel, NS2:181-224), build container only:

    python tests/golden/make_golden_audio_to_mel.py

Writes tests/golden/audio_to_mel_cases.pt.

The oracle is the reference's own code over a RE-IMPLEMENTED torchaudio.  torchaudio is not installed here, so before
oracle/ref_stub.py loads the reference this script puts a small shim into sys.modules["torchaudio"]: `transforms.Spectrogram`,
`MelScale` and `AmplitudeToDB` written from torchaudio's documented definitions (torch.stft with a periodic Hann window,
power 2; melscale_fbanks with f_min 0, norm None, the HTK scale; 10 log10(clamp(x, 1e-10)) with ref 1 and no top_db), plus
the names the reference imports without using (`transforms.Resample`, `functional`).  The reference's unmodified
`AudioToMel.forward` then runs on the CPU in fp32, and the same arithmetic runs in fp64.  The fixture keeps the fp64 mel
power (before the dB) of every case, the fp32 reference output's measured error against it, and each input as a recipe
(`make_audio`), not as samples.
"""
import importlib.machinery
import math
import os
import sys
import types

import torch
from torch import nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "audio_to_mel_cases.pt")

DEFAULT = dict(n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, win_length=640, hop_length=160)
WIDE = dict(DEFAULT, n_fft=2048, win_length=1200, hop_length=300)

# name -> (recipe, AudioToMel kwargs); a recipe is a list of (kind, n_samples, seed, params) segments per utterance
CASES = {
    "noise": ([[("noise", 8000, 1, 1.0)], [("noise", 8000, 2, 0.3)]], dict(DEFAULT)),
    "tone_440_int16": ([[("tone", 8000, 0, (440., 3e4))]], dict(DEFAULT)),
    "chirp": ([[("chirp", 8000, 0, (100., 8000., 0.5))]], dict(DEFAULT)),
    "silence": ([[("zeros", 4000, 0, None)]], dict(DEFAULT)),
    "silence_tone_quiet_noise": ([[("zeros", 2000, 0, None), ("tone", 3000, 0, (1000., 0.5)), ("noise", 3000, 3, 1e-6)]],
                                 dict(DEFAULT)),
    "dc": ([[("dc", 4000, 0, 0.25)]], dict(DEFAULT)),
    "minimal_length": ([[("noise", 513, 4, 1.0)]], dict(DEFAULT)),
    "length_not_multiple_of_hop": ([[("noise", 4321, 5, 1.0)], [("tone", 4321, 0, (3000., 0.1))]], dict(DEFAULT)),
    "power_no_log": ([[("noise", 4000, 6, 1.0)], [("tone", 4000, 0, (440., 0.5))]], dict(DEFAULT, log=False)),
    "nfft2048_win1200_hop300": ([[("noise", 9000, 7, 1.0)], [("tone", 9000, 0, (250., 0.8))]], dict(WIDE)),
}


def _segment(kind, n, seed, params, sr=24000):
    t = torch.arange(n, dtype=torch.float64) / sr
    if kind == "noise":
        return params * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if kind == "tone":
        f, a = params
        return a * torch.sin(2 * math.pi * f * t)
    if kind == "chirp":                    # linear sweep f0 -> f1 over the segment
        f0, f1, a = params
        dur = n / sr
        return a * torch.sin(2 * math.pi * (f0 * t + (f1 - f0) / (2 * dur) * t * t))
    if kind == "dc":
        return torch.full((n,), float(params), dtype=torch.float64)
    return torch.zeros(n, dtype=torch.float64)


def make_audio(recipe) -> torch.Tensor:
    """fp32 [b, L] from a recipe of CASES"""
    return torch.stack([torch.cat([_segment(*seg) for seg in utt]) for utt in recipe]).float()


def mel_power_fp64(audio, n_mels, sampling_rate, f_max, n_fft, win_length, hop_length, **_):
    """the arithmetic of the reference's AudioToMel before the dB, in fp64.  The filterbank is torchaudio's fp32 table, widened:
    it is a constant of the definition, and rebuilt in fp64 its weights move by ~1e-5 near the triangles' edges (cancellation
    in f_pts - freq), which would swamp the transform's own error"""
    x = audio.double()
    spec = torch.stft(x, n_fft, hop_length=hop_length, win_length=win_length, window=torch.hann_window(win_length, dtype=torch.float64),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    fb = _melscale_fbanks(n_fft // 2 + 1, 0., f_max, n_mels, sampling_rate).double()
    return torch.matmul(spec.abs().pow(2).transpose(-1, -2), fb).transpose(-1, -2)


def _melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, dtype=torch.float32):
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk"), as documented"""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min, m_max = (2595.0 * math.log10(1.0 + f / 700.0) for f in (f_min, f_max))
    f_pts = 700.0 * (10.0 ** (torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))


def install_torchaudio_shim():
    """sys.modules["torchaudio"] with the three transforms the reference's AudioToMel calls (see the module docstring)"""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__spec__ = importlib.machinery.ModuleSpec(name, loader=None)
        sys.modules[name] = m
        return m

    class Spectrogram(nn.Module):
        def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2.0,
                     normalized=False, center=True, pad_mode="reflect", onesided=True):
            super().__init__()
            assert pad == 0 and power == 2.0 and not normalized
            self.n_fft, self.win_length = n_fft, win_length or n_fft
            self.hop_length = hop_length or self.win_length // 2
            self.window = window_fn(self.win_length)
            self.center, self.pad_mode, self.onesided = center, pad_mode, onesided

        def forward(self, waveform):
            shape = waveform.size()
            x = waveform.reshape(-1, shape[-1])
            spec = torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=self.window,
                              center=self.center, pad_mode=self.pad_mode, normalized=False, onesided=self.onesided,
                              return_complex=True)
            spec = spec.reshape(shape[:-1] + spec.shape[-2:])
            return spec.abs().pow(2.0)

    class MelScale(nn.Module):
        def __init__(self, n_mels=128, sample_rate=16000, f_min=0., f_max=None, n_stft=201, norm=None, mel_scale="htk"):
            super().__init__()
            assert norm is None and mel_scale == "htk"
            self.fb = _melscale_fbanks(n_stft, f_min, f_max if f_max is not None else float(sample_rate // 2), n_mels, sample_rate)

        def forward(self, specgram):
            return torch.matmul(specgram.transpose(-1, -2), self.fb).transpose(-1, -2)

    class AmplitudeToDB(nn.Module):
        def __init__(self, stype="power", top_db=None):
            super().__init__()
            assert stype == "power" and top_db is None
            self.multiplier, self.amin, self.db_multiplier = 10.0, 1e-10, math.log10(max(1e-10, 1.0))

        def forward(self, x):
            x_db = self.multiplier * torch.log10(torch.clamp(x, min=self.amin))
            return x_db - self.multiplier * self.db_multiplier

    class Resample(nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    ta = mod("torchaudio")
    ta.transforms = mod("torchaudio.transforms", Spectrogram=Spectrogram, MelScale=MelScale, AmplitudeToDB=AmplitudeToDB,
                        Resample=Resample)
    ta.functional = mod("torchaudio.functional")


def frame_errors(got, mel64, log):
    """(power: max over frames of max_m |d| / max_m mel64, dB: max |d dB| where mel64 >= 1e-5 x the frame's max)"""
    peak = mel64.amax(dim=-2, keepdim=True)
    if not log:
        return float(((got.double() - mel64).abs().amax(dim=-2, keepdim=True) / peak.clamp(min=1e-300)).max())
    ref_db = 10 * torch.log10(mel64.clamp(min=1e-10))
    live = mel64 >= 1e-5 * peak
    return float((got.double() - ref_db).abs()[live].max())


def main():
    sys.path.insert(0, ROOT)
    assert "torchaudio" not in sys.modules
    install_torchaudio_shim()
    from oracle.ref_stub import load_reference
    ref = load_reference()
    cases = {}
    for name, (recipe, kw) in CASES.items():
        audio = make_audio(recipe)
        m = ref.AudioToMel(**kw)
        with torch.no_grad():
            out32 = m(audio)
        mel64 = mel_power_fp64(audio, **kw)
        err = frame_errors(out32, mel64, kw.get("log", True))
        print(f"{name:28s} {tuple(audio.shape)} -> {tuple(out32.shape)}  reference fp32 vs fp64: {err:.2e}")
        cases[name] = dict(recipe=recipe, kwargs=kw, mel64=mel64, ref_fp32_err=err)
    torch.save(dict(cases=cases, power_bound=2e-6, db_bound=1e-3, db_floor=1e-5), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
