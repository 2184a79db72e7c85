"""AudioToMel's HIP kernel (csrc/audio_to_mel.hip) on an MI355X against the stored fp64 fixtures, fp64 torch.stft on the GPU at
full size, and the composite; NaturalSpeech2.forward(raw audio, ...) on the GPU."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from tests.golden.make_golden_audio_to_mel import frame_errors, make_audio      # noqa: E402
from tests.test_audio_to_mel_cpu import build_wrapper, raw_inputs               # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "audio_to_mel_cases.pt"), weights_only=False)


@pytest.fixture
def no_composite(monkeypatch):
    """fail a test that would quietly take the composite on the GPU"""
    from naturalspeech2_pytorch_amd.audio_to_mel import AudioToMel

    def refuse(self, audio):
        raise AssertionError("the composite ran")
    monkeypatch.setattr(AudioToMel, "_forward_composite", refuse)


def fp64_power(audio, m):
    """the composite's arithmetic in fp64 on the GPU, the filterbank being torchaudio's fp32 table widened"""
    from naturalspeech2_pytorch_amd.audio_to_mel import mel_filterbank
    x = audio.double()
    spec = torch.stft(x, m.n_fft, hop_length=m.hop_length, win_length=m.win_length,
                      window=torch.hann_window(m.win_length, dtype=torch.float64, device=x.device), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    power = spec.real.square_() + spec.imag.square_()
    del spec
    fb = mel_filterbank(m.n_fft // 2 + 1, 0., m.f_max, m.n_mels, m.sampling_rate).double().to(x.device)
    return torch.matmul(power.transpose(-1, -2), fb).transpose(-1, -2)


def test_fixture_cases_on_the_hip_path(fx, no_composite):
    from naturalspeech2_pytorch_amd import AudioToMel
    for name, case in fx["cases"].items():
        m = AudioToMel(**case["kwargs"])
        assert m.hip_supported(), name
        got = m(make_audio(case["recipe"]).to(DEV)).cpu()
        log = case["kwargs"].get("log", True)
        assert got.shape == case["mel64"].shape
        err = frame_errors(got, case["mel64"], log)
        assert err <= (fx["db_bound"] if log else fx["power_bound"]), (name, err)


def test_each_utterance_is_bit_equal_alone(no_composite):
    from naturalspeech2_pytorch_amd import AudioToMel
    g = torch.Generator().manual_seed(11)
    audio = torch.randn(7, 24000 + 37, generator=g)
    audio[3, 5000:9000] = 0.
    for kw in (dict(), dict(n_fft=2048, win_length=1200, hop_length=300), dict(n_fft=256, win_length=256, hop_length=64, n_mels=40),
               dict(n_fft=512, win_length=400, hop_length=512, n_mels=64, log=False)):
        m = AudioToMel(**kw)
        batch = m(audio.to(DEV))
        for i in range(audio.shape[0]):
            assert torch.equal(m(audio[i:i + 1].to(DEV))[0], batch[i]), (kw, i)
            assert torch.equal(m(audio[i].to(DEV)), batch[i]), (kw, i)


@pytest.mark.parametrize("shape", [(32, 327680), (1, 14_400_000)])
def test_full_size_against_fp64_stft(shape, no_composite):
    from naturalspeech2_pytorch_amd import AudioToMel
    g = torch.Generator(device=DEV).manual_seed(5)
    audio = torch.randn(shape, generator=g, device=DEV)
    audio[:, : shape[1] // 3] *= 1e-3                      # a quieter stretch
    t = torch.arange(shape[1], device=DEV, dtype=torch.float64) / 24000
    audio[0] += (0.5 * torch.sin(2 * torch.pi * 440. * t)).float()
    for log in (False, True):
        m = AudioToMel(log=log)
        got = m(audio)
        torch.cuda.synchronize()
        ref = fp64_power(audio, m)
        assert got.shape == (shape[0], 100, 1 + shape[1] // 160)
        err = frame_errors(got, ref, log)
        assert err <= (1e-3 if log else 2e-6), (log, err)
        del got, ref


def test_silent_frames_are_minus_100_db_exactly():
    """the composite's -100.0 on the CPU (10 log10 of the 1e-10 floor) bit for bit; torch's GPU log10 rounds differently"""
    from naturalspeech2_pytorch_amd import AudioToMel
    audio = torch.randn(3, 16000)
    audio[0] = 0.
    audio[1, 4000:12000] = 0.
    m = AudioToMel()
    got = m(audio.to(DEV)).cpu()
    comp = m(audio)
    silent = comp == -100.
    assert bool(silent[0].all()) and int(silent[1].sum()) > 100 * 40
    assert torch.equal(got[silent], comp[silent])
    assert bool((got[~silent] > -100.).all())
    gpu_comp = m._forward_composite(audio.to(DEV)).cpu()
    assert float((gpu_comp[silent] + 100.).abs().max()) <= 1e-4


@pytest.mark.parametrize("kw", [dict(n_fft=1000, win_length=640), dict(n_fft=4096, win_length=2048), dict(n_mels=300, n_fft=2048),
                                dict(hop_length=1500), dict(n_fft=128, win_length=128, hop_length=32, n_mels=20)])
def test_other_configurations_take_the_composite(kw, monkeypatch):
    from naturalspeech2_pytorch_amd import AudioToMel, ops

    def refuse(*a, **k):
        raise AssertionError("the kernel ran")
    monkeypatch.setattr(ops, "audio_to_mel", refuse)
    m = AudioToMel(**kw)
    assert not m.hip_supported()
    audio = torch.randn(2, 9000)
    got = m(audio.to(DEV)).cpu()
    want = m(audio)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-2


def test_forward_makes_no_host_synchronisation(no_composite):
    from naturalspeech2_pytorch_amd import AudioToMel
    audio = torch.randn(4, 30000, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        AudioToMel(n_mels=72, hop_length=120)(audio)        # a configuration no other test plans: the tables are built here
        AudioToMel(n_mels=72, hop_length=120)(audio)
        AudioToMel()(audio[:, :20000])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_requires_grad_on_the_gpu_runs_the_composite():
    from naturalspeech2_pytorch_amd import AudioToMel
    x = torch.randn(1, 4000, device=DEV, requires_grad=True)
    AudioToMel()(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_raw_audio_forward_on_the_gpu_equals_the_explicit_mel_call():
    from naturalspeech2_pytorch_amd import AudioToMel
    fx = torch.load(os.path.join(GOLDEN, "aligner_forward_d64.pt"), weights_only=False)
    d = build_wrapper(fx, DEV)
    inp = raw_inputs(fx, DEV)
    common = dict(text=inp["text"], prompt=inp["prompt"], pitch=inp["pitch"], times=inp["times"], noise=inp["noise"])
    with torch.no_grad():
        got = d(inp["audio"], **common)
        mel = AudioToMel(n_mels=80, hop_length=160)(inp["audio"])[..., :inp["pitch"].shape[-1]]
        want = d(inp["audio"], mel=mel, **common)
    assert mel.shape == (2, 80, 96) and torch.isfinite(got) and torch.equal(got, want)
