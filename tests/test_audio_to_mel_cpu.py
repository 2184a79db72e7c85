"""AudioToMel on the CPU composite against the fp64 fixtures of tests/golden/make_golden_audio_to_mel.py (the reference's code
over a re-implemented torchaudio), and NaturalSpeech2.forward(raw audio, text=..., pitch=...) computing its own mel frames."""
import copy
import os

import pytest
import torch

from tests.golden.gen import make_weights, make_input
from tests.golden.make_golden_audio_to_mel import frame_errors, make_audio

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "audio_to_mel_cases.pt"), weights_only=False)


def check_case(got, case, fx):
    kw = case["kwargs"]
    assert got.dtype == torch.float32 and got.shape == case["mel64"].shape
    err = frame_errors(got, case["mel64"], kw.get("log", True))
    assert err <= (fx["db_bound"] if kw.get("log", True) else fx["power_bound"]), err
    return err


def test_composite_matches_the_fp64_fixture(fx):
    from naturalspeech2_pytorch_amd import AudioToMel
    for name, case in fx["cases"].items():
        check_case(AudioToMel(**case["kwargs"])(make_audio(case["recipe"])), case, fx)


def test_silence_is_minus_100_db(fx):
    from naturalspeech2_pytorch_amd import AudioToMel
    case = fx["cases"]["silence"]
    out = AudioToMel(**case["kwargs"])(make_audio(case["recipe"]))
    assert torch.equal(out, torch.full_like(out, -100.))


def test_filterbank_structure_at_the_defaults():
    from naturalspeech2_pytorch_amd.audio_to_mel import mel_filterbank
    fb = mel_filterbank(513, 0., 8000, 100, 24000)
    assert fb.shape == (513, 100) and fb.dtype == torch.float32
    assert int((fb > 0).sum(1).max()) <= 2                   # a bin lies in at most two triangles
    assert bool((fb.amax(0) > 0).all())                      # no empty filter
    nz = (fb > 0).nonzero()
    assert int(nz[:, 0].max()) <= 341                        # bins above 341 (8 kHz) have no weight
    widths = [int(c.nonzero().max() - c.nonzero().min() + 1) for c in fb.t()]
    assert max(widths) <= 23


@pytest.mark.parametrize("L", [513, 640, 1000, 4321, 24000])
def test_output_shape_follows_the_hop(L):
    from naturalspeech2_pytorch_amd import AudioToMel
    out = AudioToMel()(torch.randn(2, 3, L))
    assert out.shape == (2, 3, 100, 1 + L // 160) and out.dtype == torch.float32
    assert AudioToMel(log=False)(torch.randn(L, dtype=torch.float64)).shape == (100, 1 + L // 160)


@pytest.mark.parametrize("L", [1, 100, 512])
def test_short_audio_raises(L):
    from naturalspeech2_pytorch_amd import AudioToMel
    with pytest.raises(ValueError, match="n_fft // 2"):
        AudioToMel()(torch.randn(1, L))


def test_module_has_no_state():
    from naturalspeech2_pytorch_amd import AudioToMel
    m = AudioToMel()
    assert not list(m.parameters()) and not list(m.buffers()) and m.state_dict() == {}


def test_requires_grad_runs_the_composite_under_autograd():
    from naturalspeech2_pytorch_amd import AudioToMel
    x = torch.randn(1, 2000, requires_grad=True)
    AudioToMel()(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


# ---------------------------------------------------------------- the wrapper
def _load(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


def tiny_codec(dim):
    """an EncodecWrapperHIP whose `encoder` is a stub callable and whose RVQ returns the latents: only the raw-audio plumbing
    of forward() is under test"""
    from naturalspeech2_pytorch_amd import EncodecWrapperHIP
    hop = EncodecWrapperHIP.seq_len_multiple_of

    def encoder(x):                                           # [b, 1, t] -> [b, dim, t / 320]
        b, _, t = x.shape
        return x.reshape(b, t // hop, hop)[..., :dim].transpose(1, 2) * 10.

    codec = EncodecWrapperHIP(torch.zeros(1, 64, 128), encoder=encoder)
    codec.codebook_dim = dim
    codec.rvq.encode = lambda lat: (torch.zeros(lat.shape[:2] + (1,), dtype=torch.long, device=lat.device), lat)
    return codec


def build_wrapper(fx, dev="cpu", **extra):
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    kw = dict(fx["wrapper_kwargs"])
    kw.pop("target_sample_hz", None)
    d = NaturalSpeech2(Model(**fx["model_kwargs"]), codec=tiny_codec(fx["model_kwargs"]["dim"]), build_aligner=True,
                       build_duration_pitch=True, **kw, **extra).eval()
    res = d.load_state_dict(make_weights(fx["shapes"], seed=fx["weight_seed"]), strict=False)
    assert res.missing_keys == ["codec.rvq.codebooks"] and not res.unexpected_keys
    if dev == "cpu":
        for enc in (d.prompt_enc, d.phoneme_enc):   # the encoders' CPU path is their autograd composite
            enc.force_autograd = True
    return d.to(dev)


def raw_inputs(fx, dev="cpu"):
    s = fx["input_seed"]
    b, n, _ = fx["audio_shape"]
    pitch = 80 + 320 * make_input("pitch", fx["pitch_shape"], seed=s, uniform=True)
    audio = 0.1 * make_input("raw_audio", (b, n * 320), seed=s)
    return dict(audio=audio.to(dev), text=fx["text"].to(dev), prompt=make_input("prompt", fx["prompt_shape"], seed=s).to(dev),
                pitch=pitch.to(dev), times=make_input("times", fx["times_shape"], seed=s, uniform=True).to(dev),
                noise=make_input("noise", fx["noise_shape"], seed=s).to(dev))


def run_raw_equals_explicit_mel(dev):
    from naturalspeech2_pytorch_amd import AudioToMel
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx, dev)
    inp = raw_inputs(fx, dev)
    common = dict(text=inp["text"], prompt=inp["prompt"], pitch=inp["pitch"], times=inp["times"], noise=inp["noise"])
    got = d(inp["audio"], **common)
    mel = AudioToMel(n_mels=80, hop_length=160)(inp["audio"])[..., :inp["pitch"].shape[-1]]
    assert mel.shape == (2, 80, 96)
    want = d(inp["audio"], mel=mel, **common)
    assert torch.isfinite(got) and torch.equal(got, want)
    return mel


def test_raw_audio_forward_equals_the_explicit_mel_call():
    run_raw_equals_explicit_mel("cpu")


def test_wrapper_builds_audio_to_mel_without_state():
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    fx = _load("aligner_forward_d64.pt")
    kwargs = dict(f_max=7000)
    before = copy.deepcopy(kwargs)
    d = NaturalSpeech2(Model(**fx["model_kwargs"]), codec=None, target_sample_hz=16000, build_aligner=True, build_duration_pitch=True,
                       aligner_dim_in=80, mel_hop_length=200, audio_to_mel_kwargs=kwargs)
    assert kwargs == before                                    # the caller's dict is not updated
    m = d.audio_to_mel
    assert (m.n_mels, m.hop_length, m.sampling_rate, m.f_max, m.n_fft, m.win_length) == (80, 200, 16000, 7000, 1024, 640)
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == fx["shapes"]     # state_dict keys unchanged
    plain = NaturalSpeech2(Model(dim=64, depth=1, dim_prompt=512, condition_on_prompt=True), codec=None, target_sample_hz=24000)
    assert hasattr(plain, "audio_to_mel") and not any(k.startswith("audio_to_mel") for k in plain.state_dict())


def test_latents_without_mel_still_name_audio_to_mel():
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx)
    inp = raw_inputs(fx)
    latents = make_input("audio", fx["audio_shape"], seed=fx["input_seed"])
    with pytest.raises(NotImplementedError, match=r"AudioToMel.*raw audio \[b, samples\]"):
        d(latents, text=inp["text"], prompt=inp["prompt"], pitch=inp["pitch"])
    with pytest.raises(NotImplementedError, match="pitch extraction"):
        d(inp["audio"], text=inp["text"], prompt=inp["prompt"])
    with pytest.raises(NotImplementedError, match="pitch extraction"):
        d(inp["audio"], text=inp["text"], prompt=inp["prompt"], mel=torch.zeros(2, 80, 96))


def test_no_aligner_still_raises_on_raw_audio():
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    d = NaturalSpeech2(Model(dim=64, depth=1, dim_prompt=512, condition_on_prompt=True), codec=tiny_codec(64))
    with pytest.raises(NotImplementedError, match="Aligner"):
        d(torch.randn(1, 3200), text=torch.zeros(1, 5, dtype=torch.long), pitch=torch.rand(1, 1, 10) * 300,
          prompt_enc=torch.randn(1, 16, 512))
