"""PitchExtractor without a GPU: the PyTorch composite against the fp64 restatement (tests/pitch_ref64.py) and against signals
whose F0 is known, the shape contract, the C ABI's argument checks, and NaturalSpeech2.forward(raw audio, text=...) computing
its own pitch.  No parity with pyworld / Kaldi is claimed, so none is tested."""
import ctypes

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib
from tests import pitch_ref64 as R
from tests.test_audio_to_mel_cpu import _load, build_wrapper, raw_inputs

FS = 24000
TONES = (80., 110., 155.5, 220., 330., 440., 600.)
EDGE = 8                                             # interior frames skip the first and last 8


def extractor(**kw):
    from naturalspeech2_pytorch_amd import PitchExtractor
    return PitchExtractor(**kw)


@pytest.mark.parametrize("fs,hop,thr", R.CONFIGS)
def test_composite_matches_restatement_on_mixture(fs, hop, thr):
    from naturalspeech2_pytorch_amd.pitch import yin_composite
    x, ref = R.mixture_case(fs, hop, thr)
    f0, tau = yin_composite(x[None], fs, hop, *R.lags(fs), thr)
    R.compare(f0[0], ref, fs, R.COMPOSITE_F0_RTOL, tau[0])
    assert torch.equal(extractor(sample_rate=fs, hop_length=hop, threshold=thr)(x), f0[0])
    assert 0.3 < (ref["tau"] > 0).mean() < 0.9       # the mixture has both kinds of frame


@pytest.mark.parametrize("f", TONES)
def test_tones_are_tracked(f):
    pe = extractor()
    for noise, bound in ((0., 1e-3), (0.05, 5e-3)):
        f0 = pe(R.tone(f, FS, FS, noise, seed=int(f)))[EDGE:-EDGE].double()
        assert bool((f0 > 0).all()), (f, noise)
        err = float(((f0 - f).abs() / f).max())
        print(f"tone {f} Hz, noise {noise}: worst relative error {err:.2e} (bound {bound:.0e})")
        assert err <= bound, (f, noise, err)


def test_chirp_is_tracked():
    n, hop = FS, 160
    f0 = extractor()(R.chirp(FS, n))[EDGE:-EDGE].double()
    centre = torch.arange(EDGE, 1 + n // hop - EDGE) * hop                # a frame's span is centred on i * hop (+- half a sample)
    inst = R.chirp_f0(FS, n)[centre]
    voiced = f0 > 0
    err = float(((f0 - inst).abs() / inst)[voiced].max())
    print(f"chirp: voiced {float(voiced.double().mean()):.3f}, worst relative error {err:.2e}")
    assert float(voiced.double().mean()) >= 0.95
    assert err <= 2e-2


def test_silence_and_noise_are_unvoiced():
    pe = extractor()
    out = pe(torch.zeros(2, FS // 2))
    assert out.dtype == torch.float32 and torch.equal(out, torch.zeros_like(out))
    noise = pe((0.1 * R._randn(FS, 7)).float())
    assert float((noise > 0).double().mean()) <= 0.05


@pytest.mark.parametrize("L", [1, 159, 160, 200, 1017, 1018])
def test_shapes(L):
    pe = extractor()
    assert pe(torch.randn(L)).shape == (1 + L // 160,)
    out = pe(torch.randn(2, 3, L))
    assert out.shape == (2, 3, 1 + L // 160) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())


def test_module_has_no_state_and_no_gradient():
    pe = extractor()
    assert not list(pe.parameters()) and not list(pe.buffers()) and pe.state_dict() == {}
    assert (pe.tau_min, pe.tau_max, 3 * pe.tau_max) == (37, 339, 1017)
    x = R.tone(200., FS, 4000).requires_grad_()
    out = pe(x)
    assert not out.requires_grad and out.grad_fn is None and bool((out[EDGE:-EDGE] > 0).all())


def test_unsupported_configuration_takes_the_composite(monkeypatch):
    from naturalspeech2_pytorch_amd import ops

    def refuse(*a, **k):
        raise AssertionError("the kernel ran")
    monkeypatch.setattr(ops, "pitch_yin", refuse)
    pe = extractor(f0_floor=10.)
    assert pe.tau_max == 2400 and not pe.hip_supported() and extractor().hip_supported()
    f0 = pe(R.tone(50., FS, FS // 2))
    mid = f0[f0.numel() // 2 - 3:f0.numel() // 2 + 3]
    assert float(((mid - 50.).abs() / 50.).max()) <= 1e-3


def test_abi_symbol_and_argument_checks():
    """no GPU here: an entry point that reached a device call would fail with NS2_ERR_HIP, not NS2_ERR_ARG"""
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.ABI["ns2hip_audio.h"].signatures["ns2_pitch_yin"] == (I, [P, I, L, I, I, I, I, F, P, P])
    assert "ns2_pitch_yin" in _lib.header_symbols("ns2hip_audio.h")
    lib = _lib.load()                                 # raises unless the library exports it
    assert lib.ns2_pitch_yin.argtypes == _lib.SIGNATURES["ns2_pitch_yin"][1] == [P, I, L, I, I, I, I, F, P, P]
    err = lambda: lib.ns2_last_error().decode()       # noqa: E731
    ok = dict(audio=16, B=1, L=4000, fs=24000, hop=160, tau_min=37, tau_max=339, thr=0.1, f0=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ns2_pitch_yin(a["audio"], a["B"], a["L"], a["fs"], a["hop"], a["tau_min"], a["tau_max"], a["thr"], a["f0"], None)
    for kw, msg in ((dict(audio=None), "null pointer"), (dict(f0=None), "null pointer"), (dict(B=0), "B must be"),
                    (dict(B=65536), "B must be"), (dict(L=0), "L must be"), (dict(hop=0), "hop_length"), (dict(fs=0), "sample_rate"),
                    (dict(tau_min=1), "tau_min < tau_max"), (dict(tau_min=339), "tau_min < tau_max"),
                    (dict(tau_max=1025), "tau_max <= 1024"), (dict(thr=float("nan")), "NaN"),
                    (dict(L=1 << 40, hop=1), "too many frames")):
        assert call(**kw) == _lib.NS2_ERR_ARG and msg in err(), (kw, err())


# ---------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def fx():
    return _load("aligner_forward_d64.pt")


@pytest.fixture(scope="module")
def plain(fx):
    return build_wrapper(fx)


@pytest.fixture(scope="module")
def with_extractor(fx):
    return build_wrapper(fx, build_pitch_extractor=True)


def voiced_audio(inp):
    """raw audio of the fixture's shape with a pitch to find: a tone per utterance"""
    b, n = inp["audio"].shape
    return torch.stack([R.tone(150. + 90. * i, FS, n, 0.05, seed=10 + i) for i in range(b)]).to(inp["audio"].device)


def test_default_wrapper_has_no_extractor_and_still_raises(fx, plain):
    inp = raw_inputs(fx)
    assert not hasattr(plain, "pitch_extractor")
    with pytest.raises(NotImplementedError, match="pitch extraction"):
        plain(inp["audio"], text=inp["text"], prompt=inp["prompt"])


def check_forward_computes_its_own_pitch(d, fx, dev):
    """forward(raw audio, text=...) equals, bit for bit, the call that is handed the extractor's pitch"""
    inp = raw_inputs(fx, dev)
    audio = voiced_audio(inp)
    pe = d.pitch_extractor
    assert (pe.sample_rate, pe.hop_length, pe.tau_min, pe.tau_max) == (24000, 160, 37, 339)
    common = dict(text=inp["text"], prompt=inp["prompt"], times=inp["times"], noise=inp["noise"])
    with torch.set_grad_enabled(dev == "cpu"):       # the encoders' CPU path is their autograd composite
        got = d(audio, **common)
        pitch = pe(audio)[:, None]
        want = d(audio, pitch=pitch, **common)
    assert pitch.shape == (2, 1, 1 + audio.shape[-1] // 160) and float((pitch > 0).float().mean()) > 0.7
    assert bool(torch.isfinite(got)) and torch.equal(got, want)
    return got, audio, common


def test_forward_computes_its_own_pitch(fx, plain, with_extractor):
    check_forward_computes_its_own_pitch(with_extractor, fx, "cpu")
    assert list(with_extractor.state_dict()) == list(plain.state_dict())
    assert with_extractor.calc_pitch_with_pyworld is True                  # accepted and stored; selects nothing


def test_extractor_with_latents_names_raw_audio(fx, with_extractor):
    from tests.golden.gen import make_input
    inp = raw_inputs(fx)
    latents = make_input("audio", fx["audio_shape"], seed=fx["input_seed"])
    with pytest.raises(NotImplementedError, match=r"PitchExtractor.*raw audio \[b, samples\]"):
        with_extractor(latents, text=inp["text"], prompt=inp["prompt"], mel=torch.zeros(2, 80, 96))
    with pytest.raises(NotImplementedError, match=r"AudioToMel.*raw audio \[b, samples\]"):
        with_extractor(latents, text=inp["text"], prompt=inp["prompt"])


def test_training_step_from_raw_audio_text_and_prompt(fx, with_extractor):
    """build_aligner + build_duration_pitch + build_pitch_extractor: a loss with its auxiliary terms and gradients, nothing precomputed"""
    d = with_extractor
    inp = raw_inputs(fx)
    loss, aux = d(voiced_audio(inp), text=inp["text"], prompt=inp["prompt"], times=inp["times"], noise=inp["noise"], return_aux_losses=True)
    (loss + aux["aux"]).backward()
    try:
        assert bool(torch.isfinite(loss.detach())) and float(aux["pitch"].detach()) > 0
        grads = [p.grad for p in d.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    finally:
        d.zero_grad(set_to_none=True)
