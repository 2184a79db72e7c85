"""PitchExtractor's HIP kernel (csrc/pitch.hip) on an MI355X against the fp64 restatement (tests/pitch_ref64.py) and the PyTorch
composite, and NaturalSpeech2.forward(raw audio, text=...) computing its own pitch on the GPU, eagerly and in a captured graph.

Shapes: the smallest at which the kernel can go wrong -- utterances of 1, 159, 160, 200 samples (one or two frames, all padding),
S - 1, S, S + 1 samples around one span, 5 hops exactly (the last frame starts at L), a few hundred frames so that a block's
frames (3 at the defaults) do not divide the count, lags up to the envelope's 1024 and down to 2, tau_max a multiple of the
64-lag chunk and not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from tests import pitch_ref64 as R                                                         # noqa: E402
from tests.test_audio_to_mel_cpu import _load, build_wrapper                               # noqa: E402
from tests.test_pitch_cpu import EDGE, FS, TONES, check_forward_computes_its_own_pitch    # noqa: E402

DEV = "cuda"


def extractor(**kw):
    from naturalspeech2_pytorch_amd import PitchExtractor
    return PitchExtractor(**kw)


@pytest.fixture
def no_composite(monkeypatch):
    """fail a test that would quietly take the composite on the GPU"""
    from naturalspeech2_pytorch_amd import pitch

    def refuse(*a, **k):
        raise AssertionError("the composite ran")
    monkeypatch.setattr(pitch, "yin_composite", refuse)


@pytest.fixture(scope="module")
def batch3():
    """three different signals of equal length and their restatements"""
    n = 12000
    x = torch.stack((R.tone(180., FS, n, 0.05, seed=21), R.chirp(FS, n, 0.02, seed=22),
                     torch.cat((R.tone(260., FS, n // 2, 0.05, seed=23), (0.1 * R._randn(n - n // 2, 24)).float()))))
    return x, [R.yin_ref64(row, FS, 160, 0.1) for row in x]


@pytest.mark.parametrize("fs,hop,thr", R.CONFIGS)
def test_kernel_matches_restatement_on_mixture(fs, hop, thr, no_composite):
    x, ref = R.mixture_case(fs, hop, thr)
    f0 = extractor(sample_rate=fs, hop_length=hop, threshold=thr)(x.to(DEV))
    assert f0.dtype == torch.float32 and f0.device.type == "cuda"
    R.compare(f0, ref, fs, R.GPU_F0_RTOL)


def test_batch_rows_match_restatement_and_the_utterance_alone(batch3, no_composite):
    x, refs = batch3
    pe = extractor()
    got = pe(x.to(DEV))
    again = pe(x.to(DEV))
    assert got.shape == (3, 76) and torch.equal(got, again)                    # two runs: bit-equal
    for i, ref in enumerate(refs):
        R.compare(got[i], ref, FS, R.GPU_F0_RTOL)
        assert torch.equal(pe(x[i].to(DEV)), got[i]), i                        # a row does not depend on the rest of the batch
    assert torch.equal(pe(x[:, None].to(DEV)), got[:, None])                   # leading dimensions are kept


def test_kernel_and_composite_agree_on_clean_tones():
    from naturalspeech2_pytorch_amd import ops
    from naturalspeech2_pytorch_amd.pitch import yin_composite
    x = torch.stack([R.tone(f, FS, 6000) for f in TONES])
    pe = extractor()
    args = (FS, 160, pe.tau_min, pe.tau_max, pe.threshold)
    got = ops.pitch_yin(x.to(DEV), *args).cpu().double()[:, EDGE:-EDGE]
    f0_c, tau_c = yin_composite(x, *args)                                      # on the CPU
    f0_c, tau_c = f0_c.double()[:, EDGE:-EDGE], tau_c[:, EDGE:-EDGE]
    assert bool((tau_c > 0).all()) and bool((got > 0).all())
    delta_c = FS / f0_c - tau_c
    assert torch.equal(torch.round(FS / got - delta_c).long(), tau_c)          # the same integer lag
    assert float(((got - f0_c).abs() / f0_c).max()) <= R.GPU_F0_RTOL + R.COMPOSITE_F0_RTOL


S_DEFAULT = 3 * 339


@pytest.mark.parametrize("L", [1, 159, 160, 200, S_DEFAULT - 1, S_DEFAULT, S_DEFAULT + 1, 5 * 160])
def test_edge_lengths_decide_as_the_restatement(L, no_composite):
    x = R.tone(300., FS, L, 0.02, seed=L)
    ref = R.yin_ref64(x, FS, 160, 0.1)
    got = extractor()(x.to(DEV)).cpu().double().numpy()
    print(f"L {L}: frames {got.size}, voiced {int((ref['tau'] > 0).sum())}, least margin {ref['margin'].min():.2e}")
    assert got.shape == (1 + L // 160,) and np.isfinite(got).all()
    assert ((got > 0) == (ref["tau"] > 0)).all()
    v = ref["tau"] > 0
    assert (np.abs(got[v] - ref["f0"][v]) <= R.GPU_F0_RTOL * ref["f0"][v]).all()


def test_zeros_give_zeros_and_no_nan(no_composite):
    x = torch.zeros(3, 4000)
    x[1, 1500:] = R.tone(200., FS, 2500)                                       # c(tau) = 0 on the silent frames of a voiced utterance too
    got = extractor()(x.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[0], torch.zeros(26)) and torch.equal(got[2], torch.zeros(26))
    assert torch.equal(got[1, :5], torch.zeros(5)) and bool((got[1, 14:20] > 0).all())


@pytest.mark.parametrize("kw,f,n,lags", [
    (dict(sample_rate=24000, hop_length=400, f0_floor=23.4375, f0_ceil=640.), 180., 9000, (37, 1024)),  # tau_max = 1024: the envelope's edge, 17 chunks
    (dict(sample_rate=24000, hop_length=400, f0_floor=23.4375, f0_ceil=32.), 180., 9000, (750, 1024)),  # ... and a search that starts in chunk 11: lag 800, six periods
    (dict(sample_rate=8000, hop_length=80, f0_floor=125., f0_ceil=4000.), 500., 2000, (2, 64)),          # tau_min = 2; tau_max a multiple of 64
    (dict(sample_rate=16000, hop_length=100, f0_floor=62.5, f0_ceil=400.), 150., 4000, (40, 256)),       # tau_max = 256: lags 0 .. 256 need a fifth chunk
    (dict(sample_rate=24000, hop_length=7, f0_floor=71., f0_ceil=640.), 220., 2400, (37, 339)),          # neither; a hop that is no multiple of 4
])
def test_envelope_edges(kw, f, n, lags, no_composite):
    """(tones below about 100 Hz have minima of d' flatter than the margin rule admits: the restatement alone sets 9 % to 74 % of
    their frames aside, so the deep lags are reached with a 180 Hz tone and a high tau_min instead)"""
    pe = extractor(**kw)
    assert (pe.tau_min, pe.tau_max) == lags and pe.hip_supported()
    fs = kw["sample_rate"]
    x = R.tone(f, fs, n, 0.02, seed=n)
    ref = R.yin_ref64(x, fs, kw["hop_length"], 0.1, kw["f0_floor"], kw["f0_ceil"])
    assert (ref["tau"] > 0).mean() > 0.3
    R.compare(pe(x.to(DEV)), ref, fs, R.GPU_F0_RTOL)


def test_unsupported_configuration_on_the_gpu_takes_the_composite(monkeypatch):
    """tau_max = 2400 is outside the kernel's envelope: a CUDA tensor goes through the composite on the GPU, not into an argument
    error of the C ABI"""
    from naturalspeech2_pytorch_amd import ops

    def refuse(*a, **k):
        raise AssertionError("the kernel ran")
    monkeypatch.setattr(ops, "pitch_yin", refuse)
    pe = extractor(f0_floor=10.)
    assert pe.tau_max == 2400 and not pe.hip_supported()
    got = pe(R.tone(50., FS, FS // 2).to(DEV))
    assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == (76,)
    mid = got[35:41].cpu()                                                      # the ground-truth bound of the CPU test of the same name
    assert float(((mid - 50.).abs() / 50.).max()) <= 1e-3


def test_strided_views_give_the_contiguous_result(batch3, no_composite):
    x, _ = batch3
    pe = extractor()
    want = pe(x.to(DEV))
    wide = torch.zeros(3, 2 * x.shape[1], device=DEV)
    wide[:, ::2] = x.to(DEV)
    view = wide[:, ::2]
    assert not view.is_contiguous() and torch.equal(pe(view), want)
    t = x.to(DEV).t().contiguous().t()                                          # [3, n] with the samples strided by 3
    assert not t.is_contiguous() and torch.equal(pe(t), want)


def test_forward_makes_no_host_synchronisation(batch3, no_composite):
    x = batch3[0].to(DEV)
    pe = extractor()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pe(x)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def fx():
    return _load("aligner_forward_d64.pt")


@pytest.fixture(scope="module")
def with_extractor(fx):
    return build_wrapper(fx, DEV, build_pitch_extractor=True)


def test_wrapper_forward_on_the_gpu_uses_the_kernel(fx, with_extractor, no_composite, monkeypatch):
    from naturalspeech2_pytorch_amd import ops
    calls, kernel = [], ops.pitch_yin

    def counted(*a, **k):
        calls.append(a[0].shape)
        return kernel(*a, **k)
    monkeypatch.setattr(ops, "pitch_yin", counted)
    check_forward_computes_its_own_pitch(with_extractor, fx, DEV)
    assert len(calls) == 2 and calls[0] == calls[1]                             # forward's own call, then the test's explicit one


def test_graphed_step_of_that_forward_returns_the_eager_loss(fx, with_extractor, no_composite):
    from naturalspeech2_pytorch_amd import training
    d = with_extractor
    _, audio, common = check_forward_computes_its_own_pitch(d, fx, DEV)
    ins = (audio, common["text"], common["prompt"], common["times"], common["noise"])

    def loss_fn(a, text, prompt, times, noise):
        return d(a, text=text, prompt=prompt, times=times, noise=noise)
    try:
        l_e = loss_fn(*ins)
        l_e.backward()
        l_e = l_e.detach().clone()
        d.zero_grad(set_to_none=True)
        step = training.GraphedTrainStep(loss_fn, ins, d)
        l_g = step(*ins).detach().clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(l_g)) and torch.equal(l_g, l_e)
        assert any(p.grad is not None for p in d.parameters())
    finally:
        d.zero_grad(set_to_none=True)
