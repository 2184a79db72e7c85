"""Resample's HIP kernel (csrc/resample.hip) on an MI355X against the fp64 restatement (tests/resample_ref64.py) within the derived
bound, its bit-level promises (reproducible, a row alone, any row alignment, `lens=`), what it refuses, a captured call, and
`input_sample_hz=` / `prompt_sample_hz=` end to end with the real HIP codec.

Shapes: the smallest at which the kernel can go wrong -- 1, 2, w, w + 1 samples (all padding), one input period `down` and its
neighbours, a workgroup's F frames (F down samples) and its neighbours, two and a half workgroups at an odd length, and per pair
lengths whose last output frame is full, holds one sample, and lacks one (up L mod down in {0, 1, down - 1})."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import EncodecWrapperHIP, Model, NaturalSpeech2, Resample, SpeechPromptEncoder, _lib, ops  # noqa: E402
from naturalspeech2_pytorch_amd import resample as RS  # noqa: E402
from tests import resample_ref64 as R  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402
from tests.test_ragged_training_gpu import YARDSTICK  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
HOP = EncodecWrapperHIP.seq_len_multiple_of
PAIR_IDS = [f"{o}to{n}" for o, n in R.PAIRS]


@pytest.fixture
def no_composite(monkeypatch):
    """fail a test that would quietly take the composite on the GPU"""
    def refuse(*a, **k):
        raise AssertionError("the composite ran")
    monkeypatch.setattr(RS, "resample_composite", refuse)


def frames_per_block(mod):
    F = _lib.load().ns2_resample_frames_per_block(mod.up, mod.down, mod.width)
    assert F > 0
    return F


def lengths(mod):
    up, down, w, F = mod.up, mod.down, mod.width, frames_per_block(mod)
    tail = {}                                                       # the first lengths past one period with up L mod down = 0, 1, down - 1
    for L in range(down + 2, 3 * down + 3):
        tail.setdefault(up * L % down, L)
    Ls = [1, 2, w, w + 1, down - 1, down, down + 1, F * down - 1, F * down, F * down + 1, int(2.5 * F * down) | 1]
    Ls += [tail[r] for r in sorted({0, 1 % down, down - 1}) if r in tail]
    return sorted({L for L in Ls if L >= 1})


def _lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- 1. the kernel against the restatement
@pytest.mark.parametrize("orig,new", R.PAIRS, ids=PAIR_IDS)
def test_kernel_matches_restatement(orig, new, no_composite):
    mod = Resample(orig, new)
    T = R.taps_per_phase(orig, new)
    worst = 0.
    for L in lengths(mod):
        for B in ((3, 1) if L % 2 else (1,)):                       # B = 3 with odd L: rows 1 and 2 are not 16-byte aligned
            x = R.noise(1000 * B + L, B, L)
            ref, S = R.resample64(x, orig, new)
            got = mod(torch.from_numpy(x).to(DEV))
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == ref.shape, (L, B)
            ratio = float((np.abs(got.cpu().double().numpy() - ref) / R.bound(S, T)).max())
            worst = max(worst, ratio)
            assert ratio <= 1, (L, B, ratio)
    print(f"{orig} -> {new} (up {mod.up}, down {mod.down}, T {T}, F {frames_per_block(mod)}): kernel against the restatement, "
          f"worst error / bound = {worst:.3f}")


# ---- 2. bits
@pytest.mark.parametrize("orig,new", [(44100, 24000), (16000, 24000), (48000, 24000)], ids=["44k1", "16k", "48k"])
def test_bits_two_runs_a_row_alone_and_any_alignment(orig, new, no_composite):
    mod = Resample(orig, new)
    L = int(1.5 * frames_per_block(mod) * mod.down) | 1             # odd: every row of the batch at another alignment
    x = torch.from_numpy(R.noise(31, 4, L)).to(DEV)
    got = mod(x)
    assert torch.equal(mod(x), got)                                 # two runs
    assert torch.equal(mod(x[:, None]), got[:, None])               # leading dimensions are kept
    buf = torch.zeros(L + 8, device=DEV)
    for i in range(4):
        assert torch.equal(mod(x[i:i + 1].clone())[0], got[i]), i   # a row does not depend on the rest of the batch
        for off in (1, 2, 3):                                       # a row view 4, 8, 12 bytes off a 16-byte boundary
            view = buf[off:off + L]
            view.copy_(x[i])
            assert view.data_ptr() % 16 == 4 * off
            assert torch.equal(mod(view), got[i]), (i, off)


# ---- 3. lens
@pytest.mark.parametrize("orig,new", [(44100, 24000), (16000, 24000), (48000, 24000), (22050, 24000)], ids=["44k1", "16k", "48k", "22k05"])
def test_lens_is_the_utterance_alone_bit_for_bit(orig, new, no_composite):
    mod = Resample(orig, new)
    F, down = frames_per_block(mod), mod.down
    L = int(2.5 * F * down) | 1
    lens = [1, down + 1, F * down, L]
    x = torch.from_numpy(R.noise(41, 4, L)).to(DEV)
    got = mod(x, lens=_lens(lens))
    assert got.shape == (4, mod.out_len(L)) and mod.out_lens(_lens(lens)).tolist() == [mod.out_len(s) for s in lens]
    for i, s in enumerate(lens):
        n = mod.out_len(s)
        assert torch.equal(got[i, :n], mod(x[i:i + 1, :s].contiguous())[0]), f"utterance {i} ({s} samples)"
        assert torch.count_nonzero(got[i, n:]) == 0
    assert not torch.equal(got[2], mod(x)[2])                       # the lengths are seen
    for value in (NAN, 7.0):                                        # what lies behind a length reaches nothing
        behind = x.clone()
        for i, s in enumerate(lens):
            behind[i, s:] = value
        assert torch.equal(mod(behind, lens=_lens(lens)), got)
    assert torch.equal(mod(x, lens=lens), got)                      # a list goes to the device
    clamped = mod(x, lens=_lens([0, -5, L + 100, 2 ** 31 - 1]))      # 0 and beyond L are clamped
    assert torch.count_nonzero(clamped[:2]) == 0 and torch.equal(clamped[2:], mod(x)[2:])
    assert torch.equal(mod(x, lens=_lens([L] * 4)), mod(x))         # full lengths: the plain entry


# ---- 4. what the kernel does not take
def test_unsupported_shape_is_unavailable_and_the_module_takes_the_composite():
    mod = Resample(1, 641)
    assert (mod.up, mod.down) == (641, 1) and not mod.hip_supported()
    x = torch.from_numpy(R.noise(51, 2, 40)).to(DEV)
    taps = torch.zeros(2 * mod.width + 1, 641, device=DEV)
    out = torch.full((2, 40 * 641), 3.0, device=DEV)
    lib = _lib.load()
    rc = lib.ns2_resample(x.data_ptr(), 2, 40, 641, 1, mod.width, taps.data_ptr(), out.data_ptr(), 40 * 641, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.NS2_UNAVAILABLE and bool((out == 3.0).all())  # nothing was launched
    with pytest.raises(_lib.Ns2Error, match="ns2_resample"):
        ops.resample(x, 641, 1, mod.width, taps)
    got = mod(x)
    assert got.is_cuda and torch.equal(got, RS.resample_composite(x, 1, 641))
    ref, S = R.resample64(x.cpu().numpy(), 1, 641)
    assert float((np.abs(got.cpu().double().numpy() - ref) / (2 * R.bound(S, 2 * mod.width + 1))).max()) <= 1
    xg = x.clone().requires_grad_()                                 # audio that requires grad: the composite, differentiable
    y = Resample(48000, 24000)(xg)
    y.sum().backward()
    assert y.requires_grad and xg.grad.abs().sum() > 0


# ---- 5. capture
def test_captured_call_replays_on_new_input(no_composite):
    mod = Resample(44100, 24000)
    L = 3 * frames_per_block(mod) * mod.down + 5
    a, b = (torch.from_numpy(R.noise(s, 2, L)).to(DEV) for s in (61, 62))
    lens = _lens([L, L // 2])
    eager_a, eager_b = mod(a, lens=lens), mod(b, lens=lens)        # (the first call on the device builds the tables)
    static = a.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mod(static, lens=lens)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # one kernel, a single branch
        out = mod(static, lens=lens)
    g.replay()
    assert torch.equal(out, eager_a)
    static.copy_(b)
    g.replay()
    assert torch.equal(out, eager_b) and not torch.equal(eager_a, eager_b)


# ---- 6. end to end with the HIP codec
@pytest.fixture(scope="module")
def codec():
    """built as tests/test_ragged_audio_gpu.py builds it: the HIP SEANet of a freshly initialised EnCodec, codebooks of the encoder's scale"""
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    hf = tf.EncodecModel(tf.EncodecConfig()).eval().to(DEV)
    with torch.no_grad():
        c = EncodecWrapperHIP.from_hf(hf, hip_seanet=True).to(DEV).eval()
        scale = c.encoder(make_input("wav", (2, 8 * HOP), seed=14).to(DEV)[:, None] * 0.1).std()
        assert float(scale) > 0
        cb = make_input("ragged_audio:codebooks", (8, 1024, 128), seed=22) * (0.5 ** torch.arange(8, dtype=torch.float32))[:, None, None]
        return EncodecWrapperHIP(cb.to(DEV) * scale, encoder=c.encoder, decoder=c.decoder).to(DEV).eval()


def _diffusion(codec):
    m = Model(dim=128, depth=1, ragged_training=True)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=71))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", "exact"
    return m, NaturalSpeech2(m, codec=codec, timesteps=2, objective="eps", min_snr_loss_weight=False, ragged_audio=True).to(DEV)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


def _loss_and_grads(m, d, *a, **kw):
    for p in m.parameters():
        p.grad = None
    loss = d(*a, **kw)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_codec_and_forward_take_input_sample_hz(codec, no_composite):
    rs = Resample(48000, 24000)
    raw = make_input("resample:raw48", (2, 2 * 9 * HOP + 75), seed=81).to(DEV) * 0.1
    emb, codes, _ = codec(raw, input_sample_hz=48000)
    emb_h, codes_h, _ = codec(rs(raw))
    assert emb.shape == (2, 9, 128) and codec(raw)[0].shape[1] == 18
    assert torch.equal(emb, emb_h) and torch.equal(codes, codes_h) and emb.abs().sum() > 0
    with pytest.raises(ValueError, match="input_sample_hz"):
        codec(emb, input_sample_hz=48000)
    m, d = _diffusion(codec)
    t, noise = make_input("times", (2,), seed=72, uniform=True).to(DEV), make_input("noise", (2, 9, 128), seed=73).to(DEV)
    got = d(raw, input_sample_hz=48000, times=t, noise=noise)
    want = d(rs(raw), times=t, noise=noise)
    assert torch.isfinite(got) and torch.equal(got, want)


def test_ragged_raw_audio_at_another_rate_is_the_mean_of_the_solo_losses(codec, no_composite):
    """the rule of tests/test_ragged_audio_gpu.py: twice the equal-length batch-against-solo yardstick; NaN behind the lengths, same bits.
    48 k -> 24 k, 9 and 7 frames after conversion, a padded input length that is no multiple of the hop"""
    m, d = _diffusion(codec)
    rs = Resample(48000, 24000)
    lens = [2 * (9 * HOP + 10), 2 * (7 * HOP + 50) + 1]
    raw = make_input("resample:ragged48", (2, lens[0] + 7), seed=82).to(DEV) * 0.1
    assert (rs.out_lens(_lens(lens)) // HOP).tolist() == [9, 7] and rs.out_len(raw.shape[1]) % HOP
    t, noise = make_input("times", (2,), seed=72, uniform=True).to(DEV), make_input("noise", (2, 9, 128), seed=73).to(DEV)
    loss, g = _loss_and_grads(m, d, raw, audio_lens=_lens(lens), input_sample_hz=48000, times=t, noise=noise)
    solo, gs = [], None
    for i, (s, f) in enumerate(zip(lens, (9, 7))):
        l, gi = _loss_and_grads(m, d, raw[i:i + 1, :s].contiguous(), input_sample_hz=48000, times=t[i:i + 1], noise=noise[i:i + 1, :f].contiguous())
        solo.append(l)
        gs = gi if gs is None else {k: gs[k] + gi[k] for k in gs}
    worst = ("loss", rel(loss, torch.stack(solo).mean()))
    for k in gs:
        worst = max(worst, (k, rel(g[k], gs[k] / 2)), key=lambda z: z[1])
    bound = 2 * YARDSTICK[("uncond", "exact")]
    print(f"ragged raw audio at 48 kHz, loss and gradients vs the mean of the solos: worst {worst[0]} {worst[1]:.3e} (bound {bound:.3e})")
    assert torch.isfinite(loss) and set(g) == set(gs)
    behind = raw.clone()
    behind[1, lens[1]:] = NAN
    loss_n, g_n = _loss_and_grads(m, d, behind, audio_lens=_lens(lens), input_sample_hz=48000, times=t, noise=noise)
    assert torch.equal(loss_n, loss) and all(torch.equal(g_n[k], g[k]) for k in g)
    assert torch.equal(d(raw, audio_lens=lens, input_sample_hz=48000, times=t, noise=noise).detach(), loss)     # a list: checked on the host
    with pytest.raises(ValueError, match="at least 7 codec frames"):
        d(raw, audio_lens=[lens[0], 2 * 7 * HOP - 2], input_sample_hz=48000, times=t, noise=noise)
    assert worst[1] <= bound, worst


def test_sample_takes_prompt_sample_hz(codec, no_composite):
    m = Model(dim=128, depth=1, dim_prompt=64, condition_on_prompt=True, num_latents_m=16)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=91))
    d = NaturalSpeech2(m.eval(), codec=codec, timesteps=2)
    enc = SpeechPromptEncoder(128, dims=(64, 128, 64), depth=1)
    enc.load_state_dict(make_weights({k: tuple(v.shape) for k, v in enc.state_dict().items()}, seed=92))
    d.prompt_enc = enc
    d = d.to(DEV).eval()
    rs = Resample(16000, 24000)
    raw = make_input("resample:prompt16", (2, 2400), seed=83).to(DEV) * 0.1         # 3600 samples at 24 kHz: 11 frames, curtailed from the left
    cond, noise = make_input("cond", (2, 64, 8), seed=84).to(DEV), make_input("noise", (2, 8, 128), seed=85).to(DEV)
    got = d.sample(length=8, prompt=raw, prompt_sample_hz=16000, cond=cond, noise=noise)
    want = d.sample(length=8, prompt=rs(raw), cond=cond, noise=noise)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, d.sample(length=8, prompt=raw, cond=cond, noise=noise))                      # the rate is not ignored
    lens = [2400, 1500]                                                                # 3600 -> 11 frames, 2250 -> 7 frames
    a = d.sample(length=8, prompt=raw, prompt_sample_hz=16000, prompt_lens=lens, cond=cond, noise=noise)
    b = d.sample(length=8, prompt=rs(raw, lens=lens)[:, :11 * HOP], prompt_lens=[11 * HOP, 7 * HOP], cond=cond, noise=noise)
    assert torch.isfinite(a).all() and torch.equal(a, b)
