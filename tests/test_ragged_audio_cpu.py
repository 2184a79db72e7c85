"""Ragged RAW AUDIO on the CPU (include/ns2hip_audio.h; ns2_rvq_ce_lens in include/ns2hip_train.h): the three entries of the C ABI and what they refuse, the
composites of `AudioToMel(lens=)`, `PitchExtractor(lens=)` and `codec.rq(..., lens=)`, and `NaturalSpeech2(ragged_audio=True)`:
`forward(raw audio, audio_lens=samples)` with and without the RVQ cross-entropy term, the text-conditioned branch, what is refused, and
the Trainer.  The definition under test: what utterance i yields in the padded batch is what it yields alone, cut to its length; what lies
at or behind a length (NaN included) reaches no value and no gradient before it; what is returned at or behind a length is an exact 0."""
import ctypes
import os
import subprocess

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, AudioToMel, EncodecWrapperHIP, NaturalSpeech2, PitchExtractor
from naturalspeech2_pytorch_amd.training import Trainer
from tests import pitch_ref64 as PR
from tests.golden.gen import make_input
from tests.test_audio_to_mel_cpu import _load, build_wrapper, raw_inputs, tiny_codec
from tests.test_ragged_training_cpu import _loss_and_grads, _model, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUT_BAR = 1e-4                                           # the project's output bar (tests/test_ragged_training_cpu.py)
NAN = float("nan")
HOP = EncodecWrapperHIP.seq_len_multiple_of                 # 320 samples per codec frame


# ---- 1. the C ABI
def test_ragged_audio_header_is_plain_c_parses_and_the_library_exports_it(tmp_path):
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert {"ns2_audio_to_mel_lens", "ns2_pitch_yin_lens"} <= set(_lib.header_symbols("ns2hip_audio.h"))     # each beside its base entry
    assert "ns2_rvq_ce_lens" in _lib.header_symbols("ns2hip_train.h")                                        # ... as is this, beside ns2_rvq_ce
    sig = {k: _lib.SIGNATURES[k] for k in ("ns2_audio_to_mel_lens", "ns2_pitch_yin_lens", "ns2_rvq_ce_lens")}
    assert sig["ns2_audio_to_mel_lens"] == (I, [P, I, L, I, I, P, P, P, P, I, I, I, I, P, P, P])
    assert sig["ns2_pitch_yin_lens"] == (I, [P, I, L, I, I, I, I, F, P, P, P])
    assert sig["ns2_rvq_ce_lens"] == (I, [P, P, P, P, P, P, P, P, I, I, P, I, I, I, P, L, P])
    # each is the entry without lengths plus the lengths (ns2_rvq_ce: M replaced by B, n, row_lens)
    mel, yin, ce = (_lib.SIGNATURES[k][1] for k in ("ns2_audio_to_mel", "ns2_pitch_yin", "ns2_rvq_ce"))
    assert sig["ns2_audio_to_mel_lens"][1] == mel[:-1] + [P] + mel[-1:] and sig["ns2_pitch_yin_lens"][1] == yin[:-1] + [P] + yin[-1:]
    assert sig["ns2_rvq_ce_lens"][1] == ce[:8] + [I, I, P] + ce[9:]
    src = tmp_path / "abi.c"
    src.write_text('#include "ns2hip_audio.h"\n#include "ns2hip_train.h"\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)
    lib = _lib.load()                                       # raises unless the library exports them
    assert all(getattr(lib, k).argtypes == v[1] for k, v in sig.items())


def test_the_three_entries_refuse_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error"""
    lib = _lib.load()
    p = 1 << 20                                             # addresses that are compared against null and never read

    def refused(name, rc, word):
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith(name + ":") and word in msg, (name, rc, msg)

    def mel(**kw):
        a = dict(audio=p, B=2, L=4096, n_fft=1024, hop=160, lens=p, out=p)
        a.update(kw)
        return lib.ns2_audio_to_mel_lens(a["audio"], a["B"], a["L"], a["n_fft"], a["hop"], p, p, p, p, 300, 80, 400, 1, a["out"], a["lens"], None)
    for kw, word in ((dict(lens=None), "sample_lens is null"), (dict(audio=None), "bad arguments"), (dict(B=0), "bad arguments"),
                     (dict(n_fft=1000), "power of two"), (dict(hop=0), "hop_length"), (dict(L=512), "n_fft / 2")):
        refused("ns2_audio_to_mel_lens", mel(**kw), word)

    def yin(**kw):
        a = dict(audio=p, B=2, L=4000, hop=160, tau_max=339, lens=p, f0=p)
        a.update(kw)
        return lib.ns2_pitch_yin_lens(a["audio"], a["B"], a["L"], 24000, a["hop"], 37, a["tau_max"], 0.1, a["f0"], a["lens"], None)
    for kw, word in ((dict(lens=None), "sample_lens is null"), (dict(f0=None), "null pointer"), (dict(B=65536), "B must be"),
                     (dict(L=0), "L must be"), (dict(hop=0), "hop_length"), (dict(tau_max=1025), "tau_max <= 1024")):
        refused("ns2_pitch_yin_lens", yin(**kw), word)

    def ce(**kw):
        a = dict(x=p, B=2, n=5, lens=p, Q=8, C=1024, D=128, quant=None, ws=None, nbytes=0)
        a.update(kw)
        return lib.ns2_rvq_ce_lens(a["x"], p, p, p, p, p, a["quant"], None, a["B"], a["n"], a["lens"], a["Q"], a["C"], a["D"], a["ws"], a["nbytes"], None)
    for kw, word in ((dict(lens=None), "row_lens is null"), (dict(x=None), "null pointer"), (dict(B=0), "must be positive"),
                     (dict(n=0), "must be positive"), (dict(B=1 << 20, n=1 << 12), "fit an int"), (dict(D=64), "codebook_dim 128"),
                     (dict(C=100), "codebook_size % 64"), (dict(quant=p), "needs a workspace"),
                     (dict(quant=p, ws=p, nbytes=lib.ns2_rvq_ce_workspace_bytes(10, 8, 1) - 1), "needs a workspace")):
        refused("ns2_rvq_ce_lens", ce(**kw), word)
    assert lib.ns2_rvq_ce_workspace_bytes(10, 8, 1) == 10 * 8 * 8


# ---- 2. the composites of AudioToMel(lens=) and PitchExtractor(lens=)
def _behind(x, lens, value=NAN):
    y = x.clone()
    for i, s in enumerate(lens):
        y[i, s:] = value
    return y


def test_audio_to_mel_composite_with_lens_is_the_utterance_alone():
    mod = AudioToMel(n_mels=40, n_fft=256, win_length=256, hop_length=64)
    lens = [1024, 640, 192]
    x = make_input("ragged_audio:mel", (3, 1024), seed=11)
    got = mod(x, lens=torch.tensor(lens))
    assert got.shape == (3, 40, 17) and got.dtype == torch.float32
    for i, s in enumerate(lens):
        T = 1 + s // 64
        assert torch.equal(got[i, :, :T], mod(x[i, :s])) and torch.count_nonzero(got[i, :, T:]) == 0
    assert not torch.equal(got[1], mod(x)[1])               # without the lengths the reflection is taken at the end of the batch
    assert torch.equal(mod(_behind(x, lens), lens=lens), got)
    for bad in (torch.tensor([1., 2., 3.]), [1024, 640], torch.tensor([[1024, 640, 192]])):
        with pytest.raises(ValueError, match="one integer sample count per utterance"):
            mod(x, lens=bad)


def test_pitch_composite_with_lens_is_the_utterance_alone():
    fs, hop = 8000, 80
    mod = PitchExtractor(sample_rate=fs, hop_length=hop)
    lens, L = [2400, 1600, 800], 2400
    x = torch.stack([PR.tone(f, fs, L) for f in (150., 220., 330.)])
    got = mod(x, lens=torch.tensor(lens))
    assert got.shape == (3, 31) and got.dtype == torch.float32
    for i, s in enumerate(lens):
        T = 1 + s // hop
        alone = mod(x[i, :s])
        assert torch.equal(got[i, :T], alone) and torch.count_nonzero(got[i, T:]) == 0
        assert int((alone > 0).sum()) > 0                   # ... and not an equality of zeros
    assert not torch.equal(got[1], mod(x)[1])
    assert torch.equal(mod(_behind(x, lens), lens=lens), got)
    with pytest.raises(ValueError, match="one integer sample count per utterance"):
        mod(x, lens=[2400, 1600])


# ---- 3. codec.rq(..., lens=), composite
def _rq(Q=4, C=64, D=128):
    cb = make_input("ragged_audio:codebooks", (Q, C, D), seed=12) * (0.5 ** torch.arange(Q, dtype=torch.float32))[:, None, None]
    return EncodecWrapperHIP(cb).rq


def test_rq_composite_with_lens_is_the_mean_of_the_solo_losses():
    rq = _rq()
    lens, b, n = [20, 13, 1], 3, 20
    x = make_input("ragged_audio:rq:x", (b, n, 128), seed=13)
    idx = (make_input("ragged_audio:rq:idx", (b, n, 4), seed=13, uniform=True) * 64).long().clamp(max=63)

    def run(x, idx, **kw):
        xr = x.clone().requires_grad_(True)
        quant, loss = rq(xr, idx, **kw)
        loss.backward()
        return loss.detach(), xr.grad, quant.detach()
    loss, g, quant = run(x, idx, lens=torch.tensor(lens))
    solo = [run(x[i:i + 1, :s], idx[i:i + 1, :s]) for i, s in enumerate(lens)]
    want = torch.stack([s[0] for s in solo]).mean()
    e_loss = rel(loss, want)
    e_grad = max(rel(g[i, :s], solo[i][1][0] / b) for i, s in enumerate(lens))
    print(f"rq(lens=) composite vs the solos: loss {e_loss:.3e}, worst gradient {e_grad:.3e}")
    assert e_loss < OUTPUT_BAR and e_grad < OUTPUT_BAR
    for i, s in enumerate(lens):
        assert torch.count_nonzero(g[i, s:]) == 0 and torch.count_nonzero(quant[i, s:]) == 0
        assert torch.equal(quant[i, :s], solo[i][2][0])
    xn, idxn = _behind(x, lens), _behind(idx, lens, -1)
    loss_n, g_n, quant_n = run(xn, idxn, lens=lens)
    assert torch.equal(loss_n, loss) and torch.equal(g_n, g) and torch.equal(quant_n, quant)
    assert rel(run(x, idx)[0], want) > 1e-3                # without the lengths the padding is in the mean: the test sees it
    with pytest.raises(ValueError, match="one integer frame count per utterance"):
        rq(x, idx, lens=[20, 13])


# ---- 4. the wrapper
LENS_F = [12, 9, 7]                                         # frames; 7 = EncodecWrapperHIP.min_causal_prompt_frames
LENS_S = [f * HOP for f in LENS_F]


def stub_codec(dim=64, Q=2, C=64):
    """tiny_codec (a stub encoder that makes frame t of samples [320 t, 320 t + dim): causal) with codebooks of the model's width and an RVQ
    encode in plain torch, so that `codec.rq` has codes to score"""
    codec = tiny_codec(dim)
    cb = make_input("ragged_audio:stub:codebooks", (Q, C, dim), seed=14) * (0.5 ** torch.arange(Q, dtype=torch.float32))[:, None, None]
    codec.rvq.codebooks = cb

    def encode(lat):
        r, codes, emb = lat, [], torch.zeros_like(lat)
        for q in range(Q):
            k = torch.cdist(torch.nan_to_num(r), cb[q][None].expand(r.shape[0], -1, -1)).argmin(-1)
            codes.append(k)
            r, emb = r - cb[q][k], emb + cb[q][k]
        return torch.stack(codes, -1), lat
    codec.rvq.encode = encode
    return codec


def _raw_wrapper(**kw):
    return NaturalSpeech2(_model("uncond", ragged_training=True), codec=stub_codec(), timesteps=2, objective="eps", min_snr_loss_weight=False,
                          ragged_audio=True, **kw)


@pytest.mark.parametrize("ce_weight", [0., 0.1])
def test_raw_audio_with_audio_lens_is_the_mean_of_the_solo_raw_losses(ce_weight):
    d = _raw_wrapper(rvq_cross_entropy_loss_weight=ce_weight)
    assert d.ragged_audio is True
    b, n = 3, max(LENS_F)
    raw = 0.1 * make_input("ragged_audio:raw", (b, n * HOP), seed=15)
    t, noise = make_input("times", (b,), seed=15, uniform=True), make_input("noise", (b, n, 64), seed=16)
    loss, g = _loss_and_grads(d, raw, audio_lens=torch.tensor(LENS_S), times=t, noise=noise)
    solo, gs = [], None
    for i, (s, f) in enumerate(zip(LENS_S, LENS_F)):
        l, gi = _loss_and_grads(d, raw[i:i + 1, :s], times=t[i:i + 1], noise=noise[i:i + 1, :f])
        solo.append(l)
        gs = gi if gs is None else {k: gs[k] + gi[k] for k in gs}
    worst = ("loss", rel(loss, torch.stack(solo).mean()))
    for k in gs:
        worst = max(worst, (k, rel(g[k], gs[k] / b)), key=lambda z: z[1])
    print(f"raw audio_lens (RVQ weight {ce_weight}) loss and gradients vs the mean of the solos: worst {worst[0]} {worst[1]:.3e}")
    assert torch.isfinite(loss) and worst[1] < OUTPUT_BAR, worst
    loss_n, g_n = _loss_and_grads(d, _behind(raw, LENS_S), audio_lens=LENS_S, times=t, noise=_behind(noise, LENS_F))
    assert torch.equal(loss_n, loss) and all(torch.equal(g_n[k], g[k]) for k in g)
    assert rel(_loss_and_grads(d, raw, times=t, noise=noise)[0], torch.stack(solo).mean()) > 1e-3    # the test sees the padding
    if ce_weight:                                           # the term is in the loss, and with latents and codes= it takes the frame counts
        assert rel(loss, _loss_and_grads(_raw_wrapper(), raw, audio_lens=LENS_S, times=t, noise=noise)[0]) > 1e-3
        lat, codes, _ = d.codec(raw, return_encoded=True)
        loss_l = d(lat, codes=codes, audio_lens=LENS_F, times=t, noise=noise)
        assert torch.equal(loss_l.detach(), loss)


# ---- 5. the text-conditioned branch
class _Seen(Exception):
    pass


def test_text_branch_hands_the_aligner_each_utterances_own_mel_pitch_and_mel_lens(monkeypatch):
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx, ragged_audio=True, build_pitch_extractor=True)
    inp = raw_inputs(fx)
    audio = inp["audio"]                                    # [2, 15360]
    lens = [audio.shape[-1], 31 * HOP]
    seen = []

    def spy(text, text_lens, mel, mel_lens, pitch, prompt_enc, return_aux_losses=False):
        seen.append((mel, mel_lens, pitch))
        raise _Seen
    monkeypatch.setattr(d, "text_forward_cond", spy)
    common = dict(times=inp["times"], noise=inp["noise"])
    with pytest.raises(_Seen):
        d(_behind(audio, lens), text=inp["text"], prompt=inp["prompt"], audio_lens=torch.tensor(lens), **common)
    mel, mel_lens, pitch = seen.pop()
    assert mel_lens.tolist() == [1 + s // d.mel_hop_length for s in lens] and pitch.shape == (2, 1, mel.shape[-1])
    for i, s in enumerate(lens):
        with pytest.raises(_Seen):
            d(audio[i:i + 1, :s], text=inp["text"][i:i + 1], prompt=inp["prompt"][i:i + 1], times=inp["times"][i:i + 1])
        mel_i, mel_lens_i, pitch_i = seen.pop()
        T = mel_i.shape[-1]
        assert mel_lens_i is None and T == int(mel_lens[i])
        assert torch.equal(mel[i, :, :T], mel_i[0]) and torch.count_nonzero(mel[i, :, T:]) == 0
        assert torch.equal(pitch[i, :, :T], pitch_i[0]) and torch.count_nonzero(pitch[i, :, T:]) == 0
        assert int((pitch_i > 0).sum()) >= 0
    # a given mel / pitch / mel_lens is the caller's
    with pytest.raises(_Seen):
        d(audio, text=inp["text"], prompt=inp["prompt"], pitch=inp["pitch"], mel_lens=torch.tensor([5, 6]), audio_lens=lens, **common)
    mel, mel_lens, pitch = seen.pop()
    assert mel_lens.tolist() == [5, 6] and pitch is inp["pitch"]


# ---- 6. what is refused
def test_refusals():
    lat = make_input("latents", (3, 12, 64), seed=17)
    raw = torch.zeros(3, 12 * HOP)
    off = NaturalSpeech2(_model("uncond", ragged_training=True), codec=stub_codec(), timesteps=2, rvq_cross_entropy_loss_weight=0.1)
    assert off.ragged_audio is False
    with pytest.raises(NotImplementedError, match="audio_lens with raw audio: the frozen codec's encode of a padded batch is not shown to equal"):
        off(raw, audio_lens=LENS_S)
    with pytest.raises(NotImplementedError, match="ns2_rvq_ce averages over all frames, it takes no per-utterance lengths"):
        off(lat, codes=torch.zeros(3, 12, 2, dtype=torch.long), audio_lens=LENS_F)
    with pytest.raises(NotImplementedError, match="prompt_lens in training"):
        off(lat, audio_lens=LENS_F, prompt_lens=[3] * 3)
    d = _raw_wrapper()
    with pytest.raises(NotImplementedError, match="prompt_lens in training"):
        d(raw, audio_lens=LENS_S, prompt_lens=[3] * 3)
    for bad in ([12 * HOP, 9 * HOP + 1, 7 * HOP], [12 * HOP, 0, 7 * HOP], [13 * HOP, 9 * HOP, 7 * HOP]):
        with pytest.raises(ValueError, match="positive multiple of the codec's seq_len_multiple_of"):
            d(raw, audio_lens=bad)
    with pytest.raises(ValueError, match="positive multiple of the codec's seq_len_multiple_of"):
        d(raw[:, :-1], audio_lens=LENS_S)
    with pytest.raises(ValueError, match="at least 7 codec frames"):
        d(raw, audio_lens=torch.tensor([12 * HOP, 9 * HOP, 6 * HOP]))
    with pytest.raises(ValueError, match="integers"):
        d(raw, audio_lens=torch.tensor([3840., 2880., 2240.]))
    with pytest.raises(ValueError, match="one frame count per utterance"):
        d(raw, audio_lens=LENS_S[:2])
    plain = NaturalSpeech2(_model("uncond"), codec=stub_codec(), timesteps=2, ragged_audio=True)
    with pytest.raises(NotImplementedError, match="ragged_training"):      # Model's own error comes through
        plain(raw, audio_lens=LENS_S)


# ---- 7. the Trainer
class _TorchAdam(torch.optim.Adam):
    """HipAdam steps on HIP kernels only and refuses CPU parameters, so here the Trainer's loop drives torch's Adam behind the three calls
    it makes besides zero_grad / step (the real optimizer takes the same batches in tests/test_ragged_audio_gpu.py)"""

    def bind(self, *a):
        pass

    def mark(self):
        pass


def test_trainer_takes_dict_batches_of_raw_audio_with_audio_lens(tmp_path):
    d = _raw_wrapper(rvq_cross_entropy_loss_weight=0.1)
    batches = [{"audio": 0.1 * make_input("ragged_audio:trainer", (3, 12 * HOP), seed=s), "audio_lens": torch.tensor(lens)}
               for s, lens in ((18, LENS_S), (19, LENS_S[::-1]))]
    tr = Trainer(d, dataloader=batches, train_lr=1e-3, train_num_steps=2, use_ema=False, save_and_sample_every=0, results_folder=tmp_path,
                 use_graph=False)
    tr.opt = _TorchAdam([p for p in d.parameters() if p.requires_grad], lr=1e-3)
    seen = []
    fwd = d.forward
    d.forward = lambda *a, **kw: seen.append((a, kw)) or fwd(*a, **kw)
    before = [p.detach().clone() for p in d.model.parameters()]
    losses = [float(tr.train_step()) for _ in range(2)]
    assert tr.step == 2 and all(l == l and abs(l) < float("inf") for l in losses)
    assert [sorted(kw) for a, kw in seen] == [["audio", "audio_lens"]] * 2 and not any(a for a, kw in seen)
    assert [kw["audio_lens"].tolist() for a, kw in seen] == [LENS_S, LENS_S[::-1]]
    assert any(not torch.equal(a, p) for a, p in zip(before, d.model.parameters()))
