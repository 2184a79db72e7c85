"""Resample on the CPU: the fp64 restatement (tests/resample_ref64.py) against an independent witness of its indexing
(scipy.signal.upfirdn on the same taps laid out as one FIR), the properties of the formula, the PyTorch composite against the restatement
within the derived bound, `lens=` on the composite, the keywords `input_sample_hz=` / `prompt_sample_hz=` through the codec wrapper and
NaturalSpeech2, and the header ns2hip_audio.h."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, EncodecWrapperHIP, Resample
from naturalspeech2_pytorch_amd import resample as RS
from tests import resample_ref64 as R
from tests.test_audio_to_mel_cpu import tiny_codec
from tests.test_ragged_audio_cpu import _raw_wrapper
from tests.test_ragged_front_cpu import wrapper  # noqa: F401  (a fixture)
from tests.golden.gen import make_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = EncodecWrapperHIP.seq_len_multiple_of
NAN = float("nan")
PAIR_IDS = [f"{o}to{n}" for o, n in R.PAIRS]


# ---- 1. the restatement
@pytest.mark.parametrize("orig,new", R.PAIRS, ids=PAIR_IDS)
def test_restatement_against_upfirdn(orig, new):
    """the witness: the taps as one FIR h[p down - (i - w) up + shift] = k[p][i], shift = down ceil((w + down - 1) up / down), through
    scipy's polyphase upfirdn; output q of the formula is sample q + shift / down of it.  It shares the table and nothing of the
    restatement's own framing"""
    upfirdn = pytest.importorskip("scipy.signal").upfirdn
    up, down, w, k = R.table64(orig, new)
    T = k.shape[1]
    assert T == 2 * w + down == R.taps_per_phase(orig, new)
    shift = down * math.ceil((w + down - 1) * up / down)
    h = np.zeros(shift + (up - 1) * down + w * up + 1)
    for p in range(up):
        for i in range(T):
            h[p * down - (i - w) * up + shift] = k[p, i]
    for L in (1, down + 1, 5 * down + 3, 777):
        x = R.noise(L, 2, L)
        out, _ = R.resample64(x, orig, new)
        y = upfirdn(h, x.astype(np.float64), up, down, axis=1)
        off = shift // down
        assert out.shape[1] == R.out_len(L, up, down) and np.abs(out).max() > 0
        worst = np.abs(y[:, off:off + out.shape[1]] - out).max()
        assert worst <= 1e-12, (L, worst)


@pytest.mark.parametrize("orig,new", R.PAIRS, ids=PAIR_IDS)
def test_tones_and_dc_come_back(orig, new):
    up, down, _, _ = R.table64(orig, new)
    L, e = 40 * max(up, down) + 2000, R.edge(orig, new)
    for f in (200., 1000.):
        out, _ = R.resample64(R.tone(f, orig, L), orig, new)
        want = 0.5 * np.sin(2 * np.pi * f * np.arange(out.shape[1]) / new)
        worst = np.abs(out[0] - want)[e:-e].max()
        print(f"{orig} -> {new}: {f:.0f} Hz tone, worst error {worst:.2e} of full scale")
        assert worst <= 2e-3, (f, worst)
    out, _ = R.resample64(np.full((1, L), 0.5, dtype=np.float32), orig, new)
    assert np.abs(out[0] - 0.5)[e:-e].max() <= 2e-3


@pytest.mark.parametrize("orig", [48000, 44100])
def test_a_tone_above_the_new_nyquist_is_attenuated(orig):
    new = 24000
    e = R.edge(orig, new)
    out, _ = R.resample64(R.tone(0.75 * new, orig, 30000), orig, new)
    worst = np.abs(out[0])[e:-e].max()
    print(f"{orig} -> {new}: a half-scale tone at {0.75 * new:.0f} Hz comes out at {worst:.2e}")
    assert worst <= 4e-3


@pytest.mark.parametrize("orig,new", R.PAIRS, ids=PAIR_IDS)
def test_silence_and_output_length(orig, new):
    up, down, _, _ = R.table64(orig, new)
    out, S = R.resample64(np.zeros((1, 3 * down + 1), dtype=np.float32), orig, new)
    assert not out.any() and not S.any()
    mod = Resample(orig, new)
    for L in range(1, 2 * down + 4):
        want = math.ceil(up * L / down)
        assert R.resample64(np.ones((1, L), dtype=np.float32), orig, new)[0].shape[1] == want == mod.out_len(L)
        assert RS.resample_composite(torch.ones(1, L), orig, new).shape == (1, want)
    assert mod.out_lens([0, 1, down, down + 1]).tolist() == [0, math.ceil(up / down), up, up + math.ceil(up / down)]


# ---- 2. the composite
@pytest.mark.parametrize("orig,new", R.PAIRS, ids=PAIR_IDS)
def test_composite_against_the_restatement(orig, new):
    """F.conv1d does not promise one ascending chain per output (a blocked or vectorised sum): held to twice the derived bound, as
    tests/resample_ref64.py argues"""
    up, down, w, k = R.table64(orig, new)
    T = k.shape[1]
    mod = Resample(orig, new)
    assert (mod.up, mod.down, mod.width) == (up, down, w) and not list(mod.parameters()) and not list(mod.buffers())
    assert np.array_equal(RS.resample_table(orig, new)[3].float().numpy(), k.astype(np.float32))      # the table, rounded once
    worst = 0.
    for L in (1, w, w + 1, down - 1, down, down + 1, 7 * down + 3):
        if L < 1:
            continue
        x = R.noise(100 + L, 3, L)
        ref, S = R.resample64(x, orig, new)
        got = mod(torch.from_numpy(x))
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        ratio = (np.abs(got.double().numpy() - ref) / (2 * R.bound(S, T))).max()
        worst = max(worst, ratio)
        assert ratio <= 1, (L, ratio)
    print(f"{orig} -> {new}: composite against the restatement, worst error / (2 x bound) = {worst:.3f}")
    x = torch.from_numpy(R.noise(5, 2, 3, 50))
    assert torch.equal(mod(x), mod(x.reshape(6, 50)).reshape(2, 3, -1))                               # leading dimensions are kept
    assert Resample(24000, 24000)(x) is x                                                             # equal rates: unchanged


def test_composite_runs_under_autograd():
    x = torch.from_numpy(R.noise(6, 2, 300)).requires_grad_()
    y = Resample(48000, 24000)(x)
    assert y.requires_grad
    y.square().sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0


@pytest.mark.parametrize("orig,new", [(48000, 24000), (16000, 24000), (44100, 24000)], ids=["48k", "16k", "44k1"])
def test_composite_lens_is_the_utterance_alone(orig, new):
    mod = Resample(orig, new)
    L = 6 * mod.down + 5
    lens = [L, 2 * mod.down + 1, 1, 0, L + 9]
    x = torch.from_numpy(R.noise(7, len(lens), L))
    got = mod(x, lens=lens)
    assert got.shape == (len(lens), mod.out_len(L))
    for i, s in enumerate(lens):
        s = min(s, L)
        n = mod.out_len(s)
        assert mod.out_lens(torch.tensor(lens).clamp(max=L))[i] == n
        if s:
            assert torch.equal(got[i, :n], mod(x[i:i + 1, :s])[0]), i
        assert torch.count_nonzero(got[i, n:]) == 0
    assert not torch.equal(got[1], mod(x)[1])                                                        # the lengths are seen
    behind = x.clone()
    for i, s in enumerate(lens):
        behind[i, s:] = NAN
    assert torch.equal(mod(behind, lens=torch.tensor(lens)), got)
    with pytest.raises(ValueError, match="lens"):
        mod(x, lens=[1., 2., 3., 4., 5.])
    with pytest.raises(ValueError, match="lens"):
        mod(x, lens=[1, 2])


# ---- 3. the interface
def test_codec_forward_takes_input_sample_hz():
    codec = tiny_codec(64)
    raw = 0.1 * make_input("resample:raw", (2, 20 * HOP + 33), seed=3)
    emb, codes, _ = codec(raw, input_sample_hz=48000)
    emb24, _, _ = codec(raw)
    assert emb24.shape[1] == 20 and emb.shape[1] == 10
    by_hand, codes_h, _ = codec(Resample(48000, 24000)(raw))
    assert torch.equal(emb, by_hand) and torch.equal(codes, codes_h)
    assert torch.equal(codec(raw, input_sample_hz=24000)[0], emb24) and torch.equal(codec(raw, input_sample_hz=None)[0], emb24)
    left = codec(raw, curtail_from_left=True, input_sample_hz=48000)[0]                              # resampled, then curtailed
    assert torch.equal(left, codec(Resample(48000, 24000)(raw), curtail_from_left=True)[0]) and not torch.equal(left, emb)
    lat = torch.zeros(2, 5, 64)
    with pytest.raises(ValueError, match="input_sample_hz"):
        codec(lat, input_sample_hz=48000)
    assert codec(lat, input_sample_hz=24000)[0].shape == lat.shape


def test_forward_takes_input_sample_hz():
    d = _raw_wrapper()
    raw = 0.1 * make_input("resample:raw", (2, 24 * HOP + 100), seed=4)
    t, noise = make_input("times", (2,), seed=4, uniform=True), make_input("noise", (2, 12, 64), seed=5)
    got = d(raw, input_sample_hz=48000, times=t, noise=noise)
    want = d(Resample(48000, 24000)(raw), times=t, noise=noise)
    assert torch.isfinite(got) and torch.equal(got, want)
    assert not torch.equal(got, d(raw[:, :12 * HOP], times=t, noise=noise))                          # the rate is not ignored
    assert torch.equal(d(raw[:, :12 * HOP], input_sample_hz=24000, times=t, noise=noise), d(raw[:, :12 * HOP], times=t, noise=noise))
    with pytest.raises(ValueError, match="input_sample_hz"):
        d(torch.zeros(2, 12, 64), input_sample_hz=48000, times=t, noise=noise)


def test_forward_converts_ragged_lengths_and_checks_them():
    """48 k -> 24 k: lengths of 2 * (9 hop + 10) and 2 * (7 hop + 50) input samples are 9 and 7 frames, and the padded input length is no
    multiple of the hop.  The batch is the mean of the utterances alone, each resampled by hand"""
    d = _raw_wrapper()
    rs = Resample(48000, 24000)
    lens = [2 * (9 * HOP + 10), 2 * (7 * HOP + 50) + 1]
    assert (rs.out_lens(lens) // HOP * HOP).tolist() == [9 * HOP, 7 * HOP]
    raw = 0.1 * make_input("resample:ragged", (2, lens[0] + 7), seed=6)
    assert raw.shape[1] % HOP and rs.out_len(raw.shape[1]) % HOP
    t, noise = make_input("times", (2,), seed=6, uniform=True), make_input("noise", (2, 9, 64), seed=7)
    seen = []
    check = d.codec.forward
    d.codec.forward = lambda x, **kw: (seen.append(x.clone()), check(x, **kw))[1]
    got = d(raw, audio_lens=lens, input_sample_hz=48000, times=t, noise=noise)
    batch, = seen
    assert batch.shape == (2, 9 * HOP)
    solo = []
    for i, (s, f) in enumerate(zip(lens, (9, 7))):
        alone = rs(raw[i:i + 1, :s])
        assert torch.equal(batch[i, :f * HOP], alone[0, :f * HOP]) and torch.count_nonzero(batch[i, rs.out_len(s):]) == 0
        solo.append(d(alone, times=t[i:i + 1], noise=noise[i:i + 1, :f]))
    assert abs(float(got.detach()) - float(torch.stack(solo).mean().detach())) <= 1e-4 * abs(float(got.detach()))
    behind = raw.clone()
    behind[1, lens[1]:] = NAN
    assert torch.equal(d(behind, audio_lens=torch.tensor(lens), input_sample_hz=48000, times=t, noise=noise), got)
    with pytest.raises(ValueError, match="at least 7 codec frames"):                                  # 6 frames after conversion
        d(raw, audio_lens=[lens[0], 2 * 7 * HOP - 2], input_sample_hz=48000, times=t, noise=noise)


def test_sample_takes_prompt_sample_hz(wrapper):  # noqa: F811
    d, install, seen, text, _ = wrapper
    install(ragged=True)

    class Codec(torch.nn.Module):
        target_sample_hz, seq_len_multiple_of, codebook_dim = 24000, HOP, 64
        calls = []

        def forward(self, x, curtail_from_left=False, return_encoded=True):
            self.calls.append(x.clone())
            return torch.zeros(x.shape[0], x.shape[1] // HOP, 32), None, None

        def decode(self, emb):
            return emb.mean(dim=-1).repeat_interleave(HOP, dim=-1)[:, None]
    d.codec, d.seq_len_multiple_of = Codec(), HOP
    rs = Resample(16000, 24000)
    raw = 0.1 * make_input("resample:prompt", (2, 2 * HOP + 11), seed=8)                              # 16 kHz: 3 frames and a bit at 24 kHz
    noise = make_input("noise", (2, 7, 64), seed=9)
    got = d.sample(length=7, prompt=raw, text=text, prompt_sample_hz=16000, noise=noise)
    want = d.sample(length=7, prompt=rs(raw), text=text, noise=noise)
    assert torch.equal(got, want) and torch.equal(Codec.calls[0], Codec.calls[1]) and Codec.calls[0].shape == (2, rs.out_len(raw.shape[1]))
    assert torch.equal(d.sample(length=7, prompt=raw, text=text, prompt_sample_hz=24000, noise=noise),
                       d.sample(length=7, prompt=raw, text=text, noise=noise)) and Codec.calls[-1].shape == raw.shape
    # prompt_lens count input samples: 2 hop + 11 -> ceil(1.5 (2 hop + 11)) = 977 -> 3 frames; hop + 3 -> 485 -> 1 frame
    del seen[:], Codec.calls[:]
    lens = [2 * HOP + 11, HOP + 3]
    d.sample(length=7, prompt=raw, text=text, prompt_sample_hz=16000, prompt_lens=lens, noise=noise)
    assert (rs.out_lens(lens) // HOP * HOP).tolist() == [3 * HOP, HOP]
    assert next(r[1] for r in seen if r[0] == "prompt_enc").tolist() == [3, 1]
    assert Codec.calls[0].shape == (2, 3 * HOP) and torch.equal(Codec.calls[0][1, :HOP], rs(raw[1:, :lens[1]])[0, :HOP])
    with pytest.raises(ValueError, match="multiple"):                                                 # 0 frames after conversion
        d.sample(length=7, prompt=raw, text=text, prompt_sample_hz=16000, prompt_lens=[lens[0], 100], noise=noise)
    with pytest.raises(ValueError, match="prompt_sample_hz"):
        d.sample(length=7, prompt=torch.zeros(2, 5, 32), text=text, prompt_sample_hz=16000, noise=noise)


# ---- 4. the C ABI
def test_resample_header_is_plain_c_parses_and_the_library_exports_it(tmp_path):
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "ns2hip_audio.h" in _lib.HEADERS and list(_lib.ABI) == list(_lib.HEADERS)
    assert {"ns2_resample", "ns2_resample_frames_per_block", "ns2_resample_lens"} <= set(_lib.header_symbols("ns2hip_audio.h"))
    sig = {k: v for k, v in _lib.ABI["ns2hip_audio.h"].signatures.items() if k.startswith("ns2_resample")}
    assert len(sig) == 3 and all(_lib.SIGNATURES[k] == v for k, v in sig.items())
    assert sig["ns2_resample"] == (I, [P, I, L, I, I, I, P, P, L, P])
    assert sig["ns2_resample_lens"] == (I, [P, I, L, I, I, I, P, P, L, P, P])
    assert sig["ns2_resample_frames_per_block"] == (I, [I, I, I])
    assert sum(k in t.signatures for t in _lib.ABI.values() for k in sig) == 3                      # no name in two headers
    assert _lib.header_symbols() == sorted(_lib.SIGNATURES)
    with pytest.raises(_lib.Ns2Error, match="already declared"):                                    # a name an earlier header has is refused
        (tmp_path / "first.h").write_text("int ns2_version(void);\n")
        (tmp_path / "dup.h").write_text("int ns2_version(void);\n")
        _lib.load_abi(str(tmp_path), ("first.h", "dup.h"))
    src = tmp_path / "abi.c"
    src.write_text('#include "ns2hip_audio.h"\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)
    lib = _lib.load()                                                                               # raises unless the library exports them
    assert all(getattr(lib, k).argtypes == v[1] and getattr(lib, k).restype == v[0] for k, v in sig.items())


def test_frames_per_block_and_refusals_are_host_arithmetic():
    lib = _lib.load()
    for orig, new in R.PAIRS:
        up, down, w, k = R.table64(orig, new)
        F = lib.ns2_resample_frames_per_block(up, down, w)
        assert F > 0 and F % 4 == 0 and 4 * (F * down + 2 * w + 8) <= 64 * 1024, (orig, new, F)
        assert Resample(orig, new).hip_supported()
    assert lib.ns2_resample_frames_per_block(640, 639, 7) > 0 and lib.ns2_resample_frames_per_block(1, 640, 192) > 0      # T = 1024
    for up, down, w in ((641, 1, 7), (1, 641, 7), (1, 640, 193), (0, 2, 13), (1, 0, 13), (1, 2, -1)):
        assert lib.ns2_resample_frames_per_block(up, down, w) == 0, (up, down, w)
    assert not Resample(1, 641).hip_supported()
    p = 1 << 20                                             # addresses that are compared against null and never read
    # no GPU here: an entry that reached a device call would come back with a HIP error, not with these
    assert lib.ns2_resample(p, 1, 100, 641, 1, 7, p, p, 64100, None) == _lib.NS2_UNAVAILABLE
    assert b"641" in lib.ns2_last_error()
    assert lib.ns2_resample_lens(p, 1, 100, 1, 640, 193, p, p, 1, p, None) == _lib.NS2_UNAVAILABLE
    for bad in (dict(audio=None), dict(B=0), dict(L=0), dict(up=0), dict(L_out=51), dict(audio=p + 2)):
        a = dict(audio=p, B=1, L=100, up=1, down=2, w=13, taps=p, out=p, L_out=50)
        a.update(bad)
        assert lib.ns2_resample(a["audio"], a["B"], a["L"], a["up"], a["down"], a["w"], a["taps"], a["out"], a["L_out"], None) == _lib.NS2_ERR_ARG, bad
    assert lib.ns2_resample_lens(p, 1, 100, 1, 2, 13, p, p, 50, None, None) == _lib.NS2_ERR_ARG


def test_forward_converts_a_raw_prompts_lengths_under_ragged_conditioning(wrapper):  # noqa: F811
    """forward(prompt=raw, prompt_lens=, input_sample_hz=): with ragged_conditioning the lengths count input samples and reach
    _prompt_frame_lens converted, with the prompt resampled per utterance and cut to whole frames; without it prompt_lens stays the
    tolerated, unused keyword it is at the codec's rate and the whole prompt is resampled"""
    d, _, _, _, _ = wrapper
    d.seq_len_multiple_of = HOP
    rs = Resample(16000, 24000)
    raw = 0.1 * make_input("resample:prompt", (2, 2 * HOP + 11), seed=8)
    lens, got = [2 * HOP + 11, HOP + 3], {}

    class Seen(Exception):
        pass

    def frame_lens(prompt_lens, prompt, prompt_enc, trust_device=False):
        got.update(lens=torch.as_tensor(prompt_lens).tolist(), prompt=prompt)
        raise Seen

    def process(prompt=None):
        got.update(processed=prompt)
        raise Seen
    d._prompt_frame_lens, d.process_prompt = frame_lens, process
    d.ragged_conditioning = True
    with pytest.raises(Seen):
        d(torch.zeros(2, 9, 64), prompt=raw, prompt_lens=lens, input_sample_hz=16000)
    assert got["lens"] == [3 * HOP, HOP] and got["prompt"].shape == (2, 3 * HOP)
    assert torch.equal(got["prompt"], rs(raw, lens=lens)[:, :3 * HOP])
    d.ragged_conditioning = False
    with pytest.raises(Seen):
        d(torch.zeros(2, 9, 64), prompt=raw, prompt_lens=lens, input_sample_hz=16000)
    assert torch.equal(got["processed"], rs(raw))
