"""Ragged prompts and text on the CPU: its entries of the C ABI (include/ns2hip_frontend.h; ns2_model_prepare_cond_lens in include/ns2hip.h), the composite restatement of the
rule its kernels follow -- every front-end output of utterance i of a padded batch equals what utterance i gives alone with its text cut
to text_lens[i] and its prompt cut to prompt_lens[i] --, and the keyword rules of NaturalSpeech2.sample(prompt_lens=)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, Model, NaturalSpeech2
from naturalspeech2_pytorch_amd.autograd_path import (duration_pitch_autograd, model_forward_autograd,
                                                     speech_prompt_encoder_autograd)
from naturalspeech2_pytorch_amd.duration_pitch import DurationPitchPredictor
from naturalspeech2_pytorch_amd.encoders import SpeechPromptEncoder
from tests.golden.gen import make_weights, make_input

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL = 1e-5            # composite against composite, batch against alone: the bound of tests/test_ragged_cpu.py's sampler comparison
ENTRIES = ["ns2_groupnorm_silu_lens", "ns2_mean_rows_lens", "ns2_model_prepare_cond_lens", "ns2_zero_rows_lens"]


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


# ---- the C ABI
def test_front_header_parses_and_the_library_exports_it():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert set(ENTRIES) - {"ns2_model_prepare_cond_lens"} <= set(_lib.header_symbols("ns2hip_frontend.h"))
    assert "ns2_model_prepare_cond_lens" in _lib.header_symbols("ns2hip.h")          # a Model entry: beside ns2_model_prepare_cond
    S = {**_lib.ABI["ns2hip_frontend.h"].signatures, **_lib.ABI["ns2hip.h"].signatures}
    assert S["ns2_groupnorm_silu_lens"] == (I, [P, I, I, I, I, P, P, F, P, P, P, P, P, I, I, P, L, P])
    assert S["ns2_zero_rows_lens"] == (I, [P, L, I, I, P, P])
    assert S["ns2_mean_rows_lens"] == (I, [P, I, I, I, P, P, P])
    assert S["ns2_model_prepare_cond_lens"] == (I, [P, P, I, P, P, I, I, I, I, P, P, L, P])
    _lib.load()                                                              # raises unless the library exports them


def test_c99_caller_includes_the_fifth_header_and_links(tmp_path):     # (ns2hip_frontend.h, the second of five now)
    if shutil.which("gcc") is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs gcc and the built library")
    src = tmp_path / "front_caller.c"
    src.write_text(r'''
#include <stdio.h>
#include "ns2hip.h"
#include "ns2hip_frontend.h"
int main(void) {
  int lens[2] = {3, 1};
  int r0 = ns2_groupnorm_silu_lens(0, 2, 8, 32, 8, 0, 0, 1e-5f, 0, lens, 0, 0, 0, 32, 3, 0, 0, 0);
  int r1 = ns2_zero_rows_lens(0, 64, 2, 8, lens, 0);
  int r2 = ns2_mean_rows_lens(0, 2, 8, 32, lens, 0, 0);
  int r3 = ns2_model_prepare_cond_lens(0, 0, 8, lens, 0, 8, 0, 2, 8, 0, 0, 0, 0);
  printf("%d %d %d %d\n", r0, r1, r2, r3);
  printf("%s\n", ns2_last_error());
  return 0;
}
''')
    exe = tmp_path / "front_caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lns2hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out
    lines = out.stdout.splitlines()
    assert lines[0].split() == [str(_lib.NS2_ERR_ARG)] * 4, lines          # null arguments come back as codes
    assert lines[1].startswith("ns2_model_prepare_cond_lens:"), lines


def test_every_entry_refuses_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error"""
    lib = _lib.load()
    fake = 1 << 20                                          # 16-byte aligned addresses that are compared against null and never read
    lens = (ctypes.c_int * 2)(3, 1)

    def refused(rc, who, word):
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith(who + ":") and word in msg, (rc, msg)

    def gn(x=fake, B=2, n=8, C=32, groups=8, out=fake, ldo=32, prec=3, ws=fake, ws_bytes=1 << 20, row_lens=lens, hi=None, lo=None):
        return lib.ns2_groupnorm_silu_lens(x, B, n, C, groups, fake, fake, 1e-5, None, row_lens, out, hi, lo, ldo, prec, ws, ws_bytes, None)
    who = "ns2_groupnorm_silu_lens"
    refused(gn(x=None), who, "bad arguments")
    refused(gn(out=None), who, "bad arguments")
    refused(gn(B=0), who, "bad arguments")
    refused(gn(C=36), who, "multiple of 4")
    refused(gn(prec=5), who, "precision")
    refused(gn(hi=fake, C=48, groups=4, ldo=48), who, "plane output")
    refused(gn(hi=fake, prec=3), who, "lo plane")
    refused(gn(ws_bytes=16), who, "workspace")
    refused(gn(x=fake + 4), who, "aligned")
    refused(gn(B=70000, ws_bytes=1 << 30), who, "65535")
    refused(gn(x=None, row_lens=None), "ns2_groupnorm_silu", "bad arguments")      # without lengths: ns2_groupnorm_silu's own refusal
    who = "ns2_zero_rows_lens"
    refused(lib.ns2_zero_rows_lens(None, 64, 2, 8, lens, None), who, "bad arguments")
    refused(lib.ns2_zero_rows_lens(fake, 64, 2, 8, None, None), who, "bad arguments")
    refused(lib.ns2_zero_rows_lens(fake, 64, 0, 8, lens, None), who, "bad arguments")
    refused(lib.ns2_zero_rows_lens(fake, 24, 2, 8, lens, None), who, "16-byte")
    refused(lib.ns2_zero_rows_lens(fake + 8, 64, 2, 8, lens, None), who, "16-byte")
    refused(lib.ns2_zero_rows_lens(fake, 64, 70000, 8, lens, None), who, "65535")
    who = "ns2_mean_rows_lens"
    refused(lib.ns2_mean_rows_lens(None, 2, 8, 32, lens, fake, None), who, "bad arguments")
    refused(lib.ns2_mean_rows_lens(fake, 2, 8, 32, None, fake, None), who, "bad arguments")
    refused(lib.ns2_mean_rows_lens(fake, 2, 8, 0, lens, fake, None), who, "bad arguments")
    refused(lib.ns2_mean_rows_lens(fake, 70000, 8, 32, lens, fake, None), who, "65535")
    who = "ns2_model_prepare_cond_lens"
    refused(lib.ns2_model_prepare_cond_lens(None, fake, 8, lens, fake, 8, 0, 2, 8, fake, fake, 1 << 20, None), who, "null model")
    # (a model handle that is not null is read only after these: `fake` is never dereferenced)
    refused(lib.ns2_model_prepare_cond_lens(fake, fake, 8, lens, fake, 8, 0, 0, 8, fake, fake, 1 << 20, None), who, "B and N")
    refused(lib.ns2_model_prepare_cond_lens(fake, None, 8, lens, fake, 8, 0, 2, 8, fake, fake, 1 << 20, None), who, "are required")
    refused(lib.ns2_model_prepare_cond_lens(fake, fake, 0, lens, fake, 8, 0, 2, 8, fake, fake, 1 << 20, None), who, "are required")
    refused(lib.ns2_model_prepare_cond_lens(fake, fake, 8, lens, fake, 8, 0, 2, 8, None, fake, 1 << 20, None), who, "are required")


# ---- the composite: batch against alone
def _edit_padding(t, lens, fill, seed=9):
    """a copy of t [b, n, ...] whose rows from lens[i] on hold other finite random values (fill=None) or `fill`"""
    out = t.clone()
    g = torch.Generator().manual_seed(seed)
    for i, l in enumerate(lens):
        if l < t.shape[1]:
            out[i, l:] = torch.randn(out[i, l:].shape, generator=g) * 3 if fill is None else fill
    return out


def _check_batch_against_alone(run, alone, inputs, lens_of, outputs_len):
    """run(inputs, with_lens) -> tuple of outputs [b, n, ...]; alone[i] -> the same tuple for utterance i alone; inputs: dict name ->
    tensor, lens_of: name -> lengths of the float inputs whose padding is edited; outputs_len: the lengths of the output rows"""
    edited = {k: (_edit_padding(v, lens_of[k], None) if k in lens_of else v) for k, v in inputs.items()}
    nan = {k: (_edit_padding(v, lens_of[k], float("nan")) if k in lens_of else v) for k, v in inputs.items()}
    with torch.no_grad():
        y, y_edit, y_nan = run(inputs, True), run(edited, True), run(nan, True)
        leaky, leaky_edit = run(inputs, False), run(edited, False)
    worst_leak = 0.
    for o, (a, b, c) in enumerate(zip(y, y_edit, y_nan)):
        for i, n in enumerate(outputs_len):
            for name, t in (("lengths", a), ("edited padding", b), ("NaN padding", c)):
                e = rel(t[i:i + 1, :n], alone[i][o])
                print(f"output {o} utterance {i} ({n} rows), {name}: batch vs alone {e:.3e}")
                assert e < TOL, (o, i, name, e)
            worst_leak = max(worst_leak, rel(leaky_edit[o][i:i + 1, :n], leaky[o][i:i + 1, :n]))
    print(f"without lengths the edit of the padding moves the valid rows by {worst_leak:.3e}")
    assert worst_leak > 1e-3                                  # the test can see a leak
    return y


def test_speech_prompt_encoder_composite_batch_against_alone():
    torch.manual_seed(0)
    enc = SpeechPromptEncoder(dim_codebook=32, dims=(32, 64, 32), depth=1, heads=2, dim_head=32).eval()
    lens = [20, 1, 4, 13]
    x = torch.randn(4, 20, 32)
    with torch.no_grad():
        alone = [(speech_prompt_encoder_autograd(enc, x[i:i + 1, :n]),) for i, n in enumerate(lens)]
    run = lambda inp, with_lens: (speech_prompt_encoder_autograd(enc, inp["x"], lens=torch.tensor(lens) if with_lens else None),)   # noqa: E731
    y, = _check_batch_against_alone(run, alone, dict(x=x), dict(x=lens), lens)
    for i, n in enumerate(lens):
        assert torch.count_nonzero(y[i, n:]) == 0            # rows behind a length are exactly 0
    with torch.no_grad():                                     # the module's own keyword takes the same route on the CPU; a list is accepted
        assert torch.equal(enc(x, lens=lens), y)


@pytest.mark.parametrize("use_resnet_block", [True, False])
def test_duration_pitch_composite_batch_against_alone(use_resnet_block):
    torch.manual_seed(1)
    dp = DurationPitchPredictor(dim=32, dim_hidden=32, depth=2, heads=2, dim_head=32, dropout=0., use_resnet_block=use_resnet_block).eval()
    with torch.no_grad():
        for tr in (dp.to_duration_pred, dp.to_pitch_pred):
            tr.to_pred[0].bias.fill_(2.0)                     # keep the ReLU heads away from an all-zero output
        for p in dp.to_pitch_pred.parameters():
            p.add_(0.01 * torch.randn_like(p))                # the two trunks start as copies: make them differ
    tl, pl = [12, 8, 9, 1], [10, 1, 8, 5]
    x, pr = torch.randn(4, 12, 32), torch.randn(4, 10, 32)
    with torch.no_grad():
        alone = [tuple(t[..., None] for t in duration_pitch_autograd(dp, x[i:i + 1, :a], pr[i:i + 1, :b])) for i, (a, b) in enumerate(zip(tl, pl))]

    def run(inp, with_lens):
        kw = dict(text_lens=torch.tensor(tl), prompt_lens=torch.tensor(pl)) if with_lens else {}
        return tuple(t[..., None] for t in duration_pitch_autograd(dp, inp["x"], inp["pr"], **kw))
    d, p = _check_batch_against_alone(run, alone, dict(x=x, pr=pr), dict(x=tl, pr=pl), tl)
    assert d.abs().sum() > 0 and p.abs().sum() > 0
    for i, n in enumerate(tl):
        assert torch.count_nonzero(d[i, n:]) == 0 and torch.count_nonzero(p[i, n:]) == 0
    with torch.no_grad():
        # either keyword alone: the other side counts as full
        only_t = duration_pitch_autograd(dp, x, pr, text_lens=torch.tensor(tl))
        both_t = duration_pitch_autograd(dp, x, pr, text_lens=torch.tensor(tl), prompt_lens=torch.full((4,), 10))
        only_p = duration_pitch_autograd(dp, x, pr, prompt_lens=torch.tensor(pl))
        both_p = duration_pitch_autograd(dp, x, pr, text_lens=torch.full((4,), 12), prompt_lens=torch.tensor(pl))
        for a, b in zip(only_t + only_p, both_t + both_p):
            assert rel(a, b) < TOL
        got = dp(x, pr, text_lens=tl, prompt_lens=pl)         # the module's keywords, on the CPU
        assert torch.equal(got[0], d[..., 0]) and torch.equal(got[1], p[..., 0])


def test_model_composite_prompt_lens_batch_against_alone():
    kw = dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)
    m = Model(**kw).eval()
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    x = make_input("x", (3, 24, 64), seed=2)
    t = make_input("times", (3,), seed=2, uniform=True)
    prompt = make_input("prompt", (3, 11, 48), seed=2)
    cond = make_input("cond", (3, 48, 24), seed=2)
    pl = [11, 1, 5]
    with torch.no_grad():
        alone = [(model_forward_autograd(m, x[i:i + 1], t[i:i + 1], prompt=prompt[i:i + 1, :n], cond=cond[i:i + 1], cond_drop_prob=0.),)
                 for i, n in enumerate(pl)]

    def run(inp, with_lens):
        return (model_forward_autograd(m, x, t, prompt=inp["prompt"], cond=cond, cond_drop_prob=0.,
                                       prompt_lens=torch.tensor(pl) if with_lens else None),)
    _check_batch_against_alone(run, alone, dict(prompt=prompt), dict(prompt=pl), [24, 24, 24])
    with torch.no_grad():                                     # the null branch ignores the lengths
        a = model_forward_autograd(m, x, t, prompt=prompt, cond=cond, cond_drop_prob=1., prompt_lens=torch.tensor(pl))
        b = model_forward_autograd(m, x, t, prompt=prompt, cond=cond, cond_drop_prob=1.)
    assert torch.equal(a, b)


# ---- keyword rules
UNFUSED = dict(schedule_kwargs=dict(start=-3.0, end=3.0, tau=1.0))     # the schedule on the host: no HIP update kernel in the loop


@pytest.fixture
def wrapper():
    """a conditional NaturalSpeech2 whose four front-end modules are substituted by recording functions with TODAY's signatures unless
    `ragged` is set, the way tests/test_ragged_cpu.py substitutes them"""
    m = Model(dim=64, depth=1, dim_prompt=32, condition_on_prompt=True, num_latents_m=8).eval()
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2, build_duration_pitch=True, duration_pitch_dim=32,
                       pitch_emb_pp_hidden_dim=32, dim_codebook=32, **UNFUSED)
    g = torch.Generator().manual_seed(4)
    enc, p_enc = torch.randn(2, 6, 32, generator=g), torch.randn(2, 5, 32, generator=g)
    dur = torch.tensor([[2.2, 1.0, 0.4, 3.9, 1.0, 2.0], [1.0, 2.7, 1.1, 2.0, 5.0, 1.0]])
    pitch = torch.rand(2, 6, generator=g) * 400
    seen = []

    def install(ragged):
        if ragged:
            def step(self, x, times, prompt=None, prompt_mask=None, cond=None, cond_drop_prob=None, out=None, cond_row=None, lens=None,
                     prompt_lens=None):
                seen.append(("model", lens, prompt_lens))
                return model_forward_autograd(self, x, times, prompt=prompt, cond=cond, cond_drop_prob=cond_drop_prob, lens=lens,
                                              prompt_lens=prompt_lens)
            d.prompt_enc.forward = lambda x, *, lens=None: (seen.append(("prompt_enc", lens)), p_enc)[1]
            d.phoneme_enc.forward = lambda ids, mask=None: (seen.append(("phoneme_enc", mask)), enc)[1]
            d.duration_pitch.forward = lambda x, prompts, prompt_mask=None, *, text_lens=None, prompt_lens=None: \
                (seen.append(("duration_pitch", text_lens, prompt_lens)), (dur, pitch))[1]
        else:
            def step(self, x, times, prompt=None, prompt_mask=None, cond=None, cond_drop_prob=None, out=None, cond_row=None, lens=None):
                seen.append(("model", lens))
                return model_forward_autograd(self, x, times, prompt=prompt, cond=cond, cond_drop_prob=cond_drop_prob, lens=lens)
            d.prompt_enc.forward = lambda x: (seen.append(("prompt_enc",)), p_enc)[1]
            d.phoneme_enc.forward = lambda ids, mask=None: (seen.append(("phoneme_enc", mask)), enc)[1]
            d.duration_pitch.forward = lambda x, prompts, prompt_mask=None: (seen.append(("duration_pitch",)), (dur, pitch))[1]
        Model._forward_hip = step

    saved = Model._forward_hip
    try:
        yield d, install, seen, torch.randint(0, 100, (2, 6), generator=g), torch.randn(2, 5, 32, generator=g)
    finally:
        Model._forward_hip = saved


def test_sample_prompt_lens_hands_lengths_to_all_four_modules(wrapper):
    d, install, seen, text, latents = wrapper
    install(ragged=True)
    audio, lens = d.sample(length=None, prompt=latents, text=text, text_lens=torch.tensor([6, 3]), prompt_lens=torch.tensor([5, 2]),
                           return_lens=True)
    assert lens.tolist() == [9, 4] and audio.shape == (2, 9, 64)
    by = {}
    for rec in seen:
        by.setdefault(rec[0], []).append(rec[1:])
    assert [l.tolist() for l, in by["prompt_enc"]] == [[5, 2]]
    (mask,), = by["phoneme_enc"]
    assert mask.dtype == torch.bool and mask.sum(dim=1).tolist() == [6, 3] and mask[1].tolist() == [True] * 3 + [False] * 3
    (tl, pl), = by["duration_pitch"]
    assert tl.tolist() == [6, 3] and pl.tolist() == [5, 2]
    assert len(by["model"]) == 2 and all(l.tolist() == [9, 4] and p.tolist() == [5, 2] for l, p in by["model"])
    # a missing text_lens counts as full; prompt_enc= given: the lengths count its rows and the encoder is not called
    del seen[:]
    d.sample(length=7, prompt_enc=torch.randn(2, 5, 32), text=text, prompt_lens=[5, 2])
    names = [r[0] for r in seen]
    assert "prompt_enc" not in names
    tl, pl = next(r[1:] for r in seen if r[0] == "duration_pitch")
    assert tl.tolist() == [6, 6] and pl.tolist() == [5, 2]
    assert next(r[1] for r in seen if r[0] == "phoneme_enc").all()
    assert all(r[1] is None and r[2].tolist() == [5, 2] for r in seen if r[0] == "model")
    with pytest.raises(ValueError, match="prompt_lens"):
        d.sample(length=7, prompt=latents, text=text, prompt_lens=[5, 2, 1])
    with pytest.raises(ValueError, match="prompt_lens"):
        d.sample(length=7, prompt=latents, text=text, prompt_lens=torch.tensor([5., 2.]))


def test_sample_text_lens_alone_calls_the_modules_with_todays_arguments(wrapper):
    d, install, seen, text, latents = wrapper
    install(ragged=False)                                     # substitutes without the new keywords: any of them passed on would raise
    cut, lens = d.sample(length=None, prompt=latents, text=text, text_lens=torch.tensor([6, 3]), return_lens=True)
    assert lens.tolist() == [9, 4] and cut.shape == (2, 9, 64)
    assert [r for r in seen if r[0] != "model"] == [("prompt_enc",), ("phoneme_enc", None), ("duration_pitch",)]
    assert all(r[1].tolist() == [9, 4] for r in seen if r[0] == "model")


def test_autograd_names_the_keywords():
    enc = SpeechPromptEncoder(dim_codebook=32, dims=(32,), depth=1, heads=2, dim_head=32).train()
    with pytest.raises(NotImplementedError, match="lens"):
        enc(torch.zeros(2, 8, 32), lens=torch.tensor([8, 3]))
    dp = DurationPitchPredictor(dim=32, dim_hidden=32, depth=1, heads=2, dim_head=32).train()
    with pytest.raises(NotImplementedError, match="text_lens"):
        dp(torch.zeros(2, 8, 32), torch.zeros(2, 4, 32), text_lens=torch.tensor([8, 3]))
    with pytest.raises(NotImplementedError, match="prompt_lens"):
        dp(torch.zeros(2, 8, 32), torch.zeros(2, 4, 32), prompt_lens=torch.tensor([4, 3]))
    m = Model(dim=64, depth=1, dim_prompt=32, condition_on_prompt=True, num_latents_m=8).train()
    with pytest.raises(NotImplementedError, match="prompt_lens"):
        m(torch.zeros(2, 8, 64), torch.zeros(2), prompt=torch.zeros(2, 4, 32), cond=torch.zeros(2, 32, 8), prompt_lens=torch.tensor([4, 3]))
    with pytest.raises(ValueError, match="prompt_lens"):      # no prompt / an unconditional model
        m.eval()(torch.zeros(2, 8, 64), torch.zeros(2), cond=torch.zeros(2, 32, 8), prompt_lens=torch.tensor([4, 3]))
    with pytest.raises(ValueError, match="prompt_lens"):
        Model(dim=64, depth=1).eval()(torch.zeros(2, 8, 64), torch.zeros(2), prompt_lens=torch.tensor([4, 3]))


def test_raw_audio_prompt_lengths_must_be_multiples_of_the_hop(wrapper):
    d, install, seen, text, _ = wrapper
    install(ragged=True)

    class Codec(torch.nn.Module):
        target_sample_hz, seq_len_multiple_of, codebook_dim = 24000, 4, 64
        calls = []

        def forward(self, x, curtail_from_left=False, return_encoded=True):
            self.calls.append(tuple(x.shape))
            return torch.zeros(x.shape[0], x.shape[1] // 4, 32), None, None

        def decode(self, emb):
            return emb.mean(dim=-1).repeat_interleave(4, dim=-1)[:, None]
    d.codec, d.seq_len_multiple_of = Codec(), 4
    wav = torch.zeros(2, 12)
    for bad in ([12, 6], [12, 0], [16, 8]):
        with pytest.raises(ValueError, match="multiple"):
            d.sample(length=7, prompt=wav, text=text, prompt_lens=bad)
    with pytest.raises(ValueError, match="multiple"):
        d.sample(length=7, prompt=torch.zeros(2, 14), text=text, prompt_lens=[12, 8])
    assert not seen and not Codec.calls                       # refused before anything ran
    d.sample(length=7, prompt=wav, text=text, prompt_lens=[12, 8])
    assert next(r[1] for r in seen if r[0] == "prompt_enc").tolist() == [3, 2]        # frames = samples // hop
    assert all(r[2].tolist() == [3, 2] for r in seen if r[0] == "model")
