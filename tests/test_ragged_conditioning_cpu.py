"""Ragged text and prompts in training (include/ns2hip_train.h) on the host: the header and its table, the switches and what
still raises without them, and the host logic of the conditioning passes with lengths -- the autograd Functions run on
`tests/emu_backend_ragged_cond.RaggedCondEmuBackend` (the new backend calls restated in torch from their contract) and every output and
gradient is compared with torch autograd on the composite with the same lengths.  The kernels are checked on the MI355X
(tests/test_ragged_conditioning_gpu.py)."""
import os
import re

import pytest
import torch

from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, NaturalSpeech2, PhonemeEncoder, SpeechPromptEncoder, _lib, autograd_path, training
from naturalspeech2_pytorch_amd.training.functions import GroupNormSiluFn, KeepRowsFn
from tests.emu_backend_ragged_cond import RaggedCondEmuBackend
from tests.golden.gen import make_input, make_weights

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN = float("nan")
TOL = 1e-4            # the bound the emulated backend is held to elsewhere (fp32 torch ops on both sides)
B, N = 4, 24
TEXT_LENS, PROMPT_LENS = [24, 13, 9, 1], [24, 10, 4, 1]


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


@pytest.fixture()
def emu():
    bk = RaggedCondEmuBackend()
    prev = training.set_backend(bk)
    yield bk
    training.set_backend(prev)


def _load(m, seed):
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    return m.train()


def _pad(t, lens, value, dim=1):
    t = t.clone()
    for i, l in enumerate(lens):
        if dim == 1:
            t[i, l:] = value
        else:
            t[i, ..., l:] = value
    return t


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _grads(m, fn, cots):
    for p in m.parameters():
        p.grad = None
    outs = fn()
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    return [o.detach().clone() for o in outs], {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check(got, ref, out_lens):
    (y, g), (yr, gr) = got, ref
    for a, b, ol in zip(y, yr, out_lens):
        assert rel(a, b) < TOL
        if ol is not None:
            assert all(torch.count_nonzero(a[i, l:]) == 0 for i, l in enumerate(ol))
    for k, v in gr.items():
        if v is None or v.norm() == 0:
            assert g[k] is None or g[k].norm() == 0, k
        else:
            assert rel(g[k], v) < TOL, (k, rel(g[k], v))


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    for k, v in a[1].items():
        assert (v is None and b[1][k] is None) or torch.equal(v, b[1][k]), k


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_table_and_entry():
    assert "ns2_groupnorm_silu_bwd_lens" in _lib.header_symbols("ns2hip_train.h")
    res, args = _lib.ABI["ns2hip_train.h"].signatures["ns2_groupnorm_silu_bwd_lens"]
    ref_res, ref_args = _lib.SIGNATURES["ns2_groupnorm_silu_bwd"]
    assert res is ref_res and len(args) == len(ref_args) + 1                        # the entry that exists plus row_lens
    src = open(os.path.join(ROOT, "naturalspeech2_pytorch_amd", "csrc", "capi_train.cpp")).read()
    assert re.search(r'extern "C" int ns2_groupnorm_silu_bwd_lens\(', src)
    kern = open(os.path.join(ROOT, "naturalspeech2_pytorch_amd", "csrc", "duration_pitch.hip")).read()
    assert "gn_bwd_cols_kernel<true>" in kern and "gn_bwd_apply_kernel<true>" in kern and kern.count("void gn_bwd_cols_kernel(") == 1


def test_the_library_exports_the_entry():
    lib_path = os.path.join(ROOT, "naturalspeech2_pytorch_amd", "libns2hip.so")
    if not os.path.exists(lib_path):
        pytest.skip("libns2hip.so is not built")
    assert hasattr(_lib.load(), "ns2_groupnorm_silu_bwd_lens")


# ------------------------------------------------------------------------------------------------ the switches
def test_switches_default_off_and_lengths_under_autograd_still_raise():
    enc = SpeechPromptEncoder(dim_codebook=32, dims=(64, 64), depth=1, heads=1).train()
    dp = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=1).train()
    m = Model(dim=64, depth=1, dim_prompt=32, condition_on_prompt=True, num_latents_m=4).train()
    assert not (enc.ragged_conditioning or dp.ragged_conditioning or m.ragged_conditioning)
    with pytest.raises(NotImplementedError, match="lens"):
        enc(torch.zeros(2, 8, 32), lens=[8, 3])
    with pytest.raises(NotImplementedError, match="text_lens"):
        dp(torch.zeros(2, 8, 64), torch.zeros(2, 4, 64), text_lens=[8, 3])
    with pytest.raises(NotImplementedError, match="prompt_lens"):
        m(torch.zeros(2, 8, 64), torch.zeros(2), prompt=torch.zeros(2, 4, 32), cond=torch.zeros(2, 32, 8), prompt_lens=[4, 3])
    d = NaturalSpeech2(Model(dim=64, depth=1, dim_prompt=512, condition_on_prompt=True, num_latents_m=4, wavenet_layers=2, wavenet_stacks=1),
                       target_sample_hz=24000, timesteps=2, build_duration_pitch=True, ragged_conditioning=True)
    assert all(mod.ragged_conditioning for mod in (d, d.model, d.prompt_enc, d.phoneme_enc, d.duration_pitch))


def test_groupnorm_function_without_lengths_is_todays_call(emu):
    x = make_input("x", (2 * 9, 32), seed=1).requires_grad_(True)
    w, b_ = (make_input(k, (32,), seed=2).requires_grad_(True) for k in ("w", "b"))
    GroupNormSiluFn.apply(x, w, b_, None, 9, 8, 1e-5).sum().backward()
    assert emu.calls == ["groupnorm_silu_fwd", "groupnorm_silu_bwd"]                  # no row_lens keyword reached the backend


# ------------------------------------------------------------------------------------------------ the passes against torch autograd
def test_keep_rows_function_selects_in_both_directions(emu):
    x = _pad(make_input("x", (B, N, 8), seed=3), PROMPT_LENS, NAN).reshape(B * N, 8).requires_grad_(True)
    y = KeepRowsFn.apply(x, N, _i32(PROMPT_LENS))
    y.backward(torch.full_like(y, NAN).masked_fill(torch.isfinite(x.detach()), 1.))
    for t in (y.detach(), x.grad):
        t = t.reshape(B, N, 8)
        assert torch.isfinite(t).all() and all(torch.count_nonzero(t[i, l:]) == 0 for i, l in enumerate(PROMPT_LENS))
    assert torch.equal(x.grad.reshape(B, N, 8)[1, :10], torch.ones(10, 8))


def test_prompt_encoder_pass_with_lengths(emu):
    enc = _load(SpeechPromptEncoder(dim_codebook=32, dims=(64, 96, 64), depth=2, heads=2, dropout=0., ragged_conditioning=True), 85)
    x, cots = make_input("x", (B, N, 32), seed=86), [make_input("proj", (B, N, 64), seed=87)]
    lens = _i32(PROMPT_LENS)
    run = lambda xx: _grads(enc, lambda: (training.speech_prompt_encoder_forward_train(enc, xx, lens=lens),), cots)      # noqa: E731
    got = run(_pad(x, PROMPT_LENS, NAN))
    _same(got, run(_pad(x, PROMPT_LENS, 2.5)))
    _check(got, _grads(enc, lambda: (autograd_path.speech_prompt_encoder_autograd(enc, _pad(x, PROMPT_LENS, NAN), lens=lens),), cots), [PROMPT_LENS])
    assert "attention_masked" in emu.calls and "attention" not in emu.calls and "keep_rows" in emu.calls
    # the module's keyword on the CPU: the composite with the lengths, under autograd
    y = enc(_pad(x, PROMPT_LENS, NAN), lens=PROMPT_LENS)
    assert y.requires_grad and rel(y, got[0][0]) < TOL
    # full lengths the host can see: the call without lengths
    assert torch.equal(enc(x, lens=[N] * B), enc(x))


@pytest.mark.parametrize("name,ids,kw", [("resnet", False, {}), ("convblock_k5", False, dict(use_resnet_block=False, kernel_size=5, depth=1)),
                                         ("resnet_tokens", True, dict(num_phoneme_tokens=40, depth=1, num_convolutions_per_block=1))])
@pytest.mark.parametrize("which", ["both", "text", "prompt"])
def test_predictor_pass_with_lengths(emu, name, ids, kw, which):
    dp = _load(DurationPitchPredictor(**dict(dict(dim=64, dim_hidden=64, heads=2, depth=2, dropout=0.), **kw), ragged_conditioning=True), 91)
    x = torch.randint(0, 40, (B, N), generator=torch.Generator().manual_seed(92)) if ids else make_input("phoneme_enc", (B, N, 64), seed=92)
    pr = make_input("prompt_enc", (B, N, 64), seed=93)
    cots = [make_input("proj0", (B, N), seed=94), make_input("proj1", (B, N), seed=95)]
    lens = {}
    if which in ("both", "text"):
        lens["text_lens"] = _i32(TEXT_LENS)
    if which in ("both", "prompt"):
        lens["prompt_lens"] = _i32(PROMPT_LENS)
    tl, pl = (TEXT_LENS if "text_lens" in lens else [N] * B), (PROMPT_LENS if "prompt_lens" in lens else [N] * B)

    def padded(v):
        return (_pad(x, tl, 7 if v != v else 3) if ids else _pad(x, tl, v)), _pad(pr, pl, v)

    run = lambda xx, pp: _grads(dp, lambda: training.duration_pitch_forward_train(dp, xx, pp, **lens), cots)      # noqa: E731
    got = run(*padded(NAN))
    _same(got, run(*padded(2.5)))
    xn, pn = padded(NAN)
    _check(got, _grads(dp, lambda: autograd_path.duration_pitch_autograd(dp, xn, pn, **lens), cots), [tl, tl])
    assert emu.calls.count("attention_masked") > 0 and "attention" not in emu.calls
    n_gn = emu.calls.count("groupnorm_silu_fwd_lens")
    if kw.get("use_resnet_block", True) and "text_lens" in lens:
        assert n_gn > 0 and emu.calls.count("groupnorm_silu_bwd_lens") == n_gn and "groupnorm_silu_fwd" not in emu.calls
    else:
        assert n_gn == 0


def test_model_pass_with_prompt_lens(emu):
    m = _load(Model(dim=64, depth=1, dim_prompt=48, condition_on_prompt=True, num_latents_m=16, ragged_conditioning=True), 1)
    x, t = make_input("x", (B, 16, 64), seed=2), make_input("times", (B,), seed=2, uniform=True)
    prompt, cond, cots = make_input("prompt", (B, N, 48), seed=2), make_input("cond", (B, 48, 16), seed=2), [make_input("gw", (B, 16, 64), seed=3)]
    lens = _i32(PROMPT_LENS)
    run = lambda pp: _grads(m, lambda: (training.model_forward_train(m, x, t, prompt=pp, cond=cond, cond_drop_prob=0., prompt_lens=lens),), cots)      # noqa: E731
    got = run(_pad(prompt, PROMPT_LENS, NAN))
    _same(got, run(_pad(prompt, PROMPT_LENS, 2.5)))
    ref = _grads(m, lambda: (autograd_path.model_forward_autograd(m, x, t, prompt=_pad(prompt, PROMPT_LENS, NAN), cond=cond, cond_drop_prob=0.,
                                                                  prompt_lens=lens),), cots)
    _check(got, ref, [None])
    emu.calls.clear()
    run(prompt)
    assert emu.calls.count("attention_masked") == 2 and emu.calls.count("attention_bwd_masked") == 0          # the resampler's two layers
    # ... and utterance i is what it gives alone with its prompt cut (the composite on the CPU, through the module's keyword)
    y = m(x, t, prompt=_pad(prompt, PROMPT_LENS, NAN), cond=cond, cond_drop_prob=0., prompt_lens=PROMPT_LENS)
    for i, l in enumerate(PROMPT_LENS):
        alone = m(x[i:i + 1], t[i:i + 1], prompt=prompt[i:i + 1, :l], cond=cond[i:i + 1], cond_drop_prob=0.)
        assert rel(y[i:i + 1], alone) < TOL, i


# ------------------------------------------------------------------------------------------------ the wrapper (the composite, on the CPU)
WB, WN_PH, WT, WN_P = 3, 12, 48, 16
W_TEXT, W_PROMPT, W_MEL = [12, 7, 3], [16, 9, 2], [48, 31, 14]


def _wrapper(switch=True):
    torch.manual_seed(131)
    model = Model(dim=64, depth=1, dim_prompt=64, condition_on_prompt=True, num_latents_m=8, cond_drop_prob=0., ragged_training=True, wavenet_layers=2,
                  wavenet_stacks=1)
    d = NaturalSpeech2(model, codec=None, target_sample_hz=24000, timesteps=2, build_aligner=True, build_duration_pitch=True, dim_codebook=64,
                       aligner_dim_hidden=64, pitch_emb_pp_hidden_dim=64, ragged_conditioning=switch)
    d.phoneme_enc = PhonemeEncoder(num_tokens=150, dim=64, dim_hidden=64, depth=1, heads=1, conv_dropout=0., attn_dropout=0.)
    d.prompt_enc = SpeechPromptEncoder(dim_codebook=64, dims=(64, 64), depth=1, heads=1, dropout=0.)
    d.duration_pitch = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=1, dropout=0.)
    for mod in (d.phoneme_enc, d.prompt_enc, d.duration_pitch):
        mod.ragged_conditioning = switch
    return d.train()


def _wbatch():
    g = torch.Generator().manual_seed(140)
    return dict(audio=make_input("audio", (WB, WT, 64), seed=140), text=torch.randint(0, 150, (WB, WN_PH), generator=g),
                mel=make_input("mel", (WB, 80, WT), seed=141), pitch=80 + 300 * make_input("pitch", (WB, 1, WT), seed=142, uniform=True),
                prompt=make_input("prompt", (WB, WN_P, 64), seed=143), times=make_input("times", (WB,), seed=144, uniform=True),
                noise=make_input("noise", (WB, WT, 64), seed=145))


def _wstep(d, batch, lens):
    d.zero_grad(set_to_none=True)
    loss, aux = d(batch["audio"], return_aux_losses=True, **{k: v for k, v in batch.items() if k != "audio"}, **lens)
    (loss + aux["aux"]).backward()
    return dict(loss=loss.detach().clone(), **{k: v.detach().clone() for k, v in aux.items() if v is not None}), \
        {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in d.named_parameters()}


def test_wrapper_on_the_composite():
    d, batch = _wrapper(), _wbatch()
    lens = dict(text_lens=torch.tensor(W_TEXT), prompt_lens=torch.tensor(W_PROMPT), mel_lens=torch.tensor(W_MEL), audio_lens=torch.tensor(W_MEL))

    def behind(v):
        out = dict(batch, text=_pad(batch["text"], W_TEXT, 7 if v != v else 3), prompt=_pad(batch["prompt"], W_PROMPT, v))
        for k in ("audio", "noise"):
            out[k] = _pad(batch[k], W_MEL, v)
        for k in ("mel", "pitch"):
            out[k] = _pad(batch[k], W_MEL, v, dim=-1)
        return out

    (ta, ga), (tb, gb) = _wstep(d, behind(NAN), lens), _wstep(d, behind(2.5), lens)
    for k in ta:
        assert torch.isfinite(ta[k]) and torch.equal(ta[k], tb[k]), k
    for k, v in ga.items():
        assert (v is None and gb[k] is None) or (torch.isfinite(v).all() and torch.equal(v, gb[k])), k
    # the duration and pitch terms: the mean over the utterances of each one's own term alone
    solo = {"duration": [], "pitch": []}
    for i in range(WB):
        cut = dict(audio=batch["audio"][i:i + 1, :W_MEL[i]], text=batch["text"][i:i + 1, :W_TEXT[i]], mel=batch["mel"][i:i + 1, :, :W_MEL[i]],
                   pitch=batch["pitch"][i:i + 1, :, :W_MEL[i]], prompt=batch["prompt"][i:i + 1, :W_PROMPT[i]], times=batch["times"][i:i + 1],
                   noise=batch["noise"][i:i + 1, :W_MEL[i]])
        t, _ = _wstep(d, cut, {})
        for k in solo:
            solo[k].append(t[k].double())
    for k in solo:
        want = float(torch.stack(solo[k]).mean())
        assert abs(float(ta[k]) - want) <= TOL * abs(want), (k, float(ta[k]), want)
    # prompt_lens together with audio_lens: taken with the switch, refused without it
    with pytest.raises(NotImplementedError, match="prompt_lens in training"):
        _wstep(_wrapper(switch=False), batch, lens)
