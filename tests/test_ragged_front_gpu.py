"""Ragged prompts and text on the MI355X (include/ns2hip_frontend.h): per-utterance lengths through SpeechPromptEncoder,
DurationPitchPredictor, the conditioning of Model and NaturalSpeech2.sample(prompt_lens=).  The definition under test: every front-end
output of utterance i of a padded batch equals what utterance i gives alone with its text cut to text_lens[i] and its prompt cut to
prompt_lens[i] -- so what lies at or beyond a length (NaN included) must not reach what lies before it."""

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, SpeechPromptEncoder, _lib, ops  # noqa: E402
from naturalspeech2_pytorch_amd.autograd_path import duration_pitch_autograd, speech_prompt_encoder_autograd  # noqa: E402
from oracle import ns2_oracle as O  # noqa: E402
from tests import ragged_front_sample as S  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _pad_mask(lens, n):
    """[b, n] bool, True at or beyond each utterance's length"""
    return torch.arange(n, device=DEV)[None] >= torch.as_tensor(lens, device=DEV)[:, None]


def _edited(x, lens, fill=None, seed=70):
    """x [b, n, ...] with the rows at or beyond each utterance's length replaced by other finite random values, or by `fill`"""
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(x.device) * 3 if fill is None else torch.full_like(x, fill)
    pad = _pad_mask(lens, x.shape[1])
    return torch.where(pad.reshape(pad.shape + (1,) * (x.ndim - 2)), other, x)


def _seeded(module, seed):
    module.load_state_dict(make_weights({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed=seed))
    return module


# ------------------------------------------------------------------------------------------------ 1. GroupNorm with lengths
def _gn_case(B, n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n, C, generator=g).to(DEV) + 3.
    resid = torch.randn(B, n, C, generator=g).to(DEV)
    w = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    b = (0.2 * torch.randn(C, generator=g)).to(DEV)
    return x, resid, w, b


@pytest.mark.parametrize("C,lens", [(256, [300, 128, 129, 1, 77]), (64, [300, 128, 129, 1, 77])])
@pytest.mark.parametrize("with_resid,want_f32,precision", [(True, True, 3), (False, False, 4), (True, True, 2), (False, True, None)])
def test_groupnorm_lens_is_bit_equal_to_the_utterance_alone(C, lens, with_resid, want_f32, precision):
    """C = 256: cg = 32, 128 rows per statistics chunk, 3 chunks, 16-row apply blocks -- lengths on a chunk boundary, one row past it, one
    row, inside the first chunk.  C = 64: cg = 8, one chunk of 512 rows.  Padding rows (and their residual) are NaN."""
    B, n = 5, 300
    x, resid, w, b = _gn_case(B, n, C, seed=C)
    xn, rn = _edited(x, lens, NAN), _edited(resid, lens, NAN)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(want_f32=want_f32, precision=precision)
    out = ops.groupnorm_silu(xn.reshape(B * n, C), B, w, b, 8, resid=rn.reshape(B * n, C) if with_resid else None, lens=kl, **kw)
    outs = out if isinstance(out, tuple) else (out,)
    for i, l in enumerate(lens):
        solo = ops.groupnorm_silu(x[i, :l].contiguous(), 1, w, b, 8, resid=resid[i, :l].contiguous() if with_resid else None, **kw)
        solo = solo if isinstance(solo, tuple) else (solo,)
        for o, s in zip(outs, solo):
            ob, sb = (o.buf, s.buf) if isinstance(o, ops.Planes) else (o, s)
            ob = ob.reshape(B, n, -1)[i]
            assert torch.equal(_bits(ob[:l]), _bits(sb)), f"utterance {i} (length {l})"
            assert torch.count_nonzero(_bits(ob[l:])) == 0, f"utterance {i}: rows behind {l} are not zero bits"
    # lengths outside [1, n] are clamped into it; no lengths: the launches of ns2_groupnorm_silu
    bad = ops.groupnorm_silu(xn.reshape(B * n, C), B, w, b, 8, lens=torch.tensor([n + 5, 128, 129, 0, 77], device=DEV))
    good = ops.groupnorm_silu(xn.reshape(B * n, C), B, w, b, 8, lens=kl)
    assert torch.equal(_bits(bad), _bits(good))
    assert torch.equal(ops.groupnorm_silu(x.reshape(B * n, C), B, w, b, 8, lens=None), ops.groupnorm_silu(x.reshape(B * n, C), B, w, b, 8))


# ------------------------------------------------------------------------------------------------ 2. zero rows, masked mean
def test_zero_rows_on_fp32_rows_and_planes():
    B, n, C, lens = 3, 37, 96, [37, 1, 20]
    kl = torch.tensor(lens, device=DEV)
    x = torch.randn(B * n, C, generator=torch.Generator().manual_seed(5)).to(DEV)
    pad = _pad_mask(lens, n).reshape(B * n)
    f = _edited(x.reshape(B, n, C), lens, NAN).reshape(B * n, C).contiguous()
    assert ops.zero_rows(f, B, n, kl) is f
    assert torch.equal(f[~pad], x[~pad]) and torch.count_nonzero(_bits(f[pad])) == 0
    for precision in (3, 4):
        p = ops.split(x, precision=precision)
        before = p.buf.clone()
        p.buf[pad] = NAN                                   # every plane of the padding rows
        ops.zero_rows(p, B, n, kl)
        assert torch.equal(_bits(p.buf[~pad]), _bits(before[~pad])) and torch.count_nonzero(_bits(p.buf[pad])) == 0
        assert torch.count_nonzero(ops.join(p)[pad]) == 0   # all-zero bits are 0.0 in the format
    # clamped: 0 counts as 1, n + 5 as n
    f2 = torch.ones(B * n, C, device=DEV)
    ops.zero_rows(f2, B, n, torch.tensor([n + 5, 0, 20], device=DEV))
    assert torch.equal(f2.reshape(B, n, C)[:, :, 0] == 0, _pad_mask(lens, n))


@pytest.mark.parametrize("n,d", [(37, 48), (300, 300)])
def test_masked_mean_against_fp64(n, d):
    B, lens = 3, [1, n, n // 2 + 1]
    x = _edited(torch.randn(B, n, d, generator=torch.Generator().manual_seed(n)).to(DEV) + 1., lens, NAN).contiguous()
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = torch.empty(B, d, device=DEV)
    _lib.check(_lib.load().ns2_mean_rows_lens(x.data_ptr(), B, n, d, kl.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "ns2_mean_rows_lens")
    for i, l in enumerate(lens):
        ref = x[i, :l].double().mean(dim=0)
        e = rel(out[i], ref)
        print(f"masked mean, {l} of {n} rows: {e:.3e}")
        assert e < 1e-6, (i, e)


# ------------------------------------------------------------------------------------------------ 3. SpeechPromptEncoder
# "hybrid" is a per-site plan of the denoiser alone; the conditioning modules take its op-level arithmetic, "mixed" (half product + fp8
# correction terms), whose bound against fp32 in the existing module tests is 2.5e-4 (tests/test_reference_gpu.py, tests/test_round5_gpu.py)
ENC_TOL = {"exact": 1e-4, "mixed": 2.5e-4}


def _invisible(run, inputs, lens_of, out_lens):
    """run(inputs, with_lens) -> tuple of outputs [b, n, ...].  Replacing the padding of the inputs named in lens_of with other values, and
    with NaN, leaves the output rows before out_lens bit-equal; without lengths the finite edit changes them.  -> the outputs"""
    edit = {k: (_edited(v, lens_of[k]) if k in lens_of else v) for k, v in inputs.items()}
    nan = {k: (_edited(v, lens_of[k], NAN) if k in lens_of else v) for k, v in inputs.items()}
    with torch.no_grad():
        y, y_edit, y_nan = run(inputs, True), run(edit, True), run(nan, True)
        leaky, leaky_edit = run(inputs, False), run(edit, False)
    torch.cuda.synchronize()
    leaked = False
    for o in range(len(y)):
        for i, n in enumerate(out_lens):
            assert torch.isfinite(y[o][i, :n]).all()
            assert torch.equal(y_edit[o][i, :n], y[o][i, :n]), f"output {o} utterance {i}: rows before {n} changed with the padding"
            assert torch.equal(y_nan[o][i, :n], y[o][i, :n]), f"output {o} utterance {i}: NaN padding reached the rows before {n}"
            leaked = leaked or not torch.equal(leaky_edit[o][i, :n], leaky[o][i, :n])
    assert leaked, "without lengths the edit of the padding must reach the valid rows"
    return y, y_nan


@pytest.mark.parametrize("precision", ["exact", "mixed"])
def test_speech_prompt_encoder_padding_cannot_be_seen(precision):
    lens = [150, 1, 4, 129]
    enc = _seeded(SpeechPromptEncoder(64, dims=(64, 128, 64), depth=1, precision=precision), 21).eval()
    x = make_input("prompt_latents", (4, 150, 64), seed=22)
    with torch.no_grad():
        alone = [speech_prompt_encoder_autograd(enc, x[i:i + 1, :n]) for i, n in enumerate(lens)]        # the CPU composite, alone
    enc = enc.to(DEV)
    kl = torch.tensor(lens, device=DEV)
    (y,), (y_nan,) = _invisible(lambda inp, wl: (enc(inp["x"], lens=kl) if wl else enc(inp["x"]),), dict(x=x.to(DEV)), dict(x=lens), lens)
    for i, n in enumerate(lens):
        assert torch.count_nonzero(y[i, n:]) == 0 and torch.count_nonzero(y_nan[i, n:]) == 0             # rows behind a length: exactly 0
        e = rel(y[i:i + 1, :n].cpu(), alone[i])
        print(f"SpeechPromptEncoder {precision} utterance {i} ({n} rows) vs the composite alone: {e:.3e}")
        assert e < ENC_TOL[precision], (i, e)
    with torch.no_grad():                                  # full lengths hide nothing
        full = enc(x.to(DEV), lens=torch.full((4,), 150, device=DEV))
        assert rel(full, enc(x.to(DEV))) < ENC_TOL[precision]


# ------------------------------------------------------------------------------------------------ 4. DurationPitchPredictor
@pytest.mark.parametrize("use_resnet_block", [True, False])
@pytest.mark.parametrize("precision", ["exact", "mixed"])
def test_duration_pitch_padding_cannot_be_seen(use_resnet_block, precision):
    tl, pl = [96, 64, 65, 1], [80, 1, 64, 33]
    dp = _seeded(DurationPitchPredictor(dim=64, dim_hidden=64, depth=2, heads=2, use_resnet_block=use_resnet_block, precision=precision), 31)
    with torch.no_grad():
        dp.to_duration_pred.to_pred[0].bias.fill_(2.5)     # keep the ReLU heads away from an all-zero output
        dp.to_pitch_pred.to_pred[0].bias.fill_(150.)
    dp = dp.eval()
    x, pr = make_input("phonemes", (4, 96, 64), seed=32), make_input("prompts", (4, 80, 64), seed=33)
    with torch.no_grad():
        alone = [duration_pitch_autograd(dp, x[i:i + 1, :a], pr[i:i + 1, :b]) for i, (a, b) in enumerate(zip(tl, pl))]
    dp = dp.to(DEV)
    ktl, kpl = torch.tensor(tl, device=DEV), torch.tensor(pl, device=DEV)

    def run(inp, with_lens):
        return dp(inp["x"], inp["pr"], **(dict(text_lens=ktl, prompt_lens=kpl) if with_lens else {}))
    (d, p), (d_nan, p_nan) = _invisible(run, dict(x=x.to(DEV), pr=pr.to(DEV)), dict(x=tl, pr=pl), tl)
    for i, n in enumerate(tl):
        for t in (d, p, d_nan, p_nan):
            assert torch.count_nonzero(t[i, n:]) == 0      # durations and pitches behind the text's end: exactly 0
        assert d[i, :n].abs().sum() > 0 and p[i, :n].abs().sum() > 0
        ed, ep = rel(d[i:i + 1, :n].cpu(), alone[i][0]), rel(p[i:i + 1, :n].cpu(), alone[i][1])
        print(f"DurationPitchPredictor {precision} resnet={use_resnet_block} utterance {i}: duration {ed:.3e} pitch {ep:.3e} vs the composite alone")
        assert ed < ENC_TOL[precision] and ep < ENC_TOL[precision], (i, ed, ep)
    with torch.no_grad():                                  # either keyword alone: the other side counts as full
        a = dp(x.to(DEV), pr.to(DEV), text_lens=ktl)
        b = dp(x.to(DEV), pr.to(DEV), text_lens=ktl, prompt_lens=torch.full((4,), 80, device=DEV))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5. Model
COND = dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)      # the `cond` config of tests/test_ragged_gpu.py
MODEL_TOL = {"exact": 1e-4, "hybrid": 1e-3}                                                # ... and its tolerances


@pytest.fixture(scope="module", params=["exact", "hybrid"])
def cond_model(request):
    m = Model(**COND, precision=request.param)
    sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)
    m.load_state_dict(sd)
    N = 64
    return dict(m=m.to(DEV).eval(), sd=sd, precision=request.param, N=N, x=make_input("x", (3, N, 64), seed=3).to(DEV),
                t=make_input("times", (3,), seed=3, uniform=True).to(DEV), prompt=make_input("prompt", (3, 40, 48), seed=3).to(DEV),
                cond=make_input("cond", (3, 48, N), seed=3).to(DEV))


PL, FRAMES = [40, 1, 17], [64, 30, 17]


@pytest.mark.parametrize("cond_scale", [1., 1.5])
@pytest.mark.parametrize("with_lens", [False, True])
def test_model_prompt_padding_cannot_be_seen(cond_model, cond_scale, with_lens):
    c = cond_model
    m, x, t, cond = c["m"], c["x"], c["t"], c["cond"]
    kpl = torch.tensor(PL, dtype=torch.int32, device=DEV)
    ragged = dict(lens=torch.tensor(FRAMES, dtype=torch.int32, device=DEV)) if with_lens else {}
    frames = FRAMES if with_lens else [c["N"]] * 3

    def run(inp, wl):
        kw = dict(ragged, prompt_lens=kpl) if wl else ragged
        return (m.forward_with_cond_scale(x, t, prompt=inp["prompt"], cond=cond, cond_scale=cond_scale, **kw).clone(),)
    (y,), _ = _invisible(run, dict(prompt=c["prompt"]), dict(prompt=PL), frames)
    assert m.precision == c["precision"]                    # NaN prompt rows did not trip the range guard
    for i, (n, npr) in enumerate(zip(frames, PL)):
        with torch.no_grad():
            ref = O.model_forward_with_cond_scale(c["sd"], x[i:i + 1, :n].cpu(), t[i:i + 1].cpu(), prompt=c["prompt"][i:i + 1, :npr].cpu(),
                                                  cond=cond[i:i + 1, :, :n].cpu(), cond_scale=cond_scale)
        e = rel(y[i:i + 1, :n].cpu(), ref)
        print(f"Model {c['precision']} cond_scale {cond_scale} lens={with_lens} utterance {i} ({npr} prompt rows) vs the oracle alone: {e:.3e}")
        assert e < MODEL_TOL[c["precision"]], (i, e)


@pytest.mark.parametrize("cond_scale", [1., 1.5])
def test_model_full_prompt_lens_change_nothing_and_the_cache_follows_the_lengths(cond_model, cond_scale):
    c = cond_model
    m, x, t, prompt, cond = c["m"], c["x"], c["t"], c["prompt"], c["cond"]
    f = lambda **kw: m.forward_with_cond_scale(x, t, prompt=prompt, cond=cond, cond_scale=cond_scale, **kw).clone()   # noqa: E731
    with torch.no_grad():
        plain = f()
        assert torch.equal(f(prompt_lens=None), plain)
        assert torch.equal(f(prompt_lens=torch.full((3,), 40, dtype=torch.int32, device=DEV)), plain)
        assert torch.equal(f(prompt_lens=[40, 40, 40]), plain)
        # the conditioning cache must not serve a state computed for other lengths: the same tensor, rewritten in place
        kl = torch.tensor(PL, dtype=torch.int32, device=DEV)
        a = f(prompt_lens=kl)
        kl.copy_(torch.tensor([7, 40, 3], dtype=torch.int32))
        b = f(prompt_lens=kl)
        fresh = f(prompt_lens=torch.tensor([7, 40, 3], dtype=torch.int32, device=DEV))
        assert torch.equal(b, fresh) and not torch.equal(a, b)
        assert torch.equal(b[1], plain[1])                  # utterance 1 now has its full prompt
        with pytest.raises(ValueError, match="prompt_lens"):
            m(x, t, cond=cond, prompt_lens=kl)


# ------------------------------------------------------------------------------------------------ 6. sample(), end to end
@pytest.fixture(scope="module")
def wrapper():
    """the small text-conditioned wrapper, built once, and the precondition on the CPU composite's durations of every utterance alone that
    keeps int(duration) from flipping inside the kernels' tolerance: every duration at least MARGIN from an integer, every utterance at
    least one frame.  -> (the wrapper on the GPU, the utterances' frame totals)"""
    d = S.tiny_wrapper()
    dist, totals = S.precondition(S.alone_durations(d))
    print(f"predicted durations: smallest distance from an integer {dist:.4f}, frame totals {totals}")
    assert dist >= S.MARGIN and min(totals) >= 1, (dist, totals)
    return d.to(DEV), totals


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_sample_ragged_prompts_and_text_against_each_utterance_alone(wrapper, precision):
    d, totals = wrapper
    d.model.precision = precision                          # (re-packs the denoiser; the conditioning modules stay "exact")
    text, latents = (t.to(DEV) for t in S.inputs())
    noise = make_input("noise", (3, max(totals), 64), seed=13)
    kw = dict(length=None, prompt=latents, text=text, text_lens=torch.tensor(S.TEXT_LENS), prompt_lens=torch.tensor(S.PROMPT_LENS),
              noise=noise, return_lens=True)
    out, lens = d.sample(**kw)
    assert lens.tolist() == totals and out.shape == (3, max(totals), 64) and torch.isfinite(out).all()
    graph, glens = d.sample(use_graph=True, **kw)
    assert torch.equal(graph, out) and glens.tolist() == totals
    # the padding of the text (other ids) and of the prompt (NaN) cannot be seen
    text2 = torch.where(_pad_mask(S.TEXT_LENS, 12), (text + 7) % 150, text)
    out2, _ = d.sample(**dict(kw, text=text2, prompt=_edited(latents, S.PROMPT_LENS, NAN)))
    assert torch.equal(out2, out)
    assert d.model.precision == precision
    for i, (n, tl, pl) in enumerate(zip(totals, S.TEXT_LENS, S.PROMPT_LENS)):
        assert torch.count_nonzero(out[i, n:]) == 0
        alone, alens = d.sample(length=None, prompt=latents[i:i + 1, :pl], text=text[i:i + 1, :tl], noise=noise[i:i + 1, :n], return_lens=True)
        assert alens.tolist() == [n]
        e = rel(out[i:i + 1, :n], alone)
        print(f"sample {precision} utterance {i} ({tl} phonemes, {pl} prompt rows, {n} frames): ragged batch vs alone {e:.3e}")
        assert e < MODEL_TOL[precision], (i, e)


def test_raw_audio_prompt_frames_do_not_see_the_padding_samples():
    """sample(prompt_lens=) with a raw-audio prompt counts samples and divides by the hop: right only if the 24 kHz SEANet encoder is causal
    (seanet.py asserts it; its reflect padding is a left prefix).  Prompts of 7 and 8 hops in an 8-hop batch: the shortest the encoder
    takes -- its last convolution (k = 7 at the frame rate) mirrors frames 1 .. 6 into its prefix and refuses an input of fewer than 7
    frames, so for prompts of 2 and 3 hops there is no utterance alone to be equal to, and the mirrored prefix of a batch would read a
    2-hop prompt's padding.  sample() refuses such lengths on the host (EncodecWrapperHIP.min_causal_prompt_frames)."""
    tf = pytest.importorskip("transformers")
    from naturalspeech2_pytorch_amd import EncodecWrapperHIP, NaturalSpeech2
    torch.manual_seed(0)
    hf = tf.EncodecModel(tf.EncodecConfig()).eval().to(DEV)
    with torch.no_grad():
        codec = EncodecWrapperHIP.from_hf(hf, hip_seanet=True).to(DEV).eval()
        hop, least = codec.seq_len_multiple_of, codec.min_causal_prompt_frames
        assert least == 7
        wav = make_input("wav", (2, 8 * hop), seed=14).to(DEV) * 0.1
        lens = [7 * hop, 8 * hop]
        # the encoder's latents [b, n, 128]: a freshly initialised EnCodec has all-zero codebooks, and the RVQ behind works frame by frame
        a = codec.encoder(wav[:, None]).transpose(1, 2).clone()
        b = codec.encoder(_edited(wav, lens, seed=74)[:, None]).transpose(1, 2).clone()
    assert a.shape[:2] == (2, 8) and a.abs().sum() > 0
    assert torch.equal(a[0, :7], b[0, :7]) and torch.equal(a[1], b[1]) and not torch.equal(a[0, 7], b[0, 7])
    check = NaturalSpeech2._prompt_frame_lens

    class Host:                                             # the host check of sample(prompt_lens=), on this codec
        device = DEV
        seq_len_multiple_of = hop
    Host.codec = codec
    assert check(Host, torch.tensor(lens), wav, None).tolist() == [7, 8]
    with pytest.raises(ValueError, match="at least 7 codec frames"):
        check(Host, torch.tensor([2 * hop, 3 * hop]), wav[:, :3 * hop], None)
    with pytest.raises(ValueError, match="multiple"):
        check(Host, torch.tensor([7 * hop + 1, 8 * hop]), wav, None)
