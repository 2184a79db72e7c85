"""Aligner and NaturalSpeech2.forward(text=..., mel=..., pitch=...) on the CPU composite against the reference's recorded outputs
(tests/golden/make_golden_aligner.py)."""
import os

import pytest
import torch

from tests.golden.gen import make_weights, make_input

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


def rows_to_path(rows, t_x):
    """[b, t_y] row per column (-1: empty) -> [b, t_x, t_y] 0/1"""
    b, t_y = rows.shape
    r = rows.long()
    path = torch.zeros(b, t_x + 1, t_y)
    path.scatter_(1, torch.where(r < 0, t_x, r)[:, None], 1.)
    return path[:, :t_x]


def mp_value(case):
    """the value of a maximum_path case, rebuilt as make_golden_aligner.mp_value does"""
    shape, seed = case["shape"], case["seed"]
    if case["kind"] == "rand":
        return make_input("mp_value", shape, seed=seed, uniform=True)
    if case["kind"] == "int":
        return torch.randint(0, 4, shape, generator=torch.Generator().manual_seed(seed)).float()
    return torch.full(shape, 0.5)


def lengths_mask(tl, ml, t_x, t_y):
    return (torch.arange(t_x)[None] < tl[:, None])[:, :, None].float() * (torch.arange(t_y)[None] < ml[:, None])[:, None, :].float()


def aligner_inputs(fx):
    x = make_input("phoneme_enc", fx["x_shape"], seed=fx["input_seed"])
    mel = make_input("mel", fx["mel_shape"], seed=fx["input_seed"])
    return x, mel


def build_aligner(fx):
    from naturalspeech2_pytorch_amd.aligner import Aligner
    m = Aligner(**fx["kwargs"]).eval()
    m.load_state_dict(make_weights(fx["shapes"], seed=fx["weight_seed"]))
    return m


def forward_inputs(fx):
    s = fx["input_seed"]
    pitch = 80 + 320 * make_input("pitch", fx["pitch_shape"], seed=s, uniform=True)
    pitch[:, :, ::7] = 0.
    return dict(audio=make_input("audio", fx["audio_shape"], seed=s), text=fx["text"], prompt=make_input("prompt", fx["prompt_shape"], seed=s),
                mel=make_input("mel", fx["mel_shape"], seed=s), pitch=pitch, times=make_input("times", fx["times_shape"], seed=s, uniform=True),
                noise=make_input("noise", fx["noise_shape"], seed=s))


def build_wrapper(fx, **extra):
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    d = NaturalSpeech2(Model(**fx["model_kwargs"]), codec=None, build_aligner=True, build_duration_pitch=True, **fx["wrapper_kwargs"],
                       **extra).eval()
    sd = make_weights(fx["shapes"], seed=fx["weight_seed"])
    d.load_state_dict(sd)
    for enc in (d.prompt_enc, d.phoneme_enc):       # eval() (no dropout) with an autograd graph, as the reference records
        enc.force_autograd = True
    return d


def run_forward(d, fx, inp, dev="cpu", **kw):
    t = {k: v.to(dev) for k, v in inp.items()}
    return d(t["audio"], text=t["text"], text_lens=fx["text_lens"].to(dev), mel=t["mel"], mel_lens=fx["mel_lens"].to(dev),
             prompt=t["prompt"], pitch=t["pitch"], times=t["times"], noise=t["noise"], **kw)


def check_grads(d, fx, rtol):
    """per parameter: the gradient norm within rtol, the sampled elements within 50 rtol of the sample's largest"""
    g = fx["grads"]
    params = dict(d.named_parameters())
    worst = 0.
    for k, norm, idx, vals in zip(g["names"], g["norm"].tolist(), g["idx"].long(), g["vals"]):
        p = params[k]
        assert p.grad is not None, k
        flat = p.grad.detach().cpu().reshape(-1)
        scale = max(float(vals.abs().max()), 1e-30)
        worst = max(worst, float((flat[idx] - vals).abs().max()) / scale)
        assert abs(float(flat.double().norm()) - norm) <= rtol * max(norm, 1e-30), k
    assert worst < 50 * rtol, worst        # single elements of the small phoneme-encoder gradients move more than their norms


@pytest.fixture(scope="module")
def cases():
    return _load("aligner_cases.pt")


def test_maximum_path_composite_equals_the_reference(cases):
    from naturalspeech2_pytorch_amd.aligner import maximum_path
    for c in cases["maximum_path"]:
        b, t_x, t_y = c["shape"]
        path = maximum_path(mp_value(c), lengths_mask(c["text_lens"], c["mel_lens"], t_x, t_y))
        assert torch.equal(path, rows_to_path(c["rows"], t_x)), (c["kind"], c["shape"])
        assert torch.equal(path.sum(-1).int(), c["durations"])


def test_aligner_composite_against_the_reference(cases):
    fx = cases["aligner"]
    m = build_aligner(fx)
    x, mel = aligner_inputs(fx)
    n, T = fx["x_shape"][1], fx["mel_shape"][2]
    x_mask = (torch.arange(n)[None] < fx["text_lens"][:, None])[:, None]
    y_mask = (torch.arange(T)[None] < fx["mel_lens"][:, None])[:, None]
    with torch.no_grad():
        hard, soft, log, path = m(x, x_mask, mel, y_mask)
    assert hard.dtype == torch.int32 and torch.equal(hard, fx["hard"])
    assert torch.equal(path, rows_to_path(fx["rows"], n))
    for got, ref in ((soft, fx["soft"]), (log, fx["log"])):
        live = ref > -1e30
        assert float(((got - ref)[live]).abs().max()) <= 2e-5 * float(ref[live].abs().max())
        assert torch.equal(got[~live], ref[~live])


def test_aligner_state_dict_matches_the_reference(cases):
    fx = cases["aligner"]
    from naturalspeech2_pytorch_amd.aligner import Aligner
    m = Aligner(**fx["kwargs"])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == fx["shapes"]


@pytest.mark.parametrize("kind", ["int", "frac"])
def test_average_over_durations_against_the_reference(cases, kind):
    from naturalspeech2_pytorch_amd.aligner import average_over_durations
    c = cases["average"][kind]
    got = average_over_durations(c["pitch"], c["durs"])
    if kind == "int":
        assert torch.equal(got, c["avg"])
    else:
        assert float((got - c["avg"]).abs().max()) <= 1e-5 * float(c["avg"].abs().max())


def test_default_wrapper_has_no_aligner_and_still_raises():
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    d = NaturalSpeech2(Model(dim=64, depth=1, dim_prompt=512, condition_on_prompt=True), codec=None, target_sample_hz=24000)
    assert not any(k.startswith(("aligner.", "aligner_loss.", "bin_loss.")) for k in d.state_dict())
    with pytest.raises(NotImplementedError, match="Aligner"):
        d(torch.randn(1, 32, 64), text=torch.zeros(1, 5, dtype=torch.long), prompt_enc=torch.randn(1, 16, 512))


def test_wrapper_aligner_keys_match_the_reference():
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx)
    ours = {k: tuple(v.shape) for k, v in d.state_dict().items() if k.startswith("aligner.")}
    ref = {k: v for k, v in fx["shapes"].items() if k.startswith("aligner.")}
    assert ours == ref and len(ours) == 10


@pytest.mark.parametrize("missing", ["mel", "pitch"])
def test_missing_mel_or_pitch_names_the_module(missing):
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx)
    inp = forward_inputs(fx)
    inp[missing] = None
    with pytest.raises(NotImplementedError, match="AudioToMel" if missing == "mel" else "pitch extraction"):
        d(inp["audio"], text=inp["text"], mel=inp["mel"], pitch=inp["pitch"], prompt=inp["prompt"])


def test_text_forward_loss_and_gradients_against_the_reference():
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx)
    inp = forward_inputs(fx)
    text_lens, mel_lens = fx["text_lens"].clone(), fx["mel_lens"].clone()
    loss = run_forward(d, fx, inp)
    assert torch.equal(fx["text_lens"], text_lens) and torch.equal(fx["mel_lens"], mel_lens)   # the caller's lengths are not clamped in place
    assert abs(float(loss) - fx["loss"]) <= 2e-5 * abs(fx["loss"])
    loss.backward()
    check_grads(d, fx, 2e-4)       # small gradients deep in the phoneme encoder: attention arithmetic differs in order
    assert all(p.grad is None for k, p in d.named_parameters() if k.startswith(("aligner.", "duration_pitch.")))


def test_return_aux_losses_against_the_reference():
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx, aligner_bin_loss_weight=1.)
    loss, aux = run_forward(d, fx, forward_inputs(fx), return_aux_losses=True)
    assert abs(float(loss) - fx["loss"]) <= 2e-5 * abs(fx["loss"])
    for k in ("duration", "pitch", "bin"):
        assert abs(float(aux[k]) - fx["aux"][k]) <= 2e-5 * abs(fx["aux"][k]), k
    # with the bin term folded in: align = CTC + bin (weight 1)
    assert abs(float(aux["align"]) - (fx["aux"]["align"] + fx["aux"]["bin"])) <= 2e-5 * abs(fx["aux"]["bin"])
    (loss + aux["aux"]).backward()
    assert dict(d.named_parameters())["aligner.aligner.key_layers.0.weight"].grad is not None
    assert dict(d.named_parameters())["duration_pitch.to_pitch_pred.to_pred.0.weight"].grad is not None
