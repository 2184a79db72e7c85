"""DurationPitchPredictor and text-conditioned sampling on the MI355X: the GroupNorm + SiLU kernels against fp64 torch, the
length regulator bit for bit against the composite, the HIP predictor and sample(text=...) against the reference's outputs
(tests/golden/make_golden_duration_pitch.py).  Reads stored fixtures only."""
import os

import pytest
import torch

from tests.golden.gen import make_weights
from tests.test_duration_pitch_cpu import expansion_cases, predictor_inputs, sample_inputs

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


def _gn_ref(x, B, w, b, groups, resid):
    """fp64 GroupNorm(groups, C) + SiLU (+ resid) over token-major rows [B * n, C]"""
    xd = x.double().reshape(B, -1, x.shape[1]).transpose(1, 2)
    y = torch.nn.functional.group_norm(xd, groups, w.double(), b.double(), 1e-5)
    y = torch.nn.functional.silu(y).transpose(1, 2).reshape(x.shape)
    return y + resid.double() if resid is not None else y


GN_CASES = [(1, 77, 512, 0.), (7, 45, 256, 0.), (2, 333, 512, 100.), (7, 130, 256, 100.)]


@pytest.mark.parametrize("B,n,C,offset", GN_CASES)
@pytest.mark.parametrize("with_resid", [False, True])
def test_groupnorm_silu_against_fp64(B, n, C, offset, with_resid):
    """n not a multiple of 64 / 256, B 1 and 7, C 512 and 256, inputs of mean 100 and std 1 (cancellation)"""
    from naturalspeech2_pytorch_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + n)
    x = (torch.randn(B * n, C, generator=g) + offset).cuda()
    w = (1 + 0.3 * torch.randn(C, generator=g)).cuda()
    b = (0.2 * torch.randn(C, generator=g)).cuda()
    resid = torch.randn(B * n, C, generator=g).cuda() if with_resid else None
    ref = _gn_ref(x, B, w, b, 8, resid)
    f, planes = ops.groupnorm_silu(x, B, w, b, 8, resid=resid, precision=3)
    scale = float(ref.abs().max())
    assert float((f.double() - ref).abs().max()) < 1e-5 * scale
    assert float((ops.join(planes).double() - ref).abs().max()) < 1e-5 * scale
    f2 = ops.groupnorm_silu(x, B, w, b, 8, resid=resid)
    assert torch.equal(f, f2)                                       # bit-reproducible


@pytest.mark.parametrize("case", expansion_cases(), ids=lambda c: c[0])
def test_length_regulate_bit_identical_to_composite(case):
    from naturalspeech2_pytorch_amd import ops
    from naturalspeech2_pytorch_amd.autograd_path import length_regulate
    _, dur, pitch, enc, table = case
    ref = length_regulate(dur, pitch, enc, table)
    out = ops.length_regulate(dur.cuda(), pitch.cuda(), enc.cuda(), table.cuda())
    assert out.shape == ref.shape
    assert torch.equal(out.cpu(), ref)


def test_length_regulate_reference_fixture():
    from naturalspeech2_pytorch_amd import ops
    fix = _load("sample_text_d64.pt")
    table = make_weights({"pitch_emb.weight": fix["shapes"]["pitch_emb.weight"]}, seed=fix["weight_seed"])["pitch_emb.weight"]
    out = ops.length_regulate(fix["duration"].cuda(), fix["pitch"].cuda(), fix["phoneme_enc"].cuda(), table.cuda())
    assert torch.equal(out.cpu(), fix["cond"])


def _predictor(fix):
    from naturalspeech2_pytorch_amd import DurationPitchPredictor
    m = DurationPitchPredictor(**fix["kwargs"]).eval()
    m.load_state_dict(dict(make_weights(fix["shapes"], seed=fix["weight_seed"]), **fix["overrides"]), strict=True)
    return m.cuda()


def _rel(a, b):
    return float((a.cpu() - b).abs().max() / b.abs().max())


def test_hip_predictor_d512():
    """precision "exact" against the reference, bound 1e-4 relative; measured on an MI355X: durations 5.0e-6, pitch 2.7e-6"""
    fix = _load("duration_pitch_d512.pt")
    m = _predictor(fix)
    with torch.no_grad():
        dur, pitch = m(*(t.cuda() for t in predictor_inputs(fix)))
    assert _rel(dur, fix["duration"]) < 1e-4 and _rel(pitch, fix["pitch"]) < 1e-4
    assert torch.equal(dur.int().cpu(), fix["duration"].int())
    with torch.no_grad():
        dur2, pitch2 = m(*(t.cuda() for t in predictor_inputs(fix)))
    assert torch.equal(dur, dur2) and torch.equal(pitch, pitch2)


@pytest.mark.parametrize("name", ["convblock", "tokens", "k5", "hd128"])
def test_hip_predictor_variants(name):
    """bound 1e-4 relative; measured worst case on an MI355X 1.6e-5 (convblock durations)"""
    fix = _load("duration_pitch_variants.pt")["cases"][name]
    m = _predictor(fix)
    with torch.no_grad():
        dur, pitch = m(*(t.cuda() for t in predictor_inputs(fix)))
    assert _rel(dur, fix["duration"]) < 1e-4 and _rel(pitch, fix["pitch"]) < 1e-4, name


def test_hip_predictor_rejects_training_dropout():
    fix = _load("duration_pitch_variants.pt")["cases"]["convblock"]
    m = _predictor(fix).train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="dropout"):
        m(*(t.cuda() for t in predictor_inputs(fix)))


@pytest.fixture(scope="module")
def text_wrapper():
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    fix = _load("sample_text_d64.pt")
    d = NaturalSpeech2(Model(**fix["model_kwargs"]), codec=None, build_duration_pitch=True, **fix["wrapper_kwargs"])
    shapes = {k: tuple(v.shape) for k, v in d.state_dict().items()}
    assert all(fix["shapes"][k] == s for k, s in shapes.items())
    d.load_state_dict(dict(make_weights(shapes, seed=fix["weight_seed"]), **fix["overrides"]), strict=True)
    return fix, d.cuda().eval()


def test_sample_text_cond(text_wrapper):
    """the conditioning sample(text=...) builds: same n_frames as the reference, values within 1e-4 (measured 1.9e-5)"""
    fix, d = text_wrapper
    with torch.no_grad():
        cond = d.text_to_cond(fix["text"].cuda(), d.prompt_enc(sample_inputs(fix)[0].cuda()))
    assert cond.shape == fix["cond"].shape
    assert float((cond.cpu() - fix["cond"]).abs().max()) < 1e-4 * float(fix["cond"].abs().max())


@pytest.mark.parametrize("cond_scale", [1.0, 1.5])
def test_sample_text_end_to_end(text_wrapper, cond_scale):
    """latents within 1e-3 of the reference's (measured 1.9e-5 at cond_scale 1.0 and 1.5)"""
    fix, d = text_wrapper
    prompt, noise = sample_inputs(fix)
    out = d.sample(length=fix["length"], prompt=prompt.cuda(), text=fix["text"].cuda(), noise=noise.cuda(), cond_scale=cond_scale)
    ref = fix["outputs"][cond_scale]
    assert out.shape == ref.shape
    assert float((out.cpu() - ref).abs().max()) < 1e-3 * float(ref.abs().max())
