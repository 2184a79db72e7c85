"""Host logic of the Aligner's HIP training path on the CPU (no GPU): the fp64 references of tests/aligner_ref64.py against torch autograd
of the composite, the K_EMU measurements behind the GPU bounds, `training.aligner_forward_train` on the emulation backend against the
composite's gradients and the reference's (tests/golden/aligner_grads.pt), `aligner_unsupported_reason`, the default switches, the ABI.
The kernels themselves are checked on the MI355X (tests/test_aligner_training_gpu.py)."""
import os
import re

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, autograd_path, training
from naturalspeech2_pytorch_amd.aligner import Aligner, BinLoss, ForwardSumLoss
from tests import aligner_ref64 as R
from tests.golden.gen import make_input, make_weights
from tests.test_aligner_cpu import _load, rows_to_path

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("ns2_relu_fwd", "ns2_relu_bwd", "ns2_align_attn_bwd_workspace_bytes", "ns2_align_attn_bwd", "ns2_align_losses_workspace_bytes",
               "ns2_align_losses_fwd", "ns2_align_losses_bwd")
TOL = 1e-4            # the bound the other *_training_cpu tests use for the emulated backend (fp32 torch ops both sides)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture()
def emu():
    bk = R.AlignerEmuBackend()
    prev = training.set_backend(bk)
    yield bk
    training.set_backend(prev)


# ---------------------------------------------------------------------------------------------- ABI and keywords
def test_new_abi_names_are_in_the_header_and_in_the_binding():
    hdr = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in hdr and name in _lib.SIGNATURES, name
    src = open(os.path.join(ROOT, "naturalspeech2_pytorch_amd", "csrc", "capi_train.cpp")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    for name in ("relu_fwd", "relu_bwd", "align_attn", "align_attn_bwd", "align_losses_fwd", "align_losses_bwd"):
        assert callable(getattr(training.HipBackend, name)), name
    assert training.aligner_forward_train.__name__ in training.__all__ and training.aligner_unsupported_reason.__name__ in training.__all__


def test_keywords_and_their_defaults():
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    a = Aligner(dim_in=80, dim_hidden=64)
    assert a.train_backend == "composite" and ForwardSumLoss().backend == "composite" and BinLoss().backend == "composite"
    assert ForwardSumLoss(blank_logprob=-2, backend="hip").blank_logprob == -2
    for make in (lambda: Aligner(dim_in=80, dim_hidden=64, train_backend="triton"), lambda: ForwardSumLoss(backend="x"), lambda: BinLoss(backend="x")):
        with pytest.raises(AssertionError):
            make()
    kw = dict(dim=64, depth=1, wavenet_layers=2, wavenet_stacks=1, dim_prompt=512, condition_on_prompt=True, num_latents_m=4)
    for backend in ("composite", "hip"):
        extra = {} if backend == "composite" else dict(aligner_train_backend="hip")
        ns = NaturalSpeech2(Model(**kw), target_sample_hz=24000, timesteps=4, build_aligner=True, build_duration_pitch=True, **extra)
        assert ns.aligner.train_backend == ns.aligner_loss.backend == ns.bin_loss.backend == backend
        assert ns.duration_pitch.train_backend == "composite" and ns.phoneme_enc.train_backend == "composite"


def test_default_switches_take_todays_path(monkeypatch):
    """the backend patched to raise: the defaults never ask for one, and neither do "hip" modules on CPU tensors"""
    def boom(*a, **k):
        raise AssertionError("the HIP training path was entered")
    monkeypatch.setattr(training, "aligner_forward_train", boom)
    monkeypatch.setattr(training.passes, "backend", boom)
    monkeypatch.setattr(training, "backend", boom)
    b, n, T = 2, 9, 30
    tl, ml = torch.tensor([9, 5]), torch.tensor([30, 21])
    x_mask = (torch.arange(n)[None] < tl[:, None])[:, None]
    y_mask = (torch.arange(T)[None] < ml[:, None])[:, None]
    for tb in ("composite", "hip"):                       # CPU tensors always take the composite
        a = Aligner(dim_in=16, dim_hidden=32, attn_channels=16, train_backend=tb)
        x = torch.randn(b, n, 32, requires_grad=True)
        hard, soft, logp, path = a(x, x_mask, torch.randn(b, 16, T), y_mask)
        loss = ForwardSumLoss(backend=tb)(logp, tl, ml) + BinLoss(backend=tb)(path, logp, tl)
        loss.backward()
        assert all(p.grad is not None for p in a.parameters()) and x.grad is not None
        assert not a.train_ready(x, torch.randn(b, 16, T))


# ---------------------------------------------------------------------------------------------- references against torch autograd
def composite_attn(c):
    q, k = c["q"].clone().requires_grad_(True), c["k"].clone().requires_grad_(True)
    B, T, n, C = c["B"], c["T"], c["n"], c["C"]
    d = torch.cdist(q.reshape(B, T, C), k.reshape(B, n, C))[:, None]
    live = torch.arange(n)[None] < c["text_lens"][:, None]
    log = d.masked_fill(~live[:, None, None], -R.FLT_MAX)
    return q, k, log, log.softmax(-1)[:, 0].transpose(1, 2)


@pytest.mark.parametrize("name", ["base", "zero"])
def test_distance_backward_reference_against_autograd(name):
    c = R.attn_inputs(name)
    q, k, log, soft = composite_attn(c)
    assert torch.allclose(log.detach(), R.attn_forward_torch(c["q"], c["k"], c["text_lens"], c["B"])[0], rtol=1e-5, atol=1e-5)
    for mode in R.attn_modes(name):
        g_log, g_soft = R.attn_grads(c, mode)
        out = (0 if g_log is None else (log * g_log).sum()) + (0 if g_soft is None else (soft * g_soft).sum())
        dq_a, dk_a = torch.autograd.grad(out, (q, k), retain_graph=True)
        dq, _, dk, _ = R.attn_bwd(c["q"], c["k"], log.detach(), soft.detach(), g_log, g_soft, c["text_lens"])
        assert torch.isfinite(dq).all() and torch.isfinite(dk).all()
        assert rel(dq_a, dq) < 1e-5 and rel(dk_a, dk) < 1e-5, (name, mode)
        masked = ~(torch.arange(c["n"])[None] < c["text_lens"][:, None]).reshape(-1)
        assert bool((dk[masked] == 0).all())


def test_k_emu_distance_backward():
    worst = dict(attn_dq=0.0, attn_dk=0.0)
    for name in R.ATTN_CASES:
        c = R.attn_inputs(name)
        log, soft = R.attn_forward_torch(c["q"], c["k"], c["text_lens"], c["B"])
        for mode in R.attn_modes(name):
            g = R.attn_grads(c, mode)
            dq, aq, dk, ak = R.attn_bwd(c["q"], c["k"], log, soft, *g, c["text_lens"])
            dq32, _, dk32, _ = R.attn_bwd(c["q"], c["k"], log, soft, *g, c["text_lens"], dtype=torch.float32)
            worst["attn_dq"] = max(worst["attn_dq"], R.k_of(dq32, dq, aq)[0])
            worst["attn_dk"] = max(worst["attn_dk"], R.k_of(dk32, dk, ak)[0])
    print("K_EMU measured:", worst)
    for key, v in worst.items():
        assert v <= R.K_EMU[key], (key, v)


@pytest.mark.parametrize("name", sorted(R.LOSS_CASES))
def test_loss_references_against_the_composite_and_k_emu(name):
    c = R.loss_inputs(name)
    tl, ml = c["text_lens"], c["mel_lens"]
    l64, g64, gmax = R.ctc_torch(c["log"], tl, ml)
    x = c["log"].clone().requires_grad_(True)
    fs = ForwardSumLoss()(x, tl.long(), ml.long())
    g, = torch.autograd.grad(fs, x)
    assert abs(float(fs.detach()) - float(l64)) <= 1e-5 * abs(float(l64)) and rel(g, g64) < 2e-3
    if name == "small":
        assert bool((g64[2] == 0).all()) and float(gmax[2]) == 0        # the infeasible utterance
        assert bool((g64[:, 0, 96:] == 0).all())
    for b in range(c["B"]):
        assert bool((g64[b, 0, int(ml[b]):] == 0).all()) and bool((g64[b, 0, :, int(tl[b]):] == 0).all())
    l32, g32, _ = R.ctc_torch(c["log"], tl, ml, dtype=torch.float32)
    kl, kg = R.ctc_k(l32, g32, l64, g64, gmax)
    bl, al, bg, ag = R.bin_ref(c["log"], c["hard"], tl)
    bl32, _, bg32, _ = R.bin_ref(c["log"], c["hard"], tl, dtype=torch.float32)
    kbl, kbg = R.k_of(bl32.reshape(1), bl.reshape(1), al.reshape(1))[0], R.k_of(bg32, bg, ag)[0]
    print("K_EMU measured:", name, dict(ctc_loss=kl, ctc_grad=kg, bin_loss=kbl, bin_grad=kbg))
    assert kl <= R.K_EMU["ctc_loss"] and kg <= R.K_EMU["ctc_grad"] and kbl <= R.K_EMU["bin_loss"] and kbg <= R.K_EMU["bin_grad"]
    x = c["log"].clone().requires_grad_(True)
    bn = BinLoss()(c["hard"], x, tl.long())
    gb, = torch.autograd.grad(bn, x)
    assert abs(float(bn.detach()) - float(bl)) <= 1e-5 * abs(float(bl)) and rel(gb, bg) < 1e-4
    assert bool((bg[:, 0, :, :][(torch.arange(c["n"])[None] > tl[:, None])[:, None].expand(-1, c["T"], -1)] == 0).all())


def test_k_gpu_is_four_times_the_pin_capped():
    assert [R.k_gpu(k) for k in ("attn_dq", "attn_dk", "ctc_loss", "ctc_grad", "bin_loss", "bin_grad")] == [32, 8, 8, 64, 4, 8]


# ---------------------------------------------------------------------------------------------- the pass on the emulation backend
def golden_case(name):
    fx = _load("aligner_grads.pt")["cases"][name]
    m = Aligner(**fx["kwargs"])
    m.load_state_dict(make_weights(fx["shapes"], seed=fx["weight_seed"]))
    x = make_input("phoneme_enc", fx["x_shape"], seed=fx["input_seed"])
    mel = make_input("mel", fx["mel_shape"], seed=fx["input_seed"])
    return fx, m, x, mel


def run_losses(m, fwd, x, mel, tl, ml, fs=None, bn=None):
    fs, bn = fs or ForwardSumLoss(), bn or BinLoss()
    m.zero_grad()
    x = x.clone().requires_grad_(True)
    hard, soft, logp, path = fwd(x, mel)
    l_fs, l_bin = fs(logp, tl, ml), bn(path.detach(), logp, tl)
    (l_fs + l_bin).backward()
    return l_fs.detach(), l_bin.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, x.grad.clone(), path.detach(), hard


def test_golden_file_stays_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "aligner_grads.pt")) < 900_000
    assert sorted(_load("aligner_grads.pt")["cases"]) == ["c32", "c80"]


@pytest.mark.parametrize("name", ["c80", "c32"])
def test_forward_train_on_the_emulation_gives_the_composite_and_reference_gradients(emu, name):
    fx, m, x, mel = golden_case(name)
    tl, ml = fx["text_lens"], fx["mel_lens"]
    n, T = x.shape[1], mel.shape[-1]
    x_mask = (torch.arange(n)[None] < tl[:, None])[:, None]
    y_mask = (torch.arange(T)[None] < ml[:, None])[:, None]
    ref = run_losses(m, lambda x, mel: m._forward_composite(x, x_mask, mel, y_mask), x, mel, tl, ml)
    got = run_losses(m, lambda x, mel: training.aligner_forward_train(m, x, tl, mel, ml), x, mel, tl, ml)
    assert torch.equal(got[4], ref[4]) and torch.equal(got[4], rows_to_path(fx["rows"], n)) and torch.equal(got[5], fx["hard"].int())
    for other, label in ((ref, "composite"), ((torch.tensor(fx["fs_loss"]), torch.tensor(fx["bin_loss"]), fx["grads"], fx["dx"]), "reference")):
        assert rel(got[0], other[0]) < TOL and rel(got[1], other[1]) < TOL, label
        assert sorted(got[2]) == sorted(other[2])
        for k, g in other[2].items():
            assert rel(got[2][k], g) < TOL, (label, k, rel(got[2][k], g))
        assert rel(got[3], other[3]) < TOL, label
    assert len(got[2]) == 10
    assert emu.calls.count("relu_fwd") == 3 and emu.calls.count("relu_bwd") == 3
    assert emu.calls.count("align_attn") == 1 and emu.calls.count("align_attn_bwd") == 1


def test_mel_gets_a_gradient_when_it_asks(emu):
    fx, m, x, mel = golden_case("c32")
    mel = mel.clone().requires_grad_(True)
    hard, soft, logp, path = training.aligner_forward_train(m, x, fx["text_lens"], mel, fx["mel_lens"])
    ForwardSumLoss()(logp, fx["text_lens"], fx["mel_lens"]).backward()
    g = mel.grad.clone()
    mel2 = mel.detach().clone().requires_grad_(True)
    n, T = x.shape[1], mel.shape[-1]
    x_mask = (torch.arange(n)[None] < fx["text_lens"][:, None])[:, None]
    y_mask = (torch.arange(T)[None] < fx["mel_lens"][:, None])[:, None]
    ForwardSumLoss()(m._forward_composite(x, x_mask, mel2, y_mask)[2], fx["text_lens"], fx["mel_lens"]).backward()
    assert rel(g, mel2.grad) < TOL


def test_aligner_unsupported_reason():
    ok = Aligner(dim_in=80, dim_hidden=64)
    assert training.aligner_unsupported_reason(ok) is None
    assert "float16" in training.aligner_unsupported_reason(Aligner(dim_in=80, dim_hidden=64).half())
    assert "attn_channels=320" in training.aligner_unsupported_reason(Aligner(dim_in=80, dim_hidden=64, attn_channels=320))
    x, y = torch.zeros(1, 1025, 64), torch.zeros(1, 80, 8193)
    assert "n=1025" in training.aligner_unsupported_reason(ok, x=x)
    assert "T=8193" in training.aligner_unsupported_reason(ok, y=y)
    prefix = torch.tensor([[[True, True, False]]])
    holes = torch.tensor([[[True, False, True]]])
    assert training.aligner_unsupported_reason(ok, x_mask=prefix, y_mask=prefix) is None
    assert "x_mask" in training.aligner_unsupported_reason(ok, x_mask=holes)
    assert "y_mask" in training.aligner_unsupported_reason(ok, x_mask=prefix, y_mask=holes)
