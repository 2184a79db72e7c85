"""The RVQ cross-entropy term's switch and its float64 reference, without a GPU: the reference's own near-tie condition, the fp32 composite
against the bound of tests/rvq_ce_ref64.py (which pins K_EMU, hence the kernel's K of tests/test_rvq_ce_gpu.py), and the fall-back of
`backend="hip"` on CPU tensors."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from naturalspeech2_pytorch_amd import training
from naturalspeech2_pytorch_amd.codec import EncodecWrapperHIP, HipRVQ, ResidualVQCrossEntropy
from naturalspeech2_pytorch_amd.diffusion import NaturalSpeech2
from tests import rvq_ce_ref64 as R


def _composite_rows(x, cb, idx):
    """the composite of codec.py restated with reduction='none' (the module only returns the summed loss) -> row losses [M, Q] fp32"""
    M, Q = idx.shape
    residual, rows = x.reshape(M, -1), []
    for q in range(Q):
        e = cb[q]
        d2 = residual.pow(2).sum(-1, keepdim=True) - 2 * residual @ e.t() + e.pow(2).sum(-1)
        logits = -d2.clamp(min=0).sqrt()
        rows.append(F.cross_entropy(logits, idx[:, q], reduction="none"))
        residual = residual - F.embedding(logits.argmax(dim=-1), e)
    return torch.stack(rows, 1)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_near_tie_condition(name):
    """seeds for which the reference alone leaves out at most 1 % of the (row, stage) pairs"""
    _, _, idx, ref = R.case(name)
    pairs, rows_G, rows_q = R.compared(ref)
    left = 1.0 - pairs.double().mean().item()
    print(f"case {name}: {int((~pairs).sum())} of {pairs.numel()} (row, stage) pairs left out; G rows {int((~rows_G).sum())}, quantized rows {int((~rows_q).sum())}")
    assert left <= R.MAX_LEFT_OUT
    if R.CASES[name][5] == "uniform":
        assert (idx.reshape(-1, idx.shape[-1]) != ref["nearest"]).double().mean() > 0.9      # y and the arg-max differ
    assert torch.isfinite(ref["A_row"]).all() and torch.isfinite(ref["A_G"]).all()


def test_composite_within_k_emu():
    """the existing fp32 composite (the module for loss and G, its restatement for the row losses) meets (*) with the pinned K_EMU"""
    worst = {"row_loss": 0.0, "loss": 0.0, "G": 0.0}
    for name in sorted(R.CASES):
        x, cb, idx, ref = R.case(name)
        M = idx[..., 0].numel()
        pairs, rows_G, rows_q = R.compared(ref)
        rq = ResidualVQCrossEntropy(HipRVQ(cb))
        xg = x.clone().requires_grad_(True)
        out, loss = rq(xg, idx)
        G, = torch.autograd.grad(loss, xg)
        rows = _composite_rows(x, cb, idx.reshape(M, -1))
        k = {"row_loss": R.k_of(rows, ref["row_loss"], ref["A_row"], pairs),
             "loss": R.k_of(loss.detach(), R.mixed_loss(ref, rows), ref["A_loss"]),
             "G": R.k_of(G.reshape(M, -1), ref["G"], ref["A_G"], rows_G[:, None].expand(M, R.D))}
        print(f"case {name}: K of the fp32 composite: " + ", ".join(f"{n} {v:.2f}" for n, v in k.items()))
        assert torch.equal(out.detach().reshape(M, -1)[rows_q], ref["quantized"][rows_q])
        for n, v in k.items():
            worst[n] = max(worst[n], v)
    print("worst: " + ", ".join(f"{n} {v:.2f}" for n, v in worst.items()))
    for n, v in worst.items():
        assert v <= R.K_EMU[n], (n, v)
        assert R.k_gpu(n) <= R.K_CAP


def test_hip_backend_on_cpu_is_the_composite():
    x, cb, idx, _ = R.case("a")
    owner = HipRVQ(cb)
    comp, hip = ResidualVQCrossEntropy(owner), ResidualVQCrossEntropy(owner, backend="hip")
    why = training.rvq_ce_unsupported_reason(hip, x, idx)
    assert why is not None and "CPU" in why
    grads = []
    for rq in (comp, hip):
        xg = x.clone().requires_grad_(True)
        out, loss = rq(xg, idx)
        grads.append((out.detach(), loss.detach(), torch.autograd.grad(loss, xg)[0]))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    # (the other reasons -- dtypes -- come after the device check: exercised on the GPU, tests/test_rvq_ce_gpu.py)


def test_backend_keywords():
    """the switch exists on the three constructors, defaults to the composite, is settable and is threaded through"""
    cb = R.case("a")[1]
    assert inspect.signature(ResidualVQCrossEntropy.__init__).parameters["backend"].default == "composite"
    assert inspect.signature(EncodecWrapperHIP.__init__).parameters["rq_backend"].default == "composite"
    assert inspect.signature(EncodecWrapperHIP.from_hf).parameters["rq_backend"].default == "composite"
    assert inspect.signature(NaturalSpeech2.__init__).parameters["rvq_ce_backend"].default is None
    assert EncodecWrapperHIP(cb).rq.backend == "composite"
    codec = EncodecWrapperHIP(cb, rq_backend="hip")
    assert codec.rq.backend == "hip"
    codec.rq.backend = "composite"
    assert codec.rq.backend == "composite"
    with pytest.raises(AssertionError):
        ResidualVQCrossEntropy(HipRVQ(cb), backend="triton")

    from naturalspeech2_pytorch_amd.model import Model
    model = Model(dim=128, depth=1)
    NaturalSpeech2(model, codec=codec, rvq_cross_entropy_loss_weight=0.1)
    assert codec.rq.backend == "composite"                      # None leaves the codec's own
    NaturalSpeech2(model, codec=codec, rvq_cross_entropy_loss_weight=0.1, rvq_ce_backend="hip")
    assert codec.rq.backend == "hip"

    from naturalspeech2_pytorch_amd.compat import hip_backed_codec_class

    class RefCodec(torch.nn.Module):
        def __init__(self):
            raise AssertionError("the reference class's own __init__ must not run")

    assert hip_backed_codec_class(RefCodec)(cb, rq_backend="hip").rq.backend == "hip"
