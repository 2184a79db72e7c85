"""The Aligner's training kernels on the MI355X: ns2_align_attn_bwd and ns2_align_losses_fwd / _bwd element by element against the fp64
references of tests/aligner_ref64.py under the bounds pinned there, exact zeros where the contract says so, bit-equal repeats; the ReLU
pair; `Aligner(train_backend="hip")` with both HIP losses against the reference's recorded gradients (tests/golden/aligner_grads.pt); and
`NaturalSpeech2(aligner_train_backend="hip")` against the fixture's losses and the composite's gradients on the same GPU."""
import pytest
import torch

from tests import aligner_ref64 as R
from tests.parity_record import record
from tests.test_aligner_cpu import _load, build_wrapper, forward_inputs, rows_to_path, run_forward
from tests.test_aligner_training_cpu import golden_case, run_losses

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)


def rel(a, b):
    """max-abs error over max-abs reference (tests/test_backward_gpu.py's measure for one tensor)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module")
def bk():
    from naturalspeech2_pytorch_amd import training
    return training.HipBackend(3)


# ---------------------------------------------------------------------------------------------- ns2_relu_fwd / ns2_relu_bwd
def test_relu_pair_is_exact(bk):
    g = torch.Generator().manual_seed(3)
    M, C = 70, 80                                        # rows of 80 in a buffer of 96: a row stride larger than the width
    pre = torch.randn(M, 96, generator=g)
    pre[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    dy = torch.randn(M, 96, generator=g)
    y = bk.relu_fwd(pre.cuda()[:, :C], C)
    assert y.shape == (M, 96) and torch.equal(y[:, :C].cpu(), pre[:, :C].clamp(min=0))
    dx = bk.relu_bwd(dy.cuda()[:, :C], pre.cuda()[:, :C], C)
    assert torch.equal(dx[:, :C].cpu(), torch.where(pre[:, :C] > 0, dy[:, :C], torch.zeros(())))


# ---------------------------------------------------------------------------------------------- ns2_align_attn_bwd
@pytest.mark.parametrize("name", sorted(R.ATTN_CASES))
def test_align_attn_bwd_element_bound_zeros_and_repeats(bk, name):
    from naturalspeech2_pytorch_amd import ops
    c = R.attn_inputs(name)
    q, k, tl = c["q"].cuda(), c["k"].cuda(), c["text_lens"].cuda()
    log, soft = ops.align_attn(q, k, tl, c["B"])
    if name == "zero":
        assert float(log[0, 0, 5, 3]) == 0.0             # the copied row: a distance of exactly 0
    masked = ~(torch.arange(c["n"])[None] < c["text_lens"][:, None]).reshape(-1)
    for mode in R.attn_modes(name):
        g_log, g_soft = R.attn_grads(c, mode)
        args = (q, k, log, soft, None if g_log is None else g_log.cuda(), None if g_soft is None else g_soft.cuda(), tl)
        dq, dk = bk.align_attn_bwd(*args)
        dq2, dk2 = bk.align_attn_bwd(*args)
        assert torch.equal(dq, dq2) and torch.equal(dk, dk2), (name, mode)
        ref_dq, a_dq, ref_dk, a_dk = R.attn_bwd(c["q"], c["k"], log.cpu(), soft.cpu(), g_log, g_soft, c["text_lens"])
        assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dk).all())
        kq, iq = R.k_of(dq.cpu(), ref_dq, a_dq)
        kk, ik = R.k_of(dk.cpu(), ref_dk, a_dk)
        print(name, mode, "K dq", kq, "K dk", kk)
        assert kq <= R.k_gpu("attn_dq"), (name, mode, kq, iq)
        assert kk <= R.k_gpu("attn_dk"), (name, mode, kk, ik)
        assert bool((dk.cpu()[masked] == 0).all())
        if name == "base":                               # the fully masked utterance: no gradient at all
            assert bool((dq.cpu()[2 * c["T"]:] == 0).all())


# ---------------------------------------------------------------------------------------------- ns2_align_losses_fwd / _bwd
@pytest.fixture(scope="module")
def loss_refs():
    out = {}
    for name in R.LOSS_CASES:
        c = R.loss_inputs(name)
        out[name] = (c, R.ctc_torch(c["log"], c["text_lens"], c["mel_lens"]), R.bin_ref(c["log"], c["hard"], c["text_lens"]))
    return out


@pytest.mark.parametrize("name", sorted(R.LOSS_CASES))
def test_forward_sum_loss_and_gradient(bk, loss_refs, name):
    c, (l64, g64, gmax), _ = loss_refs[name]
    log, tl, ml = c["log"].cuda(), c["text_lens"].cuda(), c["mel_lens"].cuda()
    one = torch.ones(1, device="cuda")
    loss, _, ws = bk.align_losses_fwd(log, tl, ml, R.BLANK)
    d = bk.align_losses_bwd(log, tl, ml, R.BLANK, ws, g_fs=one)
    loss2, _, ws2 = bk.align_losses_fwd(log, tl, ml, R.BLANK)
    assert torch.equal(loss, loss2) and torch.equal(d, bk.align_losses_bwd(log, tl, ml, R.BLANK, ws2, g_fs=one))
    assert torch.equal(d, bk.align_losses_bwd(log, tl, ml, R.BLANK, ws, g_fs=one))        # the same workspace once more
    kl, kg = R.ctc_k(loss, d, l64, g64, gmax)
    print(name, "loss", float(loss), "ref", float(l64), "K loss", kl, "K grad", kg)
    assert kl <= R.k_gpu("ctc_loss") and kg <= R.k_gpu("ctc_grad"), (kl, kg)
    dc = d.cpu()
    for b in range(c["B"]):
        assert bool((dc[b, 0, int(c["mel_lens"][b]):] == 0).all()) and bool((dc[b, 0, :, int(c["text_lens"][b]):] == 0).all())
    if name == "small":
        assert bool((dc[2] == 0).all())                  # 20 frames for 32 labels: loss and gradient exactly 0
    half = bk.align_losses_bwd(log, tl, ml, R.BLANK, ws, g_fs=one * 0.5)
    assert torch.equal(half, d * 0.5)                    # the incoming gradient is a power of two here: exact


@pytest.mark.parametrize("name", sorted(R.LOSS_CASES))
def test_bin_loss_and_gradient(bk, loss_refs, name):
    c, _, (bl, al, bg, ag) = loss_refs[name]
    log, tl, hard = c["log"].cuda(), c["text_lens"].cuda(), c["hard"].cuda()
    one = torch.ones(1, device="cuda")
    _, loss, ws = bk.align_losses_fwd(log, tl, None, 0., hard=hard, want_fs=False, want_bin=True)
    d = bk.align_losses_bwd(log, tl, None, 0., ws, hard=hard, g_bin=one)
    _, loss2, ws2 = bk.align_losses_fwd(log, tl, None, 0., hard=hard, want_fs=False, want_bin=True)
    assert torch.equal(loss, loss2) and torch.equal(d, bk.align_losses_bwd(log, tl, None, 0., ws2, hard=hard, g_bin=one))
    kl = R.k_of(loss.reshape(1).cpu(), bl.reshape(1), al.reshape(1))[0]
    kg, ig = R.k_of(d.cpu(), bg, ag)
    print(name, "bin", float(loss), "ref", float(bl), "K loss", kl, "K grad", kg)
    assert kl <= R.k_gpu("bin_loss") and kg <= R.k_gpu("bin_grad"), (kl, kg, ig)
    dc = d.cpu()
    beyond = (torch.arange(c["n"])[None] > c["text_lens"][:, None])[:, None].expand(-1, c["T"], -1)
    assert bool((dc[:, 0][beyond] == 0).all())
    for b in range(c["B"]):
        assert bool((dc[b, 0, int(c["mel_lens"][b]):] == 0).all())       # the path is empty there
    # both losses in one call share the row statistics: the same bits as each alone
    fs, bn, ws = bk.align_losses_fwd(log, tl, c["mel_lens"].cuda(), R.BLANK, hard=hard, want_fs=True, want_bin=True)
    assert torch.equal(bn, loss) and torch.equal(fs, bk.align_losses_fwd(log, tl, c["mel_lens"].cuda(), R.BLANK)[0])


# ---------------------------------------------------------------------------------------------- module level
@pytest.mark.parametrize("name", ["c80", "c32"])
def test_aligner_hip_training_against_the_reference_gradients(name):
    from naturalspeech2_pytorch_amd.aligner import BinLoss, ForwardSumLoss
    fx, m, x, mel = golden_case(name)
    m = m.cuda()
    m.train_backend = "hip"
    tl, ml = fx["text_lens"].cuda(), fx["mel_lens"].cuda()
    n, T = x.shape[1], mel.shape[-1]
    x_mask = (torch.arange(n)[None] < fx["text_lens"][:, None])[:, None].cuda()
    y_mask = (torch.arange(T)[None] < fx["mel_lens"][:, None])[:, None].cuda()
    got = run_losses(m, lambda x, mel: m(x, x_mask, mel, y_mask), x.cuda(), mel.cuda(), tl, ml, ForwardSumLoss(backend="hip"), BinLoss(backend="hip"))
    assert torch.equal(got[4].cpu(), rows_to_path(fx["rows"], n))
    errs = {"fs_loss": abs(float(got[0]) - fx["fs_loss"]) / abs(fx["fs_loss"]), "bin_loss": abs(float(got[1]) - fx["bin_loss"]) / abs(fx["bin_loss"]),
            "dx": rel(got[3], fx["dx"])}
    assert sorted(got[2]) == sorted(fx["grads"]) and len(got[2]) == 10
    for k, g in fx["grads"].items():
        errs[k] = rel(got[2][k], g)
    worst = max(errs.items(), key=lambda z: z[1])
    print(name, "worst:", worst)
    record(f"aligner_training/{name}/worst_rel", {"key": worst[0], "rel": worst[1]})
    for k, e in errs.items():
        assert e < 1e-3, (name, k, e)
    # the public switch takes the pass (and only under autograd): patched away, the same call fails
    from naturalspeech2_pytorch_amd import training
    real = training.aligner_forward_train
    try:
        training.aligner_forward_train = None
        with pytest.raises(TypeError):
            m(x.cuda().requires_grad_(True), x_mask, mel.cuda(), y_mask)
        with torch.no_grad():
            m(x.cuda(), x_mask, mel.cuda(), y_mask)
    finally:
        training.aligner_forward_train = real


def test_wrapper_with_the_hip_aligner_against_the_fixture_and_the_composite():
    fx = _load("aligner_forward_d64.pt")
    inp = forward_inputs(fx)
    out = {}
    for backend in ("composite", "hip"):
        d = build_wrapper(fx, aligner_bin_loss_weight=1., aligner_train_backend=backend).cuda()
        seen = {}
        real = d.aligner.forward_lengths_train
        d.aligner.forward_lengths_train = lambda *a, seen=seen, real=real: (seen.__setitem__("train", True), real(*a))[1]
        loss, aux = run_forward(d, fx, inp, dev="cuda", return_aux_losses=True)
        (loss + aux["aux"]).backward()
        assert ("train" in seen) == (backend == "hip")
        grads = {k: p.grad.detach().clone() for k, p in d.named_parameters() if k.startswith("aligner.")}
        out[backend] = (float(loss), {k: float(v) for k, v in aux.items()}, grads, d)
    loss, aux, grads, d = out["hip"]
    assert abs(loss - fx["loss"]) <= 1e-3 * abs(fx["loss"])
    assert abs(aux["bin"] - fx["aux"]["bin"]) <= 1e-3 * abs(fx["aux"]["bin"])
    assert abs(aux["align"] - (fx["aux"]["align"] + fx["aux"]["bin"])) <= 1e-3 * abs(fx["aux"]["align"] + fx["aux"]["bin"])
    assert len(grads) == 10
    worst = ("", 0.0)
    for k, g in grads.items():
        ref = out["composite"][2][k]
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        e = rel(g, ref)
        worst = max(worst, (k, e), key=lambda z: z[1])
        assert e < 1e-3, (k, e)
    print("worst aligner gradient against the composite:", worst)
    record("aligner_training/wrapper/worst_rel_vs_composite", {"key": worst[0], "rel": worst[1]})
    # the hard path: bit-equal to the default route's (no_grad, forward_lengths)
    d0 = out["composite"][3]
    t = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        enc = d0.phoneme_enc(t["text"])
        default_path = d0.aligner.forward_lengths(enc, fx["text_lens"].cuda(), t["mel"], fx["mel_lens"].cuda())[3]
        enc_h = d.phoneme_enc(t["text"])
    hip_path = d.aligner.forward_lengths_train(enc_h.requires_grad_(True), fx["text_lens"].cuda(), t["mel"], fx["mel_lens"].cuda())[3]
    assert torch.equal(hip_path, default_path) and torch.equal(hip_path.cpu(), rows_to_path(fx["rows"], hip_path.shape[1]))
