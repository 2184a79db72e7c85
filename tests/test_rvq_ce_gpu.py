"""The fused RVQ cross-entropy kernel (csrc/rvq_ce.hip, ns2_rvq_ce) on the MI355X: row losses, loss and unit gradient against the fp64
reference of tests/rvq_ce_ref64.py under the bounds pinned there, quantized_out bit for bit, bit-equal repeats, the defined edge
behaviour, and `codec.rq` with `backend="hip"` inside `NaturalSpeech2` against the composite on the same GPU -- eager and captured."""
import pytest
import torch

from tests import rvq_ce_ref64 as R
from tests.golden.gen import make_input, make_weights

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

DEV = torch.device("cuda")


def run(x, cb, idx, need_grad=True, need_quantized=True):
    """-> (loss, row_loss [M, Q], quantized_out, G) of ops.rvq_cross_entropy on the rows of x [b, n, 128], on the CPU"""
    from naturalspeech2_pytorch_amd import ops
    M = idx[..., 0].numel()
    cbd = cb.to(DEV).contiguous()
    out = ops.rvq_cross_entropy(x.reshape(M, -1).to(DEV).contiguous(), cbd, ops.rvq_prepare(cbd), idx.reshape(M, -1).to(DEV).contiguous(),
                                need_grad, need_quantized=need_quantized)
    return tuple(None if t is None else t.cpu() for t in out)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_kernel_against_fp64(name):
    """row losses, loss and G inside (*) with the kernel's K; quantized_out EQUAL to the reference's on the compared rows: the kernel
    guarantees the same fp32 adds in stage order (0 + e_0 + e_1 + ...: ns2_rvq_decode's sum over the nearest codes), so bit-equal, not
    merely within an ulp per stage; two runs bit-identical; the loss does not depend on need_grad"""
    x, cb, idx, ref = R.case(name)
    M = idx[..., 0].numel()
    pairs, rows_G, rows_q = R.compared(ref)
    loss, rows, quant, G = run(x, cb, idx)
    k = {"row_loss": R.k_of(rows, ref["row_loss"], ref["A_row"], pairs),
         "loss": R.k_of(loss, R.mixed_loss(ref, rows), ref["A_loss"]),
         "G": R.k_of(G, ref["G"], ref["A_G"], rows_G[:, None].expand(M, R.D))}
    print(f"case {name}: K of the kernel: " + ", ".join(f"{n} {v:.2f} (allowed {R.k_gpu(n)})" for n, v in k.items()))
    assert torch.isfinite(rows).all() and torch.isfinite(G).all()
    for n, v in k.items():
        assert v <= R.k_gpu(n), (n, v)
    assert torch.equal(quant[rows_q], ref["quantized"][rows_q])

    loss2, rows2, quant2, G2 = run(x, cb, idx)
    assert torch.equal(loss, loss2) and torch.equal(rows, rows2) and torch.equal(G, G2) and torch.equal(quant, quant2)
    loss3, rows3, quant3, G3 = run(x, cb, idx, need_grad=False, need_quantized=False)
    assert G3 is None and quant3 is None
    assert torch.equal(loss, loss3) and torch.equal(rows, rows3)


def test_residual_equal_to_a_code():
    """rows that ARE a code of stage 0 (distance 0 to their target, then a zero residual in stage 1): finite losses inside (*) -- whose A
    is inf exactly where the expanded distance has no first order, i.e. at the zero distance itself -- and a finite gradient"""
    x, cb, idx, _ = R.case("a")
    M = idx[..., 0].numel()
    x, idx = x.reshape(M, -1).clone(), idx.reshape(M, -1).clone()
    hit = torch.tensor([0, 5, 40, 73])
    codes = torch.tensor([3, 64, 127, 0])
    x[hit] = cb[0][codes]
    idx[hit, 0] = codes
    ref = R.reference(x, cb, idx)
    assert (ref["nearest"][hit, 0] == codes).all() and torch.isinf(ref["A_row"][hit, 0]).all()
    pairs, rows_G, _ = R.compared(ref)
    loss, rows, quant, G = run(x, cb, idx)
    assert torch.isfinite(loss) and torch.isfinite(rows).all() and torch.isfinite(G).all()
    assert R.k_of(rows, ref["row_loss"], ref["A_row"], pairs) <= R.k_gpu("row_loss")
    # the rows that do not sit on a code keep the gradient bound (their A is finite)
    keep = rows_G.clone()
    keep[hit] = False
    assert R.k_of(G, ref["G"], ref["A_G"], keep[:, None].expand(M, R.D)) <= R.k_gpu("G")
    # on the code itself the loss of stage 0 is log sum_c exp(-dist_c) + 0 with one term exp(-0): the kernel's lse sees the distance
    # sqrt(rounding of |r|^2 - 2 r.e + |e|^2) instead of 0, and d lse / d dist <= 1.  With the cap K = 64 on the rounding of the expanded
    # d^2, whose terms add up to T = 4 |e|^2 at r = e, that is at most sqrt(64 * 2^-24 * T)
    T = 4 * cb[0][codes].double().pow(2).sum(-1)
    assert ((rows[hit, 0].double() - ref["row_loss"][hit, 0]).abs() <= (R.K_CAP * R.EPS * T).sqrt()).all()


@pytest.mark.parametrize("bad", [-1, "C"])
def test_target_outside_the_codebook_is_nan_without_a_sync(bad):
    from naturalspeech2_pytorch_amd import ops
    x, cb, idx, ref = R.case("a")
    M, C = idx[..., 0].numel(), cb.shape[1]
    idx = idx.reshape(M, -1).clone()
    idx[7, 1] = C if bad == "C" else bad
    xd, cbd, idxd = x.reshape(M, -1).to(DEV).contiguous(), cb.to(DEV).contiguous(), idx.to(DEV)
    norm = ops.rvq_prepare(cbd)
    ops.rvq_cross_entropy(xd, cbd, norm, idxd, True)                      # warm: function attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, rows, quant, G = ops.rvq_cross_entropy(xd, cbd, norm, idxd, True)      # no exception, no host read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows, G = rows.cpu(), G.cpu()
    assert torch.isnan(loss).item() and torch.isnan(rows[7, 1]).item() and torch.isnan(G[7]).all()
    ok = torch.ones(M, dtype=torch.bool)
    ok[7] = False
    assert torch.isfinite(rows[ok]).all() and torch.isfinite(G[ok]).all() and torch.isfinite(rows[7, 0])
    assert torch.equal(quant.cpu(), run(x, cb, R.case("a")[2])[2])        # the nearest codes do not depend on the targets


def test_argument_errors_and_reasons():
    from naturalspeech2_pytorch_amd import _lib, training
    from naturalspeech2_pytorch_amd.codec import HipRVQ, ResidualVQCrossEntropy
    lib = _lib.load()
    assert lib.ns2_version() >= 123
    z = torch.zeros(64 * 128, device=DEV)
    i = torch.zeros(64, dtype=torch.int64, device=DEV)
    for D, C in ((64, 64), (128, 96)):
        rc = lib.ns2_rvq_ce(z.data_ptr(), z.data_ptr(), z.data_ptr(), i.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, 4, 1, C, D, None, 0, None)
        assert rc == -1, (D, C, rc)
    x, cb, idx, _ = R.case("a")
    rq = ResidualVQCrossEntropy(HipRVQ(cb).to(DEV), backend="hip")
    xd, idxd = x.to(DEV), idx.to(DEV)
    assert training.rvq_ce_unsupported_reason(rq, xd, idxd) is None
    assert "float64" in training.rvq_ce_unsupported_reason(rq, xd.double(), idxd)
    assert "int32" in training.rvq_ce_unsupported_reason(rq, xd, idxd.int())
    assert "CPU" in training.rvq_ce_unsupported_reason(rq, x, idx)


def _wrapper(backend, tprec="exact"):
    from naturalspeech2_pytorch_amd import NaturalSpeech2
    from naturalspeech2_pytorch_amd.codec import EncodecWrapperHIP
    from naturalspeech2_pytorch_amd.model import Model
    _, cb, _, _ = R.case("a")
    m = Model(dim=128, depth=1)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=81))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    d = NaturalSpeech2(m, codec=EncodecWrapperHIP(cb), rvq_cross_entropy_loss_weight=0.1, rvq_ce_backend=backend).to(DEV)
    assert d.codec.rq.backend == backend
    return m, d


def _batch():
    _, cb, _, _ = R.case("a")
    b, n = 2, 64
    from naturalspeech2_pytorch_amd.codec import HipRVQ
    audio = make_input("rvq_ce:e2e:audio", (b, n, 128), seed=82)
    codes, _ = HipRVQ(cb).to(DEV).encode(audio.to(DEV))                   # the codec's own codes of the latents
    times = make_input("rvq_ce:e2e:times", (b,), seed=82, uniform=True)
    noise = make_input("rvq_ce:e2e:noise", (b, n, 128), seed=83)
    return tuple(t.to(DEV) for t in (audio, codes, times, noise))


def _eager(m, d, ins):
    for p in m.parameters():
        p.grad = None
    a, c, t, z = ins
    loss = d(a, codes=c, times=t, noise=z)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_end_to_end_against_the_composite():
    """NaturalSpeech2 with the term switched on: loss and every parameter gradient with rvq_ce_backend="hip" within 1e-3 relative (the
    project's gradient tolerance) of the composite backend on the same GPU"""
    ins = _batch()
    m_c, d_c = _wrapper("composite")
    m_h, d_h = _wrapper("hip")
    l_c, g_c = _eager(m_c, d_c, ins)
    l_h, g_h = _eager(m_h, d_h, ins)
    assert torch.isfinite(l_h) and abs(float(l_h) - float(l_c)) <= 1e-3 * abs(float(l_c)), (float(l_h), float(l_c))
    assert g_c.keys() == g_h.keys() and len(g_h) > 0
    worst = 0.0
    for k in g_c:
        a, b = g_h[k].double(), g_c[k].double()
        r = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        worst = max(worst, r)
        assert r <= 1e-3, (k, r)
    print(f"loss hip {float(l_h):.7f} composite {float(l_c):.7f}; worst relative gradient difference {worst:.2e}")


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
def test_graphed_step_replays_the_eager_hip_pass(tprec):
    """GraphedTrainStep over the loss with the HIP backend captures (the composite's host read of the indices cannot) and replays with the
    loss and every gradient bit-identical to the eager HIP pass, under either arithmetic of the denoiser (the term itself is fp32)"""
    from naturalspeech2_pytorch_amd import training
    ins = _batch()
    m, d = _wrapper("hip", tprec)
    l_e, g_e = _eager(m, d, ins)
    step = training.GraphedTrainStep(lambda a, c, t, z: d(a, codes=c, times=t, noise=z), ins, m)
    for p in m.parameters():
        p.grad = None
    l_g = step(*ins)
    torch.cuda.synchronize()
    assert torch.equal(l_g, l_e)
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert got.keys() == g_e.keys()
    for k in g_e:
        assert torch.equal(got[k], g_e[k]), k
