"""Training at head dims 32 and 128 on the MI355X (include/ns2hip_train.h).

  1. kernel level: the training forward (o, lse), the delta reduction and the flash backward at D = 32 / 128 against an fp64 attention on the
     values the planes hold -- partial tiles, more than two walked tiles, a context below one tile, 640-feature rows --, the column
     offset, one half alone, the plane outputs in both formats;
  2. ragged batches: rows before a length are the utterance alone bit for bit, rows from it on zero bits, NaN behind the lengths
     reaches nothing;
  3. key mask and dropout against fp64 attention with the keep mask of ns2_dropout_keep_mask;
  4. model level: the committed reference-autograd goldens at dim_head 32 and 128 through `head_dim_training=True`, exact and mixed; the
     backend's attention calls are counted, and the same model without the switch still takes the composite;
  5. the conditioning Transformer and the DurationPitchPredictor at dim_head 32 against their own composite, mask and dropout included;
  6. one GraphedTrainStep of the dim_head 32 model: bit-identical to the eager pass.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, autograd_path, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd.transformer import Transformer  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402
from tests.parity_record import record  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
HB = training.HipBackend()
HEAD_DIMS = [32, 128]
# the project's bars at head dim 64 (tests/test_backward_gpu.py test_attention_forward_lse_and_backward)
O_TOL, LSE_TOL, DELTA_TOL, GRAD_TOL = 2e-5, 1e-4, 1e-5, 5e-5


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()


def join(p):
    return ops.join(p).cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rows(p, r0, n):
    return ops.Planes(p.buf[r0:r0 + n], n, p.ld, p.has_lo, p.fmt)


def _operands(B, H, Nq, Nk, D, cross):
    a = H * D
    q, k, v = (make_input(n, (B * L, a), seed=s) for n, s, L in (("aq", 17, Nq), ("ak", 18, Nk), ("av", 19, Nk)))
    do = make_input("ado", (B * Nq, a), seed=20)
    if cross:
        qp, kvp = HB.split(q.to(DEV)), HB.split(torch.cat((k, v), -1).to(DEV))
        return qp, kvp, kvp, 0, 0, a, do
    qkv = HB.split(torch.cat((q, k, v), -1).to(DEV))
    return qkv, qkv, qkv, 0, a, 2 * a, do


def _ref64(qr, kr, vr, dor, B, H, Nq, Nk, D, kmask=None, keep=None, keep_scale=1.0):
    """fp64 attention on the values the planes hold -> (o, lse in log2, delta, dq, dk, dv) by torch autograd"""
    a = H * D
    tq, tk, tv = (t.double().clone().requires_grad_(True) for t in (qr, kr, vr))
    hd = lambda t, n: t.reshape(B, n, H, D).transpose(1, 2)          # noqa: E731
    s = hd(tq, Nq) @ hd(tk, Nk).transpose(2, 3) * D ** -0.5
    if kmask is not None:
        s = s.masked_fill(~kmask[:, None, None, :], float("-inf"))
    P = s.softmax(-1)
    if keep is not None:
        P = P * keep.double() * keep_scale
    out = (P @ hd(tv, Nk)).transpose(1, 2).reshape(B * Nq, a)
    (out * dor.double()).sum().backward()
    lse = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    delta = (dor.double() * out.detach()).reshape(B, Nq, H, D).sum(-1).transpose(1, 2)
    return out.detach(), lse, delta, tq.grad, tk.grad, tv.grad


# ------------------------------------------------------------------------------------------------ 1. the kernels against fp64
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("B,H,Nq,Nk,cross", [(2, 3, 200, 200, False), (3, 2, 160, 40, True), (1, 5, 96, 96, False)])
def test_attention_forward_lse_and_backward_at_head_dims_32_and_128(B, H, Nq, Nk, cross, D):
    a = H * D
    qp, kp, vp, qc, kc, vc, do = _operands(B, H, Nq, Nk, D, cross)
    qr, kr, vr = join(qp)[:, qc:qc + a], join(kp)[:, kc:kc + a], join(vp)[:, vc:vc + a]      # what the planes hold
    vt = HB.transpose(vp, vc, a, Nk, per_batch=True)
    o, lse = HB.attention(qp, qc, kp, kc, vt, B, H, Nq, Nk, head_dim=D)
    delta = HB.attention_delta(do.to(DEV), o, B, H, Nq, head_dim=D)
    do_row, _, _ = HB.grad_prep(do.to(DEV), a, want_row=True)
    dq = torch.full((B * Nq, a + 32), NAN, device=DEV)
    dkv = torch.full((B * Nk, 2 * a), NAN, device=DEV)
    HB.attention_bwd(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, dq=(dq, 32), dkv=(dkv, 0, a), head_dim=D)
    ro, rlse, _, rdq, rdk, rdv = _ref64(qr, kr, vr, join(do_row), B, H, Nq, Nk, D)
    rdelta = (do.double() * join(o).double()).reshape(B, Nq, H, D).sum(-1).transpose(1, 2)      # of the o the kernel wrote, as the kernel reads it
    e = dict(o=rel(join(o), ro), lse=(lse.cpu().double() - rlse).abs().max().item(), delta=rel(delta, rdelta),
             dq=rel(dq[:, 32:], rdq), dk=rel(dkv[:, :a], rdk), dv=rel(dkv[:, a:], rdv))
    print(e)
    record(f"head_dim_training/kernels_d{D}_b{B}_h{H}_q{Nq}_k{Nk}", e)
    assert e["o"] < O_TOL and e["lse"] < LSE_TOL and e["delta"] < DELTA_TOL, e
    assert max(e["dq"], e["dk"], e["dv"]) < GRAD_TOL, e
    assert torch.isnan(dq[:, :32]).all()                # the column offset is honoured
    # one half only, and two launches give the same bits (no atomics, fixed order)
    dq2 = torch.empty(B * Nq, a, device=DEV)
    HB.attention_bwd(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, dq=(dq2, 0), head_dim=D)
    assert torch.equal(dq2, dq[:, 32:])
    dkv2 = torch.full((B * Nk, 2 * a), NAN, device=DEV)
    HB.attention_bwd(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, dkv=(dkv2, 0, a), head_dim=D)
    assert torch.equal(dkv2, dkv)
    if not cross:                                       # the plane output = the conversion of the fp32 output, in both formats
        for prec in (3, 4):
            bk = training.HipBackend(prec)
            gp = bk.new_planes(B * Nq, 3 * a)
            bk.attention_bwd(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, planes=(gp, 0, a, 2 * a), head_dim=D)
            want = bk.split(torch.cat((dq[:, 32:], dkv), -1))
            assert torch.equal(_bits(gp.buf), _bits(want.buf)), prec


def test_head_dim_64_through_the_new_entries_is_the_existing_kernels_bit_for_bit():
    B, H, N, D = 2, 2, 200, 64
    a = H * D
    qp, kp, vp, qc, kc, vc, do = _operands(B, H, N, N, D, False)
    vt = HB.transpose(vp, vc, a, N, per_batch=True)
    o, lse = HB.attention(qp, qc, kp, kc, vt, B, H, N, N)
    o2 = ops._out_planes(B * N, a, DEV, 3)
    lse2 = torch.empty_like(lse)
    from naturalspeech2_pytorch_amd import _lib
    import ctypes
    blk = _lib.AttnArgs(q_hi=qp.hi, q_lo=qp.lo, ldq=qp.ld, q_col0=qc, k_hi=kp.hi, k_lo=kp.lo, ldk=kp.ld, k_col0=kc, vt_hi=vt.ptr(), vt_lo=vt.ptr() + 64,
                        vt_ld=vt.ld, o_hi=o2.hi, o_lo=o2.lo, ldo=o2.ld, B=B, H=H, Nq=N, Nk=N, scale=0.125, head_dim=64, precision=3, lse=lse2.data_ptr())
    _lib.check(HB.lib.ns2_attention_train_fwd_hd(ctypes.byref(blk), None, ops._stream()), "ns2_attention_train_fwd_hd")
    assert torch.equal(_bits(o2.buf), _bits(o.buf)) and torch.equal(lse2, lse)
    do = do.to(DEV)
    delta = HB.attention_delta(do, o, B, H, N)
    delta2 = torch.empty_like(delta)
    _lib.check(HB.lib.ns2_attention_delta_hd(do.data_ptr(), a, o.hi, o.lo, o.ld, B, H, N, 64, delta2.data_ptr(), 3, ops._stream()), "delta_hd")
    assert torch.equal(delta2, delta)


# ------------------------------------------------------------------------------------------------ 2. ragged batches, bit for bit
RB, RH, RN, RLENS = 3, 2, 200, [200, 129, 1]              # the second own tile (rows 128 ..): one row inside the length 129, wholly beyond the length 1


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_ragged_training_attention_at_head_dims_32_and_128(D):
    a = RH * D
    g = torch.Generator().manual_seed(90 + D)
    q, k, v, do = (torch.randn(RB * RN, a, generator=g).to(DEV) for _ in range(4))
    qp, kp, vp, dop = (ops.split(t, precision=3) for t in (q, k, v, do))
    vt = HB.transpose(vp, 0, a, RN, per_batch=True)
    for p in (qp, kp, vp, dop):                             # NaN behind the lengths, in every plane
        for b, n in enumerate(RLENS):
            p.buf.view(RB, RN, -1)[b, n:] = NAN
    for b, n in enumerate(RLENS):                           # ... and in the V^T columns: interleaved lines [hi(32) | lo(32)] per 32 token columns
        cols = (torch.arange(vt.ld, device=DEV) >= n).view(vt.ld // 32, 1, 32).expand(vt.ld // 32, 2, 32)
        vt.buf.view(RB, a, vt.ld // 32, 2, 32)[b][:, cols] = NAN
    kl = torch.tensor(RLENS, dtype=torch.int32, device=DEV)

    def fwd(qq, kk, vt_row, B, N, o_prec, lens=None):
        return ops._attention_fwd(qq, 0, kk, 0, vt.ptr(vt_row), vt.ptr(vt_row) + 64, vt.ld, B, RH, N, N, D ** -0.5, 3, head_dim=D, o_precision=o_prec,
                                  want_lse=True, train_lens=lens)

    lse3 = None
    for o_prec in (3, 4):
        o, lse = fwd(qp, kp, 0, RB, RN, o_prec, lens=kl)
        lse3 = lse if o_prec == 3 else lse3
        for b, n in enumerate(RLENS):
            so, sl = fwd(_rows(qp, b * RN, n), _rows(kp, b * RN, n), b * a, 1, n, o_prec)      # the utterance alone at its own length
            assert torch.equal(_bits(o.buf[b * RN:b * RN + n]), _bits(so.buf)), (o_prec, b)
            assert torch.equal(lse[b, :, :n].contiguous().view(torch.int32), sl[0].contiguous().view(torch.int32)), (o_prec, b)
            assert torch.count_nonzero(_bits(o.buf[b * RN + n:(b + 1) * RN])) == 0 and bool((lse[b, :, n:] == float("inf")).all()), (o_prec, b)
    lse = lse3.clone()
    delta = (0.1 * torch.randn(RB, RH, RN, generator=g)).to(DEV)
    for b, n in enumerate(RLENS):
        lse[b, :, n:] = NAN
        delta[b, :, n:] = NAN
    for out in ("f32", "planes3", "planes4"):
        bk = training.HipBackend(4 if out == "planes4" else 3)

        def run(qq, kk, vv, dd, ls, dl, B, N, lens):
            kw = {} if lens is None else dict(lens=lens)
            if out == "f32":
                dq, dkv = torch.full((B * N, a), NAN, device=DEV), torch.full((B * N, 2 * a), NAN, device=DEV)
                bk.attention_bwd(qq, 0, kk, 0, vv, 0, dd, ls, dl, B, RH, N, N, dq=(dq, 0), dkv=(dkv, 0, a), head_dim=D, **kw)
                return torch.cat((dq, dkv), dim=1).view(torch.int32)
            gp = bk.new_planes(B * N, 3 * a)
            gp.buf.fill_(NAN)
            bk.attention_bwd(qq, 0, kk, 0, vv, 0, dd, ls, dl, B, RH, N, N, planes=(gp, 0, a, 2 * a), head_dim=D, **kw)
            return _bits(gp.buf)

        got = run(qp, kp, vp, dop, lse, delta, RB, RN, kl)
        for b, n in enumerate(RLENS):
            r0 = b * RN
            solo = run(_rows(qp, r0, n), _rows(kp, r0, n), _rows(vp, r0, n), _rows(dop, r0, n), lse[b:b + 1, :, :n].contiguous(),
                       delta[b:b + 1, :, :n].contiguous(), 1, n, None)
            assert torch.equal(got[r0:r0 + n], solo), (out, b)
            assert torch.count_nonzero(got[r0 + n:r0 + RN]) == 0, (out, b)


# ------------------------------------------------------------------------------------------------ 3. key mask and dropout
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_masked_and_dropout_attention_at_head_dims_32_and_128(D):
    B, H, N, p = 2, 2, 150, 0.2
    a = H * D
    qp, kp, vp, qc, kc, vc, do = _operands(B, H, N, N, D, False)
    qr, kr, vr = join(qp)[:, qc:qc + a], join(kp)[:, kc:kc + a], join(vp)[:, vc:vc + a]
    kmask = torch.arange(N)[None] < torch.tensor([N, N // 2])[:, None]      # masked tails
    kmask[0, 3::7] = False                                                   # ... and scattered holes
    seed = torch.tensor([0x0123456789ABCDEF], dtype=torch.int64, device=DEV)
    drop, km_dev = (p, seed, 3), kmask.to(torch.uint8).to(DEV)
    vt = HB.transpose(vp, vc, a, N, per_batch=True)
    o, lse = HB.attention_masked(qp, qc, kp, kc, vt, B, H, N, N, kmask=km_dev, drop=drop, head_dim=D)
    delta = HB.attention_delta(do.to(DEV), o, B, H, N, head_dim=D)
    do_row, _, _ = HB.grad_prep(do.to(DEV), a, want_row=True)
    dq = torch.full((B * N, a), NAN, device=DEV)
    dkv = torch.full((B * N, 2 * a), NAN, device=DEV)
    HB.attention_bwd_masked(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, N, N, dq=(dq, 0), dkv=(dkv, 0, a), kmask=km_dev, drop=drop, head_dim=D)
    keep = HB.dropout_keep_mask(seed, 3, p, B, H, N, N).cpu()
    ro, rlse, _, rdq, rdk, rdv = _ref64(qr, kr, vr, join(do_row), B, H, N, N, D, kmask=kmask, keep=keep, keep_scale=1.0 / (1.0 - float(np.float32(p))))
    e = dict(o=rel(join(o), ro), lse=(lse.cpu().double() - rlse).abs().max().item(), dq=rel(dq, rdq), dk=rel(dkv[:, :a], rdk), dv=rel(dkv[:, a:], rdv))
    print(e)
    record(f"head_dim_training/mask_dropout_d{D}", e)
    assert e["o"] < O_TOL and e["lse"] < LSE_TOL, e       # the bars of tests/test_encoder_training_gpu.py for the same comparison at 64
    assert max(e["dq"], e["dk"], e["dv"]) < GRAD_TOL, e
    assert (dkv[(~kmask).reshape(-1).to(DEV)] == 0).all()  # masked keys: dK = dV = 0 exactly
    gp = HB.new_planes(B * N, 3 * a)
    HB.attention_bwd_masked(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, N, N, planes=(gp, 0, a, 2 * a), kmask=km_dev, drop=drop, head_dim=D)
    assert torch.equal(ops.join(gp), ops.join(HB.split(torch.cat((dq, dkv), -1))))


# ------------------------------------------------------------------------------------------------ 4. the model against the reference's autograd
OUT_TOL, PARAM_TOL = 1e-4, 1e-3                            # test_gradients_match_the_committed_reference_autograd_golden's bars
ATTN_CALLS = ("attention", "attention_masked", "attention_delta", "attention_bwd")


@pytest.fixture()
def counted(monkeypatch):
    """{HipBackend method: [the head_dim keyword of every call]}"""
    calls = {k: [] for k in ATTN_CALLS}
    for name in ATTN_CALLS:
        real = getattr(training.HipBackend, name)

        def f(self, *a, _real=real, _name=name, **k):
            calls[_name].append(k.get("head_dim"))
            return _real(self, *a, **k)
        monkeypatch.setattr(training.HipBackend, name, f)
    return calls


@pytest.fixture(scope="module")
def goldens():
    from tests.golden.make_golden_head_dim_grads import load_head_dim_grads
    return {name: load_head_dim_grads(name) for name in ("uncond_d64_hd32", "cond_d64_hd128")}      # read once, shared, left unchanged


def _golden_model(fix, tprec, **kw):
    m = Model(**fix["kwargs"], **kw)
    m.load_state_dict(make_weights(fix["shapes"], seed=fix["weight_seed"]))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    return m


def _golden_inputs(fix):
    kw = fix["kwargs"]
    b, n, d = fix["batch"], fix["n"], kw["dim"]
    x = make_input("x", (b, n, d), seed=fix["input_seed"]).to(DEV).requires_grad_(True)
    t = make_input("times", (b,), seed=fix["input_seed"], uniform=True).to(DEV)
    extra = {}
    if kw.get("condition_on_prompt"):
        extra = dict(prompt=make_input("prompt", (b, fix["n_prompt"], kw["dim_prompt"]), seed=fix["input_seed"]).to(DEV),
                     cond=make_input("cond", (b, kw["dim_prompt"], fix["n_cond"]), seed=fix["input_seed"]).to(DEV), cond_drop_prob=0.)
    return x, t, extra


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
@pytest.mark.parametrize("name", ["uncond_d64_hd32", "cond_d64_hd128"])
def test_gradients_match_the_reference_autograd_goldens_at_head_dims_32_and_128(goldens, counted, monkeypatch, name, tprec):
    fix = goldens[name]
    kw = fix["kwargs"]
    m = _golden_model(fix, tprec, head_dim_training=True)
    x, t, extra = _golden_inputs(fix)
    entered = []
    real = autograd_path.model_forward_autograd
    monkeypatch.setattr(autograd_path, "model_forward_autograd", lambda *a, **k: (entered.append(1), real(*a, **k))[1])
    y = m(x, t, **extra)                                   # Model.forward under autograd: the switch decides the path
    (y * make_input("gw", tuple(y.shape), seed=fix["loss_weight_seed"]).to(DEV)).sum().backward()
    assert not entered, "the composite was entered: the HIP training path did not run"
    n_attn = kw["depth"] * (2 if kw.get("condition_on_prompt") else 1) + (2 if kw.get("condition_on_prompt") else 0)      # + the resampler's two layers
    assert len(counted["attention"]) == n_attn and len(counted["attention_bwd"]) == n_attn and len(counted["attention_delta"]) == n_attn
    assert all(hd == kw["dim_head"] for v in counted.values() for hd in v)
    errs = {}
    for k, p in m.named_parameters():
        r = fix["grads"][k]
        assert p.grad is not None and p.grad.shape == r.shape, k
        if r.abs().max() == 0:
            assert p.grad.abs().max().item() == 0, k
        else:
            errs[k] = rel(p.grad, r)
    worst = max(errs, key=errs.get)
    res = dict(out_rel=rel(y.detach(), fix["output"]), x_grad_rel=rel(x.grad, fix["x_grad"]), n_tensors=len(errs), worst_param=worst,
               worst_rel=errs[worst], median_rel=sorted(errs.values())[len(errs) // 2])
    print(name, tprec, res)
    record(f"head_dim_training/golden_{name}_{tprec}", res)
    assert res["out_rel"] < OUT_TOL and res["x_grad_rel"] < PARAM_TOL and res["worst_rel"] < PARAM_TOL, res


def test_without_the_switch_the_same_model_still_takes_the_composite(goldens, counted, monkeypatch):
    fix = goldens["uncond_d64_hd32"]
    m = _golden_model(fix, "exact")
    assert m.head_dim_training is False
    x, t, extra = _golden_inputs(fix)
    entered = []
    real = autograd_path.model_forward_autograd
    monkeypatch.setattr(autograd_path, "model_forward_autograd", lambda *a, **k: (entered.append(1), real(*a, **k))[1])
    with pytest.warns(UserWarning, match="dim_head"):
        y = m(x, t, **extra)
    y.sum().backward()
    assert entered and not any(counted.values())
    assert rel(y.detach(), fix["output"]) < OUT_TOL


def test_ragged_batch_trains_at_head_dim_32(goldens):
    """Model(..., ragged_training=True, head_dim_training=True): NaN behind the lengths reaches nothing, rows from a length on are zero"""
    fix = goldens["uncond_d64_hd32"]
    m = _golden_model(fix, "exact", ragged_training=True, head_dim_training=True)
    x, t, _ = _golden_inputs(fix)
    lens = torch.tensor([fix["n"], 37], dtype=torch.int32, device=DEV)
    cot = make_input("gw", (fix["batch"], fix["n"], 64), seed=3).to(DEV)

    def run(xx):
        for p in m.parameters():
            p.grad = None
        y = m(xx, t, lens=lens)
        (y * cot).sum().backward()
        return y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    y0, g0 = run(x.detach())
    xn = x.detach().clone()
    xn[1, 37:] = NAN
    y1, g1 = run(xn)
    assert torch.isfinite(y1).all() and torch.equal(y1, y0) and torch.count_nonzero(y1[1, 37:]) == 0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    solo = m(x.detach()[1:2, :37], t[1:2]).detach()         # the utterance alone at its own length
    assert rel(y0[1:2, :37], solo) < 1e-5


# ------------------------------------------------------------------------------------------------ 5. encoders and predictor against their composite
def _run(m, fwd, args, kw, leaves, projs):
    for p in m.parameters():
        p.grad = None
    for l in leaves:
        l.grad = None
    outs = fwd(m, *args, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * pr).sum() for o, pr in zip(outs, projs)).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads.update({f"input{i}": l.grad.detach().clone() for i, l in enumerate(leaves)})
    return [o.detach() for o in outs], grads


def _compare(tag, outs, grads, outs0, grads0):
    errs = {k: rel(grads[k], g) for k, g in grads0.items()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    res = dict(out_rel=max(rel(o, o0) for o, o0 in zip(outs, outs0)), n_tensors=len(errs), worst_tensor=worst[0], worst_rel=worst[1])
    print(tag, res)
    record(f"head_dim_training/{tag}", res)
    # output 1e-4, every gradient tensor 1e-3: the bars of tests/test_encoder_training_gpu.py and tests/test_duration_pitch_training_gpu.py at 64
    assert res["out_rel"] < 1e-4 and res["worst_rel"] < 1e-3, (tag, res)


def _call(m, *a, **k):
    return m(*a, **k)


@pytest.fixture()
def no_composite(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the PyTorch composite was entered: the HIP training path did not run")
    saved = {n: getattr(autograd_path, n) for n in ("transformer_forward_autograd", "duration_pitch_autograd")}
    for n in saved:
        monkeypatch.setattr(autograd_path, n, refuse)
    return saved


def _explicit_keep_transformer(tr, x, mask, seed, p):
    """the fp32 composite with softmax(S) * keep / (1 - p) @ V at the module's own head dim, keep from the kernels' debug entry"""
    b, n, _ = x.shape
    D, h = tr.dim_head, x
    for li, (n1, attn, n2, ff) in enumerate(tr.layers):
        xn = autograd_path._rmsnorm(h, n1)
        q = attn.to_q(xn)
        k, v = attn.to_kv(xn).chunk(2, dim=-1)
        sp = lambda t: t.reshape(b, n, tr.heads, D).transpose(1, 2)          # noqa: E731
        s = (sp(q) @ sp(k).transpose(2, 3)) * D ** -0.5
        s = s.masked_fill(~mask[:, None, None, :], -torch.finfo(s.dtype).max)
        keep = HB.dropout_keep_mask(seed, li, p, b, tr.heads, n, n).float() / (1.0 - float(np.float32(p)))
        o = ((s.softmax(-1) * keep) @ sp(v)).transpose(1, 2).reshape(b, n, -1)
        h = attn.to_out(o) + h
        h = autograd_path._feedforward(autograd_path._rmsnorm(h, n2), ff, False) + h
    return autograd_path._rmsnorm(h, tr.norm) if hasattr(tr.norm, "gamma") else h


@pytest.mark.parametrize("variant", ["plain", "mask_dropout"])
def test_transformer_at_head_dim_32_against_its_composite(no_composite, counted, variant):
    p = 0.2 if variant == "mask_dropout" else 0.
    torch.manual_seed(301)                                 # PyTorch's default initialisation under a fixed seed
    tr = Transformer(dim=64, depth=1, dim_head=32, heads=2, dropout=p, final_norm=True, train_backend="hip", head_dim_training=True).to(DEV).train()
    b, n = 3, 150
    x = make_input("x", (b, n, 64), seed=302).to(DEV).requires_grad_(True)
    proj = make_input("proj", (b, n, 64), seed=303).to(DEV)
    if variant == "plain":
        outs, grads = _run(tr, _call, (x,), {}, [x], [proj])
        assert counted["attention"] == [32] and counted["attention_bwd"] == [32]
        outs0, grads0 = _run(tr, no_composite["transformer_forward_autograd"], (x,), {}, [x], [proj])
    else:
        mask = (torch.arange(n)[None] < torch.tensor([150, 77, 9])[:, None]).to(DEV)
        tr.dropout_seed = torch.tensor([0x5EED5EED5EED], dtype=torch.int64, device=DEV)
        outs, grads = _run(tr, _call, (x,), dict(mask=mask), [x], [proj])
        assert counted["attention_masked"] == [32] and counted["attention_bwd"] == [32]
        ref = lambda m, xx, mask: _explicit_keep_transformer(m, xx, mask, tr.dropout_seed, p)      # noqa: E731
        outs0, grads0 = _run(tr, ref, (x,), dict(mask=mask), [x], [proj])
    _compare(f"transformer_hd32_{variant}", outs, grads, outs0, grads0)


def test_duration_pitch_predictor_at_head_dim_32_against_its_composite(no_composite, counted):
    torch.manual_seed(311)
    m = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=2, dim_head=32, dropout=0., train_backend="hip",
                               head_dim_training=True).to(DEV).train()
    b, n, n_p = 2, 70, 33
    x = make_input("phoneme_enc", (b, n, 64), seed=312).to(DEV).requires_grad_(True)
    prompts = make_input("prompt_enc", (b, n_p, 64), seed=313).to(DEV).requires_grad_(True)
    projs = [make_input(f"proj{i}", (b, n), seed=314).to(DEV) for i in range(2)]
    outs, grads = _run(m, _call, (x, prompts), {}, [x, prompts], projs)
    assert counted["attention_masked"] + counted["attention"] == [32, 32] and counted["attention_bwd"] == [32, 32]      # one layer per trunk
    outs0, grads0 = _run(m, no_composite["duration_pitch_autograd"], (x, prompts), {}, [x, prompts], projs)
    assert all(0.1 <= float((o > 0).float().mean()) <= 0.9 for o in outs0)      # the ReLU of each head both passes and blocks gradient
    _compare("duration_pitch_hd32", outs, grads, outs0, grads0)


# ------------------------------------------------------------------------------------------------ 6. capture
def test_graphed_train_step_at_head_dim_32_is_the_eager_pass_bit_for_bit(goldens):
    fix = goldens["uncond_d64_hd32"]
    m = _golden_model(fix, "exact", head_dim_training=True)
    x, t, _ = _golden_inputs(fix)
    x = x.detach()
    w = make_input("gw", tuple(x.shape), seed=fix["loss_weight_seed"]).to(DEV)

    def loss_fn(xx, tt, ww):
        return (m(xx, tt) * ww).mean()

    step = training.GraphedTrainStep(loss_fn, (x, t, w), m)
    for q in m.parameters():
        q.grad = None
    l_e = loss_fn(x, t, w)
    l_e.backward()
    l_e, g_e = l_e.detach().clone(), {k: q.grad.detach().clone() for k, q in m.named_parameters()}
    for q in m.parameters():
        q.grad = None
    l_g = step(x, t, w).detach().clone()
    assert torch.equal(l_g, l_e)
    for k, q in m.named_parameters():
        assert q.grad is not None and torch.equal(q.grad, g_e[k]), k
