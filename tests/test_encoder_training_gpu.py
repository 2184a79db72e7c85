"""Training the conditioning encoders on the HIP kernels (`train_backend="hip"`), on the MI355X.

  1. golden parity: every fixture case of tests/golden/encoder_grads*.pt (the unmodified reference's autograd, CPU) -- output < 1e-4,
     every gradient tensor < 1e-3 in rel = |a - b| / |b|, the metric and bounds of tests/test_backward_gpu.py;
  2. the HIP path really ran (the composite is never entered, the masked attention entry points are);
  3. kernel level: masked and dropout variants of the attention forward-with-LSE and backward against an fp64 attention on the
     operands the kernels see, explicit mask tensors, ragged lengths, self and cross form;
  4. the dropout mask: the debug entry equals the keep function restated in torch integer arithmetic (tests/encoder_golden.keep_mask)
     bit for bit; binomial bounds on the kept share and on the agreement between heads / calls / seeds; p = 0 gives the no-dropout kernels' bits;
  5. dropout gradients against the fp32 composite on the same GPU with the EXPLICIT mask;
  6. two passes give bit-identical gradients, `token_emb.weight.grad` included;
  7. `GraphedTrainStep` over a PhonemeEncoder: bit-identical to eager without dropout; with dropout a fresh mask per replay, and an eager
     pass given a replay's seed reproduces its loss bit for bit;
  8. the wrapper: `NaturalSpeech2(encoder_train_backend="hip")` against `"composite"`;
  9. the reference's default sizes against the fp32 composite.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, PhonemeEncoder, SpeechPromptEncoder, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd import autograd_path  # noqa: E402
from naturalspeech2_pytorch_amd.transformer import Transformer  # noqa: E402
from tests.encoder_golden import build_case, keep_mask, load_cases, rel, run_case  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402
from tests.parity_record import record  # noqa: E402

DEV = torch.device("cuda:0")
CASES = load_cases()
HB = training.HipBackend()
OUT_TOL, GRAD_TOL = 1e-4, 1e-3
COMPOSITE = {"Transformer": autograd_path.transformer_forward_autograd, "PhonemeEncoder": autograd_path.phoneme_encoder_autograd,
             "SpeechPromptEncoder": autograd_path.speech_prompt_encoder_autograd}


def call(m, *args, **kw):
    return m(*args, **kw)


def seeded(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def load_seeded(m, seed):
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    return m.to(DEV).train()


def fresh(build, seed):
    """a module with PyTorch's default initialisation under a fixed seed, on the GPU in train() mode.

    Why not tests/golden/gen.make_weights at the reference's DEFAULT sizes (tests 8 and 9): with its unit-gain weights and 0.1 N biases the eight
    unnormalised SiLU convolutions of SpeechPromptEncoder lose the signal and keep the biases -- every token row leaves the encoder as the same
    vector (row spread 0.6 % of the magnitude; 2 % for PhonemeEncoder after six unit-gain residual layers).  Attention over identical
    keys is uniform, and d to_q = sum_k dS_k k_k with sum_k dS_k = 0 becomes a cancellation residue: the fp32 composite itself then
    resolves the to_q gradients of layers 1-5 only to 7e-2 (prompt) / 4e-3 (phoneme) against its own fp64 evaluation -- it is no yardstick for a
    1e-3 bound there.  PyTorch's default initialisation keeps PhonemeEncoder's rows apart (spread 76 %, composite vs fp64 <= 2e-6 per
    tensor); SpeechPromptEncoder additionally needs convolutions that preserve the variance through SiLU (`keep_variance`).  The tests
    assert that conditioning (`assert_yardstick_resolves`) instead of trusting it."""
    torch.manual_seed(seed)
    return build().to(DEV).train()


def keep_variance(enc):
    """scale the k = 9 convolutions of a default-initialised SpeechPromptEncoder to a variance-preserving gain for SiLU: default weights
    have std 1 / sqrt(3 fan_in); E[silu(z)^2] = 0.355 for z ~ N(0, 1), so gain^2 = 1 / 0.355 (gain 1.68) keeps the second moment"""
    with torch.no_grad():
        for c in enc.conv:
            if isinstance(c, torch.nn.Conv1d):
                c.weight.mul_(1.68 * math.sqrt(3.0))
    return enc


def assert_yardstick_resolves(enc, ref, args, kw, x, proj, grads32, bound=1e-4):
    """the fp32 composite against its own fp64 evaluation: every gradient tensor ten times finer than the bound it is the yardstick for"""
    import copy
    e64 = copy.deepcopy(enc).double()
    x64 = None if x is None else x.detach().double().requires_grad_(True)
    _, g64 = run_case(e64, ref, args if x is None else (x64,), kw, x64, proj.double())
    worst = max((rel(grads32[k], g64[k]), k) for k in g64)
    print("yardstick (fp32 composite vs fp64 composite), worst tensor:", worst)
    assert worst[0] < bound, worst


def compare(tag, out, grads, out_ref, grads_ref, rec=True):
    errs = {}
    for k, ref in grads_ref.items():
        assert grads.get(k) is not None, f"{tag}: no gradient for {k}"
        assert torch.isfinite(grads[k]).all(), (tag, k)
        errs[k] = rel(grads[k], ref)
    worst = max(errs.items(), key=lambda kv: kv[1])
    res = dict(n_tensors=len(errs), worst_tensor=worst[0], worst_rel=worst[1], out_rel=rel(out, out_ref))
    print(tag, res)
    if rec:
        record(f"encoder_training/{tag}", res)
    assert res["out_rel"] < OUT_TOL, (tag, res)
    for k, e in errs.items():
        assert e < GRAD_TOL, (tag, k, e)
    return res


@pytest.fixture()
def no_composite(monkeypatch):
    """a silent fall-back to the PyTorch composite fails the test"""
    def refuse(*a, **k):
        raise AssertionError("the PyTorch composite was entered: the HIP training path did not run")
    for name in ("transformer_forward_autograd", "phoneme_encoder_autograd", "speech_prompt_encoder_autograd"):
        monkeypatch.setattr(autograd_path, name, refuse)


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_parity(no_composite, name):
    meta = CASES[name]
    m, args, kw, x, proj = build_case(meta, DEV, train_backend="hip")
    out, grads = run_case(m, call, args, kw, x, proj)
    assert sorted(grads) == sorted(meta["grads"])
    compare(f"golden/{name}", out, grads, meta["out"], meta["grads"])


def test_the_hip_path_really_ran(no_composite, monkeypatch):
    counts = {}

    def counted(name):
        real = getattr(training.HipBackend, name)

        def f(self, *a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(self, *a, **k)
        monkeypatch.setattr(training.HipBackend, name, f)
    for name in ("attention", "attention_masked", "attention_bwd", "silu_fwd", "silu_bwd", "embedding_bwd", "gemm_f32", "wgrad"):
        counted(name)
    meta = CASES["phoneme"]
    m, args, kw, x, proj = build_case(meta, DEV, train_backend="hip")
    run_case(m, call, args, kw, x, proj)
    depth = meta["kwargs"]["depth"]
    assert counts["attention_masked"] == depth and counts["attention_bwd"] == depth and counts.get("attention", 0) == 0
    assert counts["silu_fwd"] == 1 and counts["silu_bwd"] == 1 and counts["embedding_bwd"] == 1 and counts["gemm_f32"] > 10
    counts.clear()
    meta = CASES["prompt"]
    m, args, kw, x, proj = build_case(meta, DEV, train_backend="hip")
    run_case(m, call, args, kw, x, proj)
    n_conv = len(meta["kwargs"]["dims"])
    assert counts["attention"] == depth and counts.get("attention_masked", 0) == 0          # no mask, dropout 0: the unmasked kernels
    assert counts["silu_fwd"] == n_conv and counts["wgrad"] >= n_conv                         # the "same" convs: transposed-copy wgrad
    # and the composite refuses what the kernels are not written for, exactly as Model does
    monkeypatch.undo()
    tr = Transformer(dim=64, depth=1, dim_head=32, heads=2, train_backend="hip").to(DEV).train()
    y = tr(torch.randn(1, 9, 64, device=DEV, requires_grad=True))
    assert y.grad_fn is not None


# ------------------------------------------------------------------------------------------------ 3
def _operands(B, H, Nq, Nk, cross):
    a = H * 64
    rnd = lambda n, shape, s: make_input(n, shape, seed=s)               # noqa: E731
    q, k, v = (rnd(n, (B * L, a), s) for n, s, L in (("aq", 17, Nq), ("ak", 18, Nk), ("av", 19, Nk)))
    do = rnd("ado", (B * Nq, a), 20)
    if cross:
        qp, kvp = HB.split(q.to(DEV)), HB.split(torch.cat((k, v), -1).to(DEV))
        kp, vp, qc, kc, vc = kvp, kvp, 0, 0, a
    else:
        qkv = HB.split(torch.cat((q, k, v), -1).to(DEV))
        qp, kp, vp, qc, kc, vc = qkv, qkv, qkv, 0, a, 2 * a
    return qp, kp, vp, qc, kc, vc, do


@pytest.mark.parametrize("masked,p", [(True, 0.0), (False, 0.2), (True, 0.2)], ids=["mask", "dropout", "mask_dropout"])
@pytest.mark.parametrize("B,H,Nq,Nk,cross", [(2, 2, 200, 200, False), (3, 2, 37, 37, False), (2, 3, 150, 75, True), (1, 2, 257, 129, True)])
def test_masked_and_dropout_attention_forward_and_backward(B, H, Nq, Nk, cross, masked, p):
    a = H * 64
    qp, kp, vp, qc, kc, vc, do = _operands(B, H, Nq, Nk, cross)
    join = lambda pl: ops.join(pl).cpu()                                # noqa: E731
    qr, kr, vr = join(qp)[:, qc:qc + a], join(kp)[:, kc:kc + a], join(vp)[:, vc:vc + a]      # what the planes hold
    kmask = None
    if masked:                                                           # an explicit mask tensor: a prefix and scattered holes
        lens = torch.tensor([Nk, max(1, Nk // 2), 5][:B])
        kmask = torch.arange(Nk)[None] < lens[:, None]
        kmask[0, 3::7] = False
    seed = seeded(0x0123456789ABCDEF)
    drop = (p, seed, 3) if p > 0 else None
    km_dev = None if kmask is None else kmask.to(torch.uint8).to(DEV)
    vt = HB.transpose(vp, vc, a, Nk, per_batch=True)
    o, lse = HB.attention_masked(qp, qc, kp, kc, vt, B, H, Nq, Nk, kmask=km_dev, drop=drop)
    delta = HB.attention_delta(do.to(DEV), o, B, H, Nq)
    do_row, _, _ = HB.grad_prep(do.to(DEV), a, want_row=True)
    dq = torch.full((B * Nq, a), float("nan"), device=DEV)
    dkv = torch.full((B * Nk, 2 * a), float("nan"), device=DEV)
    HB.attention_bwd_masked(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, dq=(dq, 0), dkv=(dkv, 0, a), kmask=km_dev, drop=drop)
    # fp64 attention on the plane values with the explicit masks
    tq, tk, tv = (t.double().clone().requires_grad_(True) for t in (qr, kr, vr))
    hd = lambda t, n: t.reshape(B, n, H, 64).transpose(1, 2)            # noqa: E731
    s = hd(tq, Nq) @ hd(tk, Nk).transpose(2, 3) * 0.125
    if kmask is not None:
        s = s.masked_fill(~kmask[:, None, None, :], float("-inf"))
    P = s.softmax(-1)
    if p > 0:
        P = P * keep_mask(int(seed.item()), 3, p, B, H, Nq, Nk).double() / (1.0 - float(np.float32(p)))
    out = (P @ hd(tv, Nk)).transpose(1, 2).reshape(B * Nq, a)
    (out * join(do_row).double()).sum().backward()
    lse_ref = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    e = dict(o=rel(join(o), out), lse=(lse.cpu().double() - lse_ref).abs().max().item(), dq=rel(dq, tq.grad), dk=rel(dkv[:, :a], tk.grad),
             dv=rel(dkv[:, a:], tv.grad))
    print(e)
    assert e["o"] < 2e-5 and e["lse"] < 1e-4, e                          # the bounds of test_attention_forward_lse_and_backward
    assert max(e["dq"], e["dk"], e["dv"]) < 5e-5, e
    if kmask is not None:                                                # masked keys: dK = dV = 0 exactly
        dead = (~kmask).reshape(-1).to(DEV)
        assert (dkv[dead] == 0).all()
    if not cross:                                                        # the gradients as operand planes = the conversion of the fp32 ones
        gp = HB.new_planes(B * Nq, 3 * a)
        HB.attention_bwd_masked(qp, qc, kp, kc, vp, vc, do_row, lse, delta, B, H, Nq, Nk, planes=(gp, 0, a, 2 * a), kmask=km_dev, drop=drop)
        assert torch.equal(ops.join(gp), ops.join(HB.split(torch.cat((dq, dkv), -1))))


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("B,H,Nq,Nk,p,seed,call_ix", [(2, 3, 37, 53, 0.2, 1, 0), (1, 2, 200, 131, 0.5, 0x7FFFFFFFFFFFFFFB, 5),
                                                       (3, 1, 64, 64, 0.1, 0x0123456789ABCDEF, 11), (1, 1, 5, 7, 0.0, 42, 0)])
def test_keep_mask_equals_its_restatement_bit_for_bit(B, H, Nq, Nk, p, seed, call_ix):
    got = HB.dropout_keep_mask(seeded(seed), call_ix, p, B, H, Nq, Nk).cpu().bool()
    assert torch.equal(got, keep_mask(seed, call_ix, p, B, H, Nq, Nk))


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_keep_mask_statistics(p):
    B, H, Nq, Nk = 2, 2, 512, 512
    N = B * H * Nq * Nk
    assert N >= 10 ** 6
    m = {(s, c): HB.dropout_keep_mask(seeded(s), c, p, B, H, Nq, Nk).bool() for s, c in ((101, 0), (101, 1), (102, 0))}
    base = m[(101, 0)]
    share = base.float().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / N)
    print("kept share", share, "+-", bound)
    assert abs(share - (1 - p)) <= bound
    e = p * p + (1 - p) ** 2                                             # two independent masks agree with this probability
    for tag, x, y in (("heads", base[:, 0], base[:, 1]), ("calls", base, m[(101, 1)]), ("seeds", base, m[(102, 0)])):
        n = x.numel()
        agree = (x == y).float().mean().item()
        sig = math.sqrt(e * (1 - e) / n)
        print(tag, agree, e, 5 * sig)
        assert abs(agree - e) <= 5 * sig, (tag, agree)


def test_dropout_zero_is_the_no_dropout_kernel_bit_for_bit():
    """dropout_p = 0 through the masked entry points (a seed given or not) gives the bits of the plain entry points, forward and backward:
    the library runs the kernels without dropout for it"""
    B, H, Nq, Nk = 2, 2, 150, 150
    a = H * 64
    qp, kp, vp, qc, kc, vc, do = _operands(B, H, Nq, Nk, False)
    vt = HB.transpose(vp, vc, a, Nk, per_batch=True)
    o0, lse0 = HB.attention(qp, qc, kp, kc, vt, B, H, Nq, Nk)
    o1, lse1 = HB.attention_masked(qp, qc, kp, kc, vt, B, H, Nq, Nk, drop=(0.0, seeded(7), 0))
    assert torch.equal(o0.buf, o1.buf) and torch.equal(lse0, lse1)
    delta = HB.attention_delta(do.to(DEV), o0, B, H, Nq)
    do_row, _, _ = HB.grad_prep(do.to(DEV), a, want_row=True)
    g = [torch.empty(B * Nq, 3 * a, device=DEV) for _ in range(2)]
    HB.attention_bwd(qp, qc, kp, kc, vp, vc, do_row, lse0, delta, B, H, Nq, Nk, dq=(g[0], 0), dkv=(g[0], a, 2 * a))
    HB.attention_bwd_masked(qp, qc, kp, kc, vp, vc, do_row, lse0, delta, B, H, Nq, Nk, dq=(g[1], 0), dkv=(g[1], a, 2 * a),
                            drop=(0.0, seeded(7), 0))
    assert torch.equal(g[0], g[1])


# ------------------------------------------------------------------------------------------------ 5
def transformer_with_explicit_keep(tr, x, mask, seed, p):
    """the fp32 composite with softmax(S) * keep / (1 - p) @ V, keep from the kernels' debug entry"""
    b, n, _ = x.shape
    h = x
    for li, (n1, attn, n2, ff) in enumerate(tr.layers):
        xn = autograd_path._rmsnorm(h, n1)
        q = attn.to_q(xn)
        k, v = attn.to_kv(xn).chunk(2, dim=-1)
        sp = lambda t: t.reshape(b, n, tr.heads, 64).transpose(1, 2)          # noqa: E731
        s = (sp(q) @ sp(k).transpose(2, 3)) * 0.125
        if mask is not None:
            s = s.masked_fill(~mask[:, None, None, :], -torch.finfo(s.dtype).max)
        keep = HB.dropout_keep_mask(seed, li, p, b, tr.heads, n, n).float() / (1.0 - float(np.float32(p)))
        o = ((s.softmax(-1) * keep) @ sp(v)).transpose(1, 2).reshape(b, n, -1)
        h = attn.to_out(o) + h
        h = autograd_path._feedforward(autograd_path._rmsnorm(h, n2), ff, False) + h
    return autograd_path._rmsnorm(h, tr.norm) if hasattr(tr.norm, "gamma") else h


def test_dropout_gradients_of_the_transformer(no_composite):
    p = 0.2
    tr = load_seeded(Transformer(dim=128, depth=2, heads=2, dropout=p, final_norm=True, train_backend="hip"), 91)
    b, n = 3, 150
    x = make_input("x", (b, n, 128), seed=92).to(DEV).requires_grad_(True)
    mask = (torch.arange(n)[None] < torch.tensor([150, 77, 9])[:, None]).to(DEV)
    proj = make_input("proj", (b, n, 128), seed=93).to(DEV)
    tr.dropout_seed = seeded(0x5EED5EED5EED)
    out, grads = run_case(tr, call, (x,), dict(mask=mask), x, proj)
    ref = lambda m, xx, mask: transformer_with_explicit_keep(m, xx, mask, tr.dropout_seed, p)      # noqa: E731
    out0, grads0 = run_case(tr, ref, (x,), dict(mask=mask), x, proj)
    compare("dropout/transformer", out, grads, out0, grads0)


def test_dropout_gradients_of_the_speech_prompt_encoder_at_its_default_dropout(no_composite):
    enc = load_seeded(SpeechPromptEncoder(32, dims=(64, 96, 64), depth=2, heads=2, train_backend="hip"), 94)
    assert enc.transformer.dropout == 0.2
    b, n = 2, 90
    x = make_input("x", (b, n, 32), seed=95).to(DEV).requires_grad_(True)
    proj = make_input("proj", (b, n, 64), seed=96).to(DEV)
    enc.transformer.dropout_seed = seeded(0xABCDEF0123)
    out, grads = run_case(enc, call, (x,), {}, x, proj)

    def ref(enc, xx):
        h = xx.transpose(1, 2)
        for m in enc.conv:
            if isinstance(m, torch.nn.Conv1d):
                h = F.silu(F.conv1d(h, m.weight, m.bias, padding=enc.padding))
        return transformer_with_explicit_keep(enc.transformer, h.transpose(1, 2), None, enc.transformer.dropout_seed, 0.2)
    out0, grads0 = run_case(enc, ref, (x,), {}, x, proj)
    compare("dropout/speech_prompt_encoder", out, grads, out0, grads0)


# ------------------------------------------------------------------------------------------------ 6
def test_two_passes_give_bit_identical_gradients(no_composite):
    enc = load_seeded(PhonemeEncoder(num_tokens=40, dim=64, dim_hidden=128, depth=2, heads=2, conv_dropout=0., attn_dropout=0.2, train_backend="hip"), 97)
    b, n = 4, 300
    ids = torch.randint(0, 40, (b, n), generator=torch.Generator().manual_seed(98))
    lens = torch.tensor([300, 211, 64, 7])
    mask = torch.arange(n)[None] < lens[:, None]
    ids = torch.where(mask, ids, torch.full_like(ids, -1)).to(DEV)
    proj = make_input("proj", (b, n, 128), seed=99).to(DEV)
    enc.transformer.dropout_seed = seeded(31337)
    out1, g1 = run_case(enc, call, (ids,), dict(mask=mask.to(DEV)), None, proj)
    out2, g2 = run_case(enc, call, (ids,), dict(mask=mask.to(DEV)), None, proj)
    assert torch.equal(out1, out2)
    for k in g1:
        assert g1[k] is not None and torch.equal(g1[k], g2[k]), k
    assert g1["token_emb.weight"].abs().sum() > 0 and g1["token_emb.weight"][enc.pad_id].abs().sum() > 0     # the padding row is an ordinary row


# ------------------------------------------------------------------------------------------------ 7
def _phoneme_graph_setup(attn_dropout):
    enc = load_seeded(PhonemeEncoder(num_tokens=40, dim=64, dim_hidden=128, depth=2, heads=2, conv_dropout=0., attn_dropout=attn_dropout,
                                     train_backend="hip"), 101)
    b, n = 2, 160
    mask = (torch.arange(n)[None] < torch.tensor([160, 99])[:, None])
    ids = torch.where(mask, torch.randint(0, 40, (b, n), generator=torch.Generator().manual_seed(102)), torch.tensor(-1)).to(DEV)
    proj = make_input("proj", (b, n, 128), seed=103).to(DEV)
    mask = mask.to(DEV)
    loss_fn = lambda i, w: (enc(i, mask=mask) * w).mean()                # noqa: E731
    return enc, ids, proj, loss_fn


def _eager(enc, loss_fn, ins):
    for q in enc.parameters():
        q.grad = None
    loss = loss_fn(*ins)
    loss.backward()
    return loss.detach().clone(), {k: q.grad.detach().clone() for k, q in enc.named_parameters()}


def test_graphed_step_without_dropout_is_the_eager_pass_bit_for_bit(no_composite):
    enc, ids, proj, loss_fn = _phoneme_graph_setup(0.)
    step = training.GraphedTrainStep(loss_fn, (ids, proj), enc)
    l_e, g_e = _eager(enc, loss_fn, (ids, proj))
    for q in enc.parameters():
        q.grad = None
    l_g = step(ids, proj).detach().clone()
    assert torch.equal(l_g, l_e)
    for k, q in enc.named_parameters():
        assert q.grad is not None and torch.equal(q.grad, g_e[k]), k


def test_graphed_step_with_dropout_draws_a_mask_per_replay_and_is_reproducible_from_its_seed(no_composite):
    enc, ids, proj, loss_fn = _phoneme_graph_setup(0.2)
    step = training.GraphedTrainStep(loss_fn, (ids, proj), enc)
    seen = []
    for _ in range(2):
        loss = step(ids, proj).detach().clone()
        seen.append((loss, enc.transformer.last_dropout_seed.detach().clone(), {k: q.grad.detach().clone() for k, q in enc.named_parameters()}))
    assert not torch.equal(seen[0][1], seen[1][1]), "the seed did not change between replays"
    assert not torch.equal(seen[0][0], seen[1][0]), "two replays on the same inputs gave the same loss: the mask did not change"
    for loss, seed, grads in seen:                                       # an eager pass given the replay's seed: the same loss, bit for bit
        enc.transformer.dropout_seed = seed
        l_e, g_e = _eager(enc, loss_fn, (ids, proj))
        assert torch.equal(l_e, loss)
        for k in grads:
            assert torch.equal(grads[k], g_e[k]), k
    enc.transformer.dropout_seed = None


# ------------------------------------------------------------------------------------------------ 8
def test_wrapper_trains_its_encoders_on_the_hip_path():
    mk = dict(dim=128, depth=2, wavenet_layers=4, wavenet_stacks=2, dim_prompt=512, condition_on_prompt=True, cond_drop_prob=0.)
    b, n_ph, T, n_p = 2, 40, 128, 70
    text = torch.randint(0, 150, (b, n_ph), generator=torch.Generator().manual_seed(111)).to(DEV)
    text_lens = torch.tensor([40, 31], device=DEV)
    mel_lens = torch.tensor([128, 100], device=DEV)
    mel = make_input("mel", (b, 80, T), seed=112).to(DEV)
    pitch = (80 + 300 * make_input("pitch", (b, 1, T), seed=113, uniform=True)).to(DEV)
    audio = make_input("audio", (b, T, 128), seed=114).to(DEV)
    prompt = make_input("prompt", (b, n_p, 128), seed=115).to(DEV)
    times, noise = make_input("times", (b,), seed=116, uniform=True).to(DEV), make_input("noise", (b, T, 128), seed=117).to(DEV)
    res = {}
    for backend in ("composite", "hip"):
        # (default initialisation under one seed: the same weights in both wrappers; see `fresh` for why not make_weights at these sizes)
        d = fresh(lambda: NaturalSpeech2(Model(**mk), codec=None, target_sample_hz=24000, build_aligner=True, encoder_train_backend=backend), 118)
        keep_variance(d.prompt_enc)
        d.model.load_state_dict(make_weights({k: tuple(v.shape) for k, v in d.model.state_dict().items()}, seed=119))     # (as every Model test)
        d.phoneme_enc.conv_dropout = 0.
        d.prompt_enc.transformer.dropout = 0.                            # all dropouts 0: the two wrappers see the same arithmetic
        assert d.phoneme_enc.train_backend == backend and d.prompt_enc.transformer.train_backend == backend
        entered = []
        real = autograd_path.transformer_forward_autograd
        autograd_path.transformer_forward_autograd = lambda *a, **k: (entered.append(1), real(*a, **k))[1]
        try:
            loss = d(audio, text=text, text_lens=text_lens, mel=mel, mel_lens=mel_lens, pitch=pitch, prompt=prompt, times=times, noise=noise)
            loss.backward()
        finally:
            autograd_path.transformer_forward_autograd = real
        assert bool(entered) == (backend == "composite")
        res[backend] = (loss.detach().clone(), {k: q.grad.detach().clone() for k, q in d.named_parameters() if q.grad is not None})
    (l_c, g_c), (l_h, g_h) = res["composite"], res["hip"]
    assert g_c.keys() == g_h.keys()
    assert abs(float(l_h) - float(l_c)) / abs(float(l_c)) < 1e-4, (float(l_h), float(l_c))
    groups = {"phoneme_enc.": [], "prompt_enc.": [], "model.": []}
    for k in g_c:
        for pre in groups:
            if k.startswith(pre):
                groups[pre].append((rel(g_h[k], g_c[k]), k))
    for pre, errs in groups.items():
        assert errs, pre
        worst = max(errs)
        print(pre, len(errs), "tensors, worst", worst)
        record(f"encoder_training/wrapper/{pre}", dict(n_tensors=len(errs), worst_rel=worst[0], worst_tensor=worst[1]))
        assert worst[0] < GRAD_TOL, (pre, worst)
    assert any(k.startswith("phoneme_enc.token_emb") for k in g_h) and len(groups["prompt_enc."]) > 40


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("which", ["phoneme", "prompt"])
def test_default_sizes_against_the_composite(no_composite, monkeypatch, which):
    b, n = 4, 256
    if which == "phoneme":
        enc = fresh(lambda: PhonemeEncoder(num_tokens=150, conv_dropout=0., attn_dropout=0., train_backend="hip"), 121)
        ids = torch.randint(0, 150, (b, n), generator=torch.Generator().manual_seed(122))
        mask = torch.arange(n)[None] < torch.tensor([256, 200, 131, 64])[:, None]
        args, kw, x = (torch.where(mask, ids, torch.full_like(ids, -1)).to(DEV),), dict(mask=mask.to(DEV)), None
    else:
        enc = keep_variance(fresh(lambda: SpeechPromptEncoder(128, dropout=0., train_backend="hip"), 123))
        x = make_input("x", (b, n, 128), seed=124).to(DEV).requires_grad_(True)
        args, kw = (x,), {}
    proj = make_input("proj", (b, n, 512), seed=125).to(DEV)
    out, grads = run_case(enc, call, args, kw, x, proj)                  # (the composite refuses to be entered here)
    monkeypatch.undo()                                                   # ... and is the yardstick from here on
    out0, grads0 = run_case(enc, COMPOSITE[type(enc).__name__], args, kw, x, proj)
    assert_yardstick_resolves(enc, COMPOSITE[type(enc).__name__], args, kw, x, proj, grads0)
    compare(f"default_sizes/{which}", out, grads, out0, grads0)
