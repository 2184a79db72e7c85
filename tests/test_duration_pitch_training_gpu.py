"""Training the DurationPitchPredictor on the HIP kernels (`train_backend="hip"`), on the MI355X.

  1. golden parity: every fixture case of tests/golden/duration_pitch_grads*.pt (the unmodified reference's autograd, CPU) -- outputs < 1e-4,
     every gradient tensor < 1e-3 in rel = |a - b| / |b|, the metric and bounds of tests/test_backward_gpu.py;
  2. the HIP path really ran (the composite is never entered; call counts of the new GroupNorm / head entries and of the attention backward);
  3. kernel level: GroupNorm + SiLU (+ residual) forward / backward against fp64 torch, bound = max(1e-5, 4 x the error of PyTorch's own fp32
     group_norm + silu backward on the same GPU against the same fp64 result); the head backward, with exactly zero rows under the ReLU;
  4. dropout gradients against an fp32 restatement on the same GPU with the EXPLICIT keep masks, applied to the attention probabilities only;
  5. two passes give bit-identical gradients, `phoneme_token_emb.weight.grad` included;
  6. `GraphedTrainStep` over a predictor without dropout: bit-identical to eager;
  7. the wrapper: `NaturalSpeech2(duration_pitch_train_backend="hip")` against `"composite"` through forward(..., return_aux_losses=True);
  8. the reference's width (dim_hidden 512, 8 heads) against the fp32 composite, which is first shown to resolve its own fp64 evaluation.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, NaturalSpeech2, training  # noqa: E402
from naturalspeech2_pytorch_amd import autograd_path  # noqa: E402
from naturalspeech2_pytorch_amd.training.functions import GroupNormSiluFn, RowDotReluFn  # noqa: E402
from tests.duration_pitch_golden import build_case, load_cases, rel, run_case  # noqa: E402
from tests.golden.gen import make_input  # noqa: E402
from tests.parity_record import record  # noqa: E402

DEV = torch.device("cuda:0")
CASES = load_cases()
HB = training.HipBackend()
OUT_TOL, GRAD_TOL = 1e-4, 1e-3


def call(m, x, prompts):
    return m(x, prompts)


def seeded(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def shares_ok(*outs):
    """the ReLU of each head both passes and blocks gradient (else the comparison below it says little)"""
    return all(0.1 <= float((o > 0).float().mean()) <= 0.9 for o in outs)


def compare(tag, outs, grads, outs_ref, grads_ref, out_tol=OUT_TOL, rec=True):
    errs = {}
    for k, ref in grads_ref.items():
        assert grads.get(k) is not None, f"{tag}: no gradient for {k}"
        assert torch.isfinite(grads[k]).all(), (tag, k)
        errs[k] = rel(grads[k], ref)
    worst = max(errs.items(), key=lambda kv: kv[1])
    res = dict(n_tensors=len(errs), worst_tensor=worst[0], worst_rel=worst[1], duration_rel=rel(outs[0], outs_ref[0]),
               pitch_rel=rel(outs[1], outs_ref[1]))
    print(tag, res)
    if rec:
        record(f"duration_pitch_training/{tag}", res)
    assert res["duration_rel"] < out_tol and res["pitch_rel"] < out_tol, (tag, res)
    for k, e in errs.items():
        assert e < GRAD_TOL, (tag, k, e)
    return res


@pytest.fixture()
def no_composite(monkeypatch):
    """a silent fall-back to the PyTorch composite fails the test"""
    def refuse(*a, **k):
        raise AssertionError("the PyTorch composite was entered: the HIP training path did not run")
    monkeypatch.setattr(autograd_path, "duration_pitch_autograd", refuse)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_parity(no_composite, name):
    meta = CASES[name]
    m, x, prompts, xf, projs = build_case(meta, DEV, train_backend="hip")
    dur, pitch, grads = run_case(m, call, x, prompts, xf, projs)
    assert sorted(grads) == sorted(meta["grads"])
    compare(f"golden/{name}", (dur, pitch), grads, (meta["duration"], meta["pitch"]), meta["grads"])


# ------------------------------------------------------------------------------------------------ 2
def test_the_hip_path_really_ran(no_composite, monkeypatch):
    counts = {}

    def counted(name):
        real = getattr(training.HipBackend, name)

        def f(self, *a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(self, *a, **k)
        monkeypatch.setattr(training.HipBackend, name, f)
    for name in ("groupnorm_silu_fwd", "groupnorm_silu_bwd", "row_dot_relu", "row_dot_relu_bwd", "attention", "attention_masked", "attention_bwd",
                 "silu_fwd", "embedding_bwd"):
        counted(name)
    meta = CASES["resnet"]
    depth = meta["kwargs"]["depth"]
    m, x, prompts, xf, projs = build_case(meta, DEV, train_backend="hip")
    run_case(m, call, x, prompts, xf, projs)
    assert counts["groupnorm_silu_fwd"] == 2 * depth * 3 * 2 and counts["groupnorm_silu_bwd"] == 2 * depth * 3 * 2
    assert counts["attention"] == 2 * depth and counts["attention_bwd"] == 2 * depth and counts.get("attention_masked", 0) == 0
    assert counts["row_dot_relu"] == 2 and counts["row_dot_relu_bwd"] == 2 and counts.get("silu_fwd", 0) == 0
    counts.clear()
    meta = CASES["convblock_k5"]
    m, x, prompts, xf, projs = build_case(meta, DEV, train_backend="hip")
    run_case(m, call, x, prompts, xf, projs)
    assert counts["silu_fwd"] == 2 * 3 and counts.get("groupnorm_silu_fwd", 0) == 0
    counts.clear()
    meta = CASES["resnet_tokens"]
    m, x, prompts, xf, projs = build_case(meta, DEV, train_backend="hip")
    run_case(m, call, x, prompts, xf, projs)
    assert counts["embedding_bwd"] == 1
    # and the composite takes what the kernels are not written for, exactly as Model and the encoders do
    monkeypatch.undo()
    dp = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=2, dim_head=32, train_backend="hip").to(DEV).train()
    d, _ = dp(torch.randn(1, 9, 64, device=DEV, requires_grad=True), torch.randn(1, 5, 64, device=DEV))
    assert d.grad_fn is not None


# ------------------------------------------------------------------------------------------------ 3
GN_SHAPES = [(2, 1, 32), (3, 37, 64), (2, 130, 512), (1, 600, 64)]


@pytest.mark.parametrize("offset", [0.0, 100.0], ids=["mean0", "mean100"])
@pytest.mark.parametrize("with_resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("B,n,C", GN_SHAPES)
def test_groupnorm_silu_forward_and_backward_against_fp64(B, n, C, with_resid, offset):
    """(2, 1, 32): a single row, groups of 4 values; (3, 37, 64): one statistics chunk, two column-sum slots with a ragged one;
    (2, 130, 512): cg = 64 -> three statistics chunks of 64 rows with a ragged last one, five column-sum slots; (1, 600, 64): cg = 8 -> two
    statistics chunks of 512 rows, nineteen column-sum slots.  mean100: inputs of mean 100 and std 1 (the shifted statistics)"""
    groups, eps = 8, 1e-5
    M = B * n
    x = make_input("gn_x", (M, C), seed=201) + offset
    gamma = 1.0 + 0.3 * make_input("gn_gamma", (C,), seed=202)
    beta = 0.3 * make_input("gn_beta", (C,), seed=203)
    resid = make_input("gn_resid", (M, C), seed=204) if with_resid else None
    w = make_input("gn_w", (M, C), seed=205)

    def torch_ref(dtype):
        ts = [t.to(DEV, dtype).requires_grad_(True) if t is not None else None for t in (x, gamma, beta, resid)]
        xx, g, b_, r = ts
        y = F.silu(F.group_norm(xx.reshape(B, n, C).transpose(1, 2), groups, g, b_, eps)).transpose(1, 2).reshape(M, C)
        if r is not None:
            y = y + r
        (y * w.to(DEV, dtype)).sum().backward()
        return dict(y=y.detach(), dx=xx.grad, dgamma=g.grad, dbeta=b_.grad), (None if r is None else r.grad)

    ref64, _ = torch_ref(torch.float64)
    ref32, _ = torch_ref(torch.float32)
    xx, g, b_ = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    r = None if resid is None else resid.to(DEV).requires_grad_(True)
    y = GroupNormSiluFn.apply(xx, g, b_, r, n, groups, eps)
    (y * w.to(DEV)).sum().backward()
    got = dict(y=y.detach(), dx=xx.grad, dgamma=g.grad, dbeta=b_.grad)
    res = {}
    for k in got:
        e_hip, e_torch = rel(got[k], ref64[k]), rel(ref32[k], ref64[k])
        res[k] = dict(hip=e_hip, torch_fp32=e_torch)
    print((B, n, C), with_resid, offset, res)
    record(f"duration_pitch_training/groupnorm_bwd/{B}x{n}x{C}/{'resid' if with_resid else 'plain'}/mean{int(offset)}", res)
    for k, e in res.items():
        assert torch.isfinite(got[k]).all(), k
        assert e["hip"] < max(1e-5, 4 * e["torch_fp32"]), (k, e)
    if r is not None:
        assert torch.equal(r.grad, w.to(DEV))                                    # the residual's gradient is dy itself


@pytest.mark.parametrize("M,K", [(1, 32), (111, 64), (300, 512)])
def test_head_backward_against_fp64(M, K):
    """(1, 32): one row, one slot; (111, 64): two 64-row slots with a ragged one, 16 rows in flight; (300, 512): five slots, 2 rows in flight.
    Bound 1e-5: fp32 sums of at most 300 terms of either sign (~ sqrt(300) 6e-8) with room for the cancellation in dw"""
    h = make_input("rd_h", (M, K), seed=211)
    w = make_input("rd_w", (1, K), seed=212) / K ** 0.5
    b = torch.tensor([0.1])
    dout = make_input("rd_dout", (M,), seed=213)
    pre64 = h.double() @ w.double().reshape(-1) + b.double()
    assert float(pre64.abs().min()) > 1e-4, "a pre-activation too close to 0 for a gate comparison"
    hh, ww, bb = (t.to(DEV).requires_grad_(True) for t in (h, w, b))
    out = RowDotReluFn.apply(hh, ww, bb)
    (out * dout.to(DEV)).sum().backward()
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    out64 = F.relu(F.linear(h64, w64, b64)[..., 0])
    (out64 * dout.double()).sum().backward()
    res = dict(out=rel(out, out64), dh=rel(hh.grad, h64.grad), dw=rel(ww.grad, w64.grad), db=rel(bb.grad, b64.grad))
    print((M, K), res)
    record(f"duration_pitch_training/head_bwd/{M}x{K}", res)
    if M > 1:
        assert 0 < int((pre64 > 0).sum()) < M
    dead = (pre64 <= 0).to(DEV)
    assert (hh.grad[dead] == 0).all() and (out[dead] == 0).all()
    assert ww.grad.shape == (1, K) and bb.grad.shape == (1,)
    if bool((pre64 > 0).any()):
        for k, e in res.items():
            assert e < 1e-5, (k, e)
    else:
        assert float(ww.grad.abs().max()) == 0 and float(bb.grad.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4
def predictor_with_explicit_keep(dp, x, prompts, seed, p):
    """the fp32 composite with softmax(S) * keep / (1 - p) @ V, keep from the kernels' debug entry; dropout nowhere else"""
    if isinstance(dp.phoneme_token_emb, torch.nn.Embedding):
        x = dp.phoneme_token_emb(x)
    b, n, _ = x.shape
    n_k = n + prompts.shape[1]
    outs = []
    for ti, tr in enumerate((dp.to_duration_pred, dp.to_pitch_pred)):
        h, k_ = x, tr.kernel_size
        for li, (convs, norm, attn) in enumerate(tr.layers):
            for blk in convs:
                if tr.use_resnet_block:
                    y = h.transpose(1, 2)
                    for bl in blk.blocks:
                        y = F.conv1d(y, bl.proj.weight, bl.proj.bias, padding=k_ // 2)
                        y = F.silu(F.group_norm(y, bl.norm.num_groups, bl.norm.weight, bl.norm.bias, bl.norm.eps))
                    h = y.transpose(1, 2) + h
                else:
                    h = F.silu(F.conv1d(h.transpose(1, 2), blk[1].weight, blk[1].bias, padding=k_ // 2)).transpose(1, 2)
            xn = autograd_path._rmsnorm(h, norm)
            q = attn.to_q(xn)
            k, v = attn.to_kv(torch.cat((xn, prompts), dim=1)).chunk(2, dim=-1)
            sp = lambda t: t.reshape(b, t.shape[1], tr.heads, 64).transpose(1, 2)          # noqa: E731
            s = (sp(q) @ sp(k).transpose(2, 3)) * 0.125
            keep = HB.dropout_keep_mask(seed, ti * len(tr.layers) + li, p, b, tr.heads, n, n_k).float() / (1.0 - float(np.float32(p)))
            o = ((s.softmax(-1) * keep) @ sp(v)).transpose(1, 2).reshape(b, n, -1)
            h = attn.to_out(o) + h
        head = tr.to_pred[0]
        outs.append(F.relu(F.linear(h, head.weight, head.bias)[..., 0]))
    return tuple(outs)


def test_dropout_gradients_against_the_explicit_masks(no_composite):
    p = 0.2
    meta = CASES["resnet"]                                            # (weights under which both heads pass and block: the fixture's conditions)
    m, x, prompts, xf, projs = build_case(meta, DEV, train_backend="hip", dropout=p)
    assert m.dropout == p and m.to_pitch_pred.dropout == p
    m.dropout_seed = seeded(0x5EED5EED5EED)
    dur, pitch, grads = run_case(m, call, x, prompts, xf, projs)
    assert m.last_dropout_seed is m.dropout_seed
    ref = lambda mm, xx, pr: predictor_with_explicit_keep(mm, xx, pr, m.dropout_seed, p)      # noqa: E731
    dur0, pitch0, grads0 = run_case(m, ref, x, prompts, xf, projs)
    assert shares_ok(dur0, pitch0)
    assert rel(dur0, meta["duration"]) > 1e-2                         # the masks acted
    compare("dropout/resnet", (dur, pitch), grads, (dur0, pitch0), grads0, out_tol=1e-3)


# ------------------------------------------------------------------------------------------------ 5
def test_two_passes_give_bit_identical_gradients(no_composite):
    meta = CASES["resnet_tokens"]
    m, _, _, _, _ = build_case(meta, DEV, train_backend="hip", dropout=0.2)
    b, n, n_p = 4, 300, 70
    ids = torch.randint(0, 40, (b, n), generator=torch.Generator().manual_seed(221)).to(DEV)
    prompts = make_input("prompt_enc", (b, n_p, 64), seed=222).to(DEV).requires_grad_(True)
    projs = tuple(make_input(f"proj{i}", (b, n), seed=223).to(DEV) for i in range(2))
    m.dropout_seed = seeded(31337)
    d1, p1, g1 = run_case(m, call, ids, prompts, None, projs)
    d2, p2, g2 = run_case(m, call, ids, prompts, None, projs)
    assert torch.equal(d1, d2) and torch.equal(p1, p2)
    for k in g1:
        assert g1[k] is not None and torch.equal(g1[k], g2[k]), k
    assert g1["phoneme_token_emb.weight"].abs().sum() > 0 and g1["prompts"].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 6
def test_graphed_step_is_the_eager_pass_bit_for_bit(no_composite):
    meta = CASES["resnet"]
    m, _, _, _, _ = build_case(meta, DEV, train_backend="hip")
    b, n, n_p = 2, 160, 45
    x = make_input("phoneme_enc", (b, n, 64), seed=231).to(DEV)
    prompts = make_input("prompt_enc", (b, n_p, 64), seed=232).to(DEV)
    w = make_input("proj", (2, b, n), seed=233).to(DEV)

    def loss_fn(xx, pr, ww):
        dur, pitch = m(xx, pr)
        return (dur * ww[0]).mean() + (pitch * ww[1]).mean()

    step = training.GraphedTrainStep(loss_fn, (x, prompts, w), m)
    for q in m.parameters():
        q.grad = None
    l_e = loss_fn(x, prompts, w)
    l_e.backward()
    l_e, g_e = l_e.detach().clone(), {k: q.grad.detach().clone() for k, q in m.named_parameters()}
    for q in m.parameters():
        q.grad = None
    l_g = step(x, prompts, w).detach().clone()
    assert torch.equal(l_g, l_e)
    for k, q in m.named_parameters():
        assert q.grad is not None and torch.equal(q.grad, g_e[k]), k


# ------------------------------------------------------------------------------------------------ 7
def test_wrapper_trains_its_predictor_on_the_hip_path():
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
    torch.manual_seed(118)                                               # PyTorch's default initialisation under a fixed seed
    d = NaturalSpeech2(Model(**mk), codec=None, target_sample_hz=24000, build_aligner=True, build_duration_pitch=True,
                       duration_pitch_train_backend="hip")
    assert d.duration_pitch.train_backend == "hip"                       # the keyword reached the predictor the wrapper built
    d.duration_pitch = DurationPitchPredictor(dim=512, depth=1, dropout=0., train_backend="hip")      # (kept small: one layer per trunk)
    d = d.to(DEV).train()
    d.phoneme_enc.conv_dropout = 0.
    d.prompt_enc.transformer.dropout = 0.                                # all dropouts 0: the two passes see the same arithmetic
    res = {}
    for backend in ("composite", "hip"):                                 # one wrapper, one set of weights; the switch is an attribute
        d.duration_pitch.train_backend = backend
        d.zero_grad(set_to_none=True)
        entered = []
        real = autograd_path.duration_pitch_autograd
        autograd_path.duration_pitch_autograd = lambda *a, **k: (entered.append(1), real(*a, **k))[1]
        try:
            loss, aux = d(audio, text=text, text_lens=text_lens, mel=mel, mel_lens=mel_lens, pitch=pitch, prompt=prompt, times=times, noise=noise,
                          return_aux_losses=True)
            (loss + aux["aux"]).backward()
        finally:
            autograd_path.duration_pitch_autograd = real
        assert bool(entered) == (backend == "composite")
        res[backend] = ({k: aux[k].detach().clone() for k in ("duration", "pitch")},
                        {k: q.grad.detach().clone() for k, q in d.duration_pitch.named_parameters() if q.grad is not None})
    (a_c, g_c), (a_h, g_h) = res["composite"], res["hip"]
    assert g_c.keys() == g_h.keys() and len(g_c) == len(list(d.duration_pitch.parameters()))
    errs = [(rel(g_h[k], g_c[k]), k) for k in g_c]
    worst = max(errs)
    out = dict(duration_rel=rel(a_h["duration"], a_c["duration"]), pitch_rel=rel(a_h["pitch"], a_c["pitch"]), n_tensors=len(errs), worst_rel=worst[0],
               worst_tensor=worst[1])
    print(out)
    record("duration_pitch_training/wrapper", out)
    assert out["duration_rel"] < GRAD_TOL and out["pitch_rel"] < GRAD_TOL and worst[0] < GRAD_TOL, out


# ------------------------------------------------------------------------------------------------ 8
def test_the_reference_width_against_the_composite(no_composite, monkeypatch):
    torch.manual_seed(241)                                               # PyTorch's default initialisation under a fixed seed
    m = DurationPitchPredictor(dim=512, dim_hidden=512, heads=8, depth=1, dropout=0., train_backend="hip").to(DEV).train()
    x = make_input("phoneme_enc", (2, 70, 512), seed=242).to(DEV).requires_grad_(True)
    prompts = make_input("prompt_enc", (2, 33, 512), seed=243).to(DEV).requires_grad_(True)
    projs = tuple(make_input(f"proj{i}", (2, 70), seed=244).to(DEV) for i in range(2))
    dur, pitch, grads = run_case(m, call, x, prompts, x, projs)             # (the composite refuses to be entered here)
    monkeypatch.undo()                                                   # ... and is the yardstick from here on
    ref = autograd_path.duration_pitch_autograd
    dur0, pitch0, grads0 = run_case(m, ref, x, prompts, x, projs)
    assert shares_ok(dur0, pitch0)
    m64 = copy.deepcopy(m).double()
    x64, p64 = x.detach().double().requires_grad_(True), prompts.detach().double().requires_grad_(True)
    _, _, g64 = run_case(m64, ref, x64, p64, x64, tuple(t.double() for t in projs))
    worst = max((rel(grads0[k], g64[k]), k) for k in g64)
    print("yardstick (fp32 composite vs fp64 composite), worst tensor:", worst)
    assert worst[0] < 1e-4, worst
    compare("reference_width", (dur, pitch), grads, (dur0, pitch0), grads0, out_tol=1e-3)
