"""Ragged TRAINING batches on the MI355X (include/ns2hip_train.h): per-utterance lengths in the training forward and the backward
attention kernels, through AttnFn / model_forward_train, Model.forward(lens=) under autograd, NaturalSpeech2.forward(audio_lens=),
GraphedTrainStep and Trainer.  The definition under test: utterance i of a ragged batch contributes to the loss and to every gradient what
it contributes alone at lens[i] frames -- so what lies at or beyond a length (NaN included) must not reach a value or a gradient before
it, and the rows at or beyond it are exact zeros."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd.autograd_path import model_forward_autograd_ragged  # noqa: E402
from naturalspeech2_pytorch_amd.training import HipBackend, Trainer  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


def _record(key, value):
    """one measured figure: printed, and merged into $NS2_RECORD_DIR/ragged_training_tests.json when that is set (what profiles/ragged_training.json quotes)"""
    print(f"{key}: {value}")
    if not os.environ.get("NS2_RECORD_DIR"):
        return
    path = os.path.join(os.environ["NS2_RECORD_DIR"], "ragged_training_tests.json")
    cur = {}
    try:
        with open(path) as f:
            cur = json.load(f)
    except Exception:
        pass
    cur[key] = value
    with open(path, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rows(p, r0, n):
    return ops.Planes(p.buf[r0:r0 + n], n, p.ld, p.has_lo, p.fmt)


# ------------------------------------------------------------------------------------------------ 1, 2. the kernels, bit for bit
KB, KH, KN, KD = 7, 2, 512, 64                             # full; partial last tile; a 128-row own tile plus one row; exactly one own tile;
KLENS = [512, 447, 129, 128, 65, 64, 1]                    # one 64-row tile plus one row; exactly one tile; one row
KA = KH * KD


def _nan_rows(p, lens):
    """NaN into the packed planes of rows at or beyond each length (the conversions never see them)"""
    for b, n in enumerate(lens):
        p.buf.view(KB, KN, -1)[b, n:] = NAN


def _fwd_operands(seed):
    """q, k, V^T bf16 hi / lo planes of a self-attention; q rows, k rows and V^T columns at or beyond each length are NaN in every plane"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(KB * KN, KA, generator=g).to(DEV) for _ in range(3))
    qp, kp, vp = ops.split(q, precision=3), ops.split(k, precision=3), ops.split(v, precision=3)
    vt = ops.split(v.reshape(KB, KN, KA).transpose(1, 2).reshape(KB * KA, KN).contiguous(), ldo=KN, precision=3)
    _nan_rows(qp, KLENS), _nan_rows(kp, KLENS), _nan_rows(vp, KLENS)
    for b, n in enumerate(KLENS):                           # interleaved lines [hi(32) | lo(32)] per 32 logical columns
        cols = (torch.arange(KN, device=DEV) >= n).view(KN // 32, 1, 32).expand(KN // 32, 2, 32)
        vt.buf.view(KB, KA, KN // 32, 2, 32)[b][:, cols] = NAN
    return qp, kp, vp, vt


def _train_fwd(qp, kp, vt, B, N, o_prec, lens=None):
    return ops._attention_fwd(qp, 0, kp, 0, vt.hi, vt.lo, vt.ld, B, KH, N, N, 0.125, 3, o_precision=o_prec, want_lse=True, train_lens=lens)


@pytest.fixture(scope="module")
def kernel_case():
    qp, kp, vp, vt = _fwd_operands(seed=90)
    kl = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    return dict(q=qp, k=kp, v=vp, vt=vt, kl=kl)


@pytest.mark.parametrize("o_prec", [3, 4])
def test_training_forward_with_lengths_is_the_utterance_alone_bit_for_bit(kernel_case, o_prec):
    c = kernel_case
    o, lse = _train_fwd(c["q"], c["k"], c["vt"], KB, KN, o_prec, lens=c["kl"])
    bad = torch.tensor([0, 9999] + KLENS[2:], dtype=torch.int32, device=DEV)      # outside [1, N]: clamped into it
    o_bad, lse_bad = _train_fwd(c["q"], c["k"], c["vt"], KB, KN, o_prec, lens=bad)
    torch.cuda.synchronize()
    assert o.fmt == ("h8" if o_prec == 4 else "bf16")
    for b, n in enumerate(KLENS):
        solo_o, solo_lse = _train_fwd(_rows(c["q"], b * KN, n), _rows(c["k"], b * KN, n), _rows(c["vt"], b * KA, KA), 1, n, o_prec)     # the call that exists
        assert torch.equal(_bits(o.buf[b * KN:b * KN + n]), _bits(solo_o.buf)), f"o of utterance {b} (length {n})"
        assert torch.equal(lse[b, :, :n].contiguous().view(torch.int32), solo_lse[0].contiguous().view(torch.int32)), f"lse of utterance {b}"
        assert torch.count_nonzero(_bits(o.buf[b * KN + n:(b + 1) * KN])) == 0, f"o rows beyond length {n} must be zero bits"
        assert bool((lse[b, :, n:] == float("inf")).all()), f"lse beyond length {n} must be +inf"
    # lengths 0 and 9999 behave as 1 and N (utterance 0 is then one frame long: compared on that frame; utterance 1 is full either way)
    solo_o, solo_lse = _train_fwd(_rows(c["q"], 0, 1), _rows(c["k"], 0, 1), _rows(c["vt"], 0, KA), 1, 1, o_prec)
    assert torch.equal(_bits(o_bad.buf[:1]), _bits(solo_o.buf)) and torch.count_nonzero(_bits(o_bad.buf[1:KN])) == 0
    assert bool((lse_bad[0, :, 1:] == float("inf")).all()) and torch.equal(lse_bad[0, :, :1], solo_lse[0])
    # (utterance 1 with 9999: its q / k / V^T hold NaN from 447 on, so only the rest of the batch is compared with the good call; the clamp
    # to N is checked on clean operands below)
    assert torch.equal(_bits(o_bad.buf[2 * KN:]), _bits(o.buf[2 * KN:])) and torch.equal(lse_bad[2:].view(torch.int32), lse[2:].view(torch.int32))


def test_training_forward_clamps_lengths_on_clean_operands():
    """lens = [0, 9999, ...] is [1, N, ...]: the whole output, on operands without NaN"""
    g = torch.Generator().manual_seed(91)
    B, N = 3, 192
    q, k, v = (torch.randn(B * N, KA, generator=g).to(DEV) for _ in range(3))
    qp, kp = ops.split(q, precision=3), ops.split(k, precision=3)
    vt = ops.split(v.reshape(B, N, KA).transpose(1, 2).reshape(B * KA, N).contiguous(), ldo=N, precision=3)
    a = _train_fwd(qp, kp, vt, B, N, 3, lens=torch.tensor([0, 9999, 70], dtype=torch.int32, device=DEV))
    b = _train_fwd(qp, kp, vt, B, N, 3, lens=torch.tensor([1, N, 70], dtype=torch.int32, device=DEV))
    assert torch.equal(_bits(a[0].buf), _bits(b[0].buf)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.isfinite(ops.join(a[0])).all()
    with pytest.raises(_lib.Ns2Error, match="ns2_attention_fwd_lens: lse"):       # the inference entry keeps refusing the training forward
        ops._attention_fwd(qp, 0, kp, 0, vt.hi, vt.lo, vt.ld, B, KH, N, N, 0.125, 3, want_lse=True, key_lens=torch.ones(B, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("out", ["f32", "planes3", "planes4"])
def test_backward_with_lengths_is_the_utterance_alone_bit_for_bit(kernel_case, out):
    c = kernel_case
    M = KB * KN
    g = torch.Generator().manual_seed(92)
    dop = ops.split(torch.randn(M, KA, generator=g).to(DEV), precision=3)
    _nan_rows(dop, KLENS)
    _, lse = _train_fwd(c["q"], c["k"], c["vt"], KB, KN, 3, lens=c["kl"])       # the real statistic on the rows before a length
    delta = (0.1 * torch.randn(KB, KH, KN, generator=g)).to(DEV)
    for b, n in enumerate(KLENS):
        lse[b, :, n:] = NAN
        delta[b, :, n:] = NAN
    bk = HipBackend(4 if out == "planes4" else 3)

    def run(q, k, v, do, ls, dl, B, N, lens):
        rows = B * N
        kw = {} if lens is None else dict(lens=lens)
        if out == "f32":
            dq, dkv = torch.full((rows, KA), NAN, device=DEV), torch.full((rows, 2 * KA), NAN, device=DEV)
            bk.attention_bwd(q, 0, k, 0, v, 0, do, ls, dl, B, KH, N, N, dq=(dq, 0), dkv=(dkv, 0, KA), **kw)
            return torch.cat((dq, dkv), dim=1).view(torch.int32)
        gp = bk.new_planes(rows, 3 * KA)
        gp.buf.fill_(NAN)
        bk.attention_bwd(q, 0, k, 0, v, 0, do, ls, dl, B, KH, N, N, planes=(gp, 0, KA, 2 * KA), **kw)
        return _bits(gp.buf)

    got = run(c["q"], c["k"], c["v"], dop, lse, delta, KB, KN, c["kl"])
    torch.cuda.synchronize()
    for b, n in enumerate(KLENS):
        r0 = b * KN
        solo = run(_rows(c["q"], r0, n), _rows(c["k"], r0, n), _rows(c["v"], r0, n), _rows(dop, r0, n), lse[b:b + 1, :, :n].contiguous(),
                   delta[b:b + 1, :, :n].contiguous(), 1, n, None)                # the call that exists, alone at Nq = Nk = len
        assert torch.equal(got[r0:r0 + n], solo), f"dq | dk | dv of utterance {b} (length {n})"
        assert torch.count_nonzero(got[r0 + n:r0 + KN]) == 0, f"gradient rows beyond length {n} must be zero bits"


# ------------------------------------------------------------------------------------------------ 3, 4. the model
MB, MN, MLENS = 4, 256, [256, 193, 64, 7]
CFG = {"uncond": dict(dim=64, depth=2), "cond": dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}
# Batch against solo on the HIP path: output rows and every parameter gradient (the sum of the four solo gradients), worst tensor,
# relative Frobenius error.  The yardstick is the same comparison with no lengths anywhere -- the equal-length batch [4, 256, 64] through
# the existing pass against its four utterances alone, the reduction-order effect of the GEMMs (split-K plans, wgrad slices and, in the
# mixed arithmetic, the loss scale follow the token count) -- per configuration and precision, measured on the MI355X on the kernels
# before this feature (profiles/ragged_training.json "gpu_batch_vs_solo").  The bound is twice the yardstick.
YARDSTICK = {("uncond", "exact"): 1.09e-7, ("uncond", "mixed"): 8.51e-6, ("cond", "exact"): 1.17e-7, ("cond", "mixed"): 9.40e-6}


def _model(name, tprec, **kw):
    m = Model(**CFG[name], **kw)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    return m


def _inputs(name):
    mk = lambda nm, shape, seed, **k: make_input(nm, shape, seed=seed, **k).to(DEV)      # noqa: E731
    x, t, cot = mk("x", (MB, MN, 64), 2), mk("times", (MB,), 2, uniform=True), mk("gw", (MB, MN, 64), 3)
    prompt = cond = None
    if CFG[name].get("condition_on_prompt"):
        prompt, cond = mk("prompt", (MB, 7, 48), 2), mk("cond", (MB, 48, MN), 2)
    return x, t, prompt, cond, cot


def _run(m, fwd, x, t, prompt, cond, cot):
    for p in m.parameters():
        p.grad = None
    kw = {} if prompt is None else dict(prompt=prompt, cond=cond, cond_drop_prob=0.)
    y = fwd(x, t, **kw)
    (y * cot).sum().backward()
    return y.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _solo_sum(m, x, t, prompt, cond, cot, lens):
    """every utterance alone at its own length through the existing pass -> (outputs, the sum of their gradients)"""
    outs, total = [], None
    for i, n in enumerate(lens):
        y, g = _run(m, lambda xs, ts, **kw: m(xs, ts, **kw), x[i:i + 1, :n].contiguous(), t[i:i + 1], None if prompt is None else prompt[i:i + 1],
                    None if cond is None else cond[i:i + 1, :, :n].contiguous(), cot[i:i + 1, :n].contiguous())
        outs.append(y)
        total = g if total is None else {k: (v if g[k] is None else (g[k] if v is None else v + g[k])) for k, v in total.items()}
    return outs, total


def _worst(y, g, outs, total, lens):
    worst = ("", 0.0)
    for i, n in enumerate(lens):
        worst = max(worst, (f"out[{i}]", rel(y[i:i + 1, :n], outs[i])), key=lambda z: z[1])
    for k, ref in total.items():
        if ref is None or ref.norm() == 0:
            assert g[k] is None or g[k].norm() == 0, k
            continue
        worst = max(worst, (k, rel(g[k], ref)), key=lambda z: z[1])
    return worst


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
def test_full_lengths_change_nothing(tprec):
    m = _model("uncond", tprec, ragged_training=True)
    x, t, _, _, cot = _inputs("uncond")
    y0, g0 = _run(m, lambda xs, ts: m(xs, ts), x, t, None, None, cot)
    for lens in ([MN] * MB, torch.full((MB,), MN, dtype=torch.int32, device=DEV)):
        y, g = _run(m, lambda xs, ts: m(xs, ts, lens=lens), x, t, None, None, cot)
        assert torch.equal(y, y0)
        for k, v in g0.items():
            assert (v is None and g[k] is None) or torch.equal(g[k], v), k


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
@pytest.mark.parametrize("name", sorted(CFG))
def test_ragged_batch_against_the_utterances_alone_on_the_hip_path(name, tprec):
    m = _model(name, tprec, ragged_training=True)
    x, t, prompt, cond, cot = _inputs(name)
    # the yardstick, re-measured here: an equal-length batch against its utterances alone, the existing pass, no lengths anywhere
    outs, total = _solo_sum(m, x, t, prompt, cond, cot, [MN] * MB)
    y, g = _run(m, lambda xs, ts, **kw: m(xs, ts, **kw), x, t, prompt, cond, cot)
    who_y, yard = _worst(y, g, outs, total, [MN] * MB)
    # the ragged batch, NaN beyond the lengths, against its utterances alone at n = len through the existing pass
    outs, total = _solo_sum(m, x, t, prompt, cond, cot, MLENS)
    xn, condn = x.clone(), None if cond is None else cond.clone()
    for i, n in enumerate(MLENS):
        xn[i, n:] = NAN
        if condn is not None:
            condn[i, :, n:] = NAN
    lens = torch.tensor(MLENS, dtype=torch.int32, device=DEV)
    y, g = _run(m, lambda xs, ts, **kw: m(xs, ts, lens=lens, **kw), xn, t, prompt, condn, cot)
    assert torch.isfinite(y).all() and all(torch.count_nonzero(y[i, n:]) == 0 for i, n in enumerate(MLENS))
    assert all(v is None or torch.isfinite(v).all() for v in g.values())
    who, e = _worst(y, g, outs, total, MLENS)
    bound = 2 * YARDSTICK[(name, tprec)]
    _record(f"gpu_batch_vs_solo/{name}_{tprec}", dict(yardstick_equal_length=yard, yardstick_tensor=who_y, ragged=e, ragged_tensor=who,
                                                      yardstick_recorded=YARDSTICK[(name, tprec)], bound=bound))
    # ... and within the project's 1e-3 per tensor of the composite's autograd with the same lengths (fp32 torch ops on the same GPU)
    yc, gc = _run(m, lambda xs, ts, **kw: model_forward_autograd_ragged(m, xs, ts, lens, **kw), xn, t, prompt, condn, cot)
    errs = {k: rel(g[k], v) for k, v in gc.items() if v is not None and v.norm() > 0}
    worst_c = max(errs.items(), key=lambda kv: kv[1])
    _record(f"gpu_vs_composite/{name}_{tprec}", dict(out_rel=rel(y, yc), worst_param=worst_c[0], worst_rel=worst_c[1]))
    assert e <= bound, (who, e, bound)
    assert rel(y, yc) < 1e-4 and worst_c[1] < 1e-3, (rel(y, yc), worst_c)


# ------------------------------------------------------------------------------------------------ 5, 6. the captured step and the Trainer
def _diffusion(tprec, seed=71):
    m = Model(dim=64, depth=1, ragged_training=True)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    return m, NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2).to(DEV)


def _batch(s, b=2, n=96):
    mk = lambda name, shape, **k: make_input(name, shape, seed=s, **k).to(DEV)    # noqa: E731
    return mk("audio", (b, n, 64)), mk("times", (b,), uniform=True), mk("noise", (b, n, 64))


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
def test_graphed_train_step_follows_lengths_rewritten_between_replays(tprec):
    m, d = _diffusion(tprec)
    a, t, z = _batch(80)
    captured, other = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([96, 40], [33, 96]))
    step = training.GraphedTrainStep(lambda au, ln, ts, no: d(au, audio_lens=ln, times=ts, noise=no), (a, captured, t, z), m)
    for lens in (other, captured):
        loss = step(a, lens, t, z).detach().clone()
        grads = [None if gr is None else gr.detach().clone() for gr in step.grads]
        for p in m.parameters():
            p.grad = None
        loss_e = d(a, audio_lens=lens, times=t, noise=z)
        loss_e.backward()
        assert torch.isfinite(loss) and torch.equal(loss, loss_e.detach())
        for p, gr in zip(step.params, grads):
            assert (gr is None and p.grad is None) or torch.equal(gr, p.grad)
    l_other = float(step(a, other, t, z))
    assert l_other != float(step(a, captured, t, z))        # the lengths do reach the loss


def test_trainer_takes_dict_batches_with_audio_lens(tmp_path):
    """dict batches reach forward as keywords and the graph copies integer inputs like any other.  times / noise travel in the batch so that
    the captured Trainer and the eager one see the same draws (the graph's warm passes would otherwise advance the generator)"""
    def batches():
        out = []
        for s, lens in ((84, [96, 51]), (85, [17, 96])):
            a, t, z = _batch(s)
            out.append({"audio": a, "audio_lens": torch.tensor(lens, dtype=torch.int32, device=DEV), "times": t, "noise": z})
        return out

    losses = {}
    for use_graph in (True, False):
        _, d = _diffusion("exact", seed=5)
        tr = Trainer(d, dataloader=batches(), train_lr=1e-3, train_num_steps=2, use_ema=False, save_and_sample_every=0,
                     results_folder=tmp_path / f"run{int(use_graph)}", use_graph=use_graph)
        got = []
        for _ in range(2):
            tr.train_step()
            got.append(float(tr.last_loss))
        assert (tr._graph is not None) == use_graph and int(tr.opt.steps_taken) == 2 and int(tr.opt.skipped) == 0
        losses[use_graph] = got
    assert all(l == l and abs(l) != float("inf") for l in losses[True]) and losses[True] == losses[False], losses
    # the two keys alone (times and noise drawn inside the captured step): finite
    _, d = _diffusion("exact", seed=5)
    data = [{k: v for k, v in b.items() if k in ("audio", "audio_lens")} for b in batches()]
    tr = Trainer(d, dataloader=data, train_lr=1e-3, train_num_steps=2, use_ema=False, save_and_sample_every=0, results_folder=tmp_path / "run2")
    for _ in range(2):
        tr.train_step()
        assert bool(torch.isfinite(tr.last_loss))
    assert tr._graph is not None
