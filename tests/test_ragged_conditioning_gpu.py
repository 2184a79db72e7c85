"""Ragged text and prompts in TRAINING on the MI355X (include/ns2hip_train.h): per-utterance lengths through the conditioning.
The definition under test is the one of the ragged front-end, now for the gradients too: utterance i of a padded batch is utterance i run
alone with its text cut to text_lens[i] and its prompt cut to prompt_lens[i] -- what lies at or beyond a length (NaN included) reaches no
value and no gradient before it, and what is returned there is an exact 0.

  1. the kernel: GroupNorm + SiLU backward with a row count per utterance (ns2_groupnorm_silu_bwd_lens), bit for bit against the entry that
     exists on the utterance alone;
  2. the passes (`ragged_conditioning=True`): SpeechPromptEncoder, DurationPitchPredictor, Model(prompt_lens=) -- padding does not matter
     (bit for bit), the batch equals its utterances alone (within twice the re-measured equal-length yardstick), agreement with the
     composite, full lengths change nothing, and the HIP path really ran;
  3. the wrapper: NaturalSpeech2.forward(text_lens=, prompt_lens=, audio_lens=), GraphedTrainStep, Trainer."""
import gc
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import _lib, training  # noqa: E402
from tests.golden.gen import make_input  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
HB = training.HipBackend()


def _record(key, value):
    """one measured figure: printed, and merged into $NS2_RECORD_DIR/ragged_conditioning_tests.json when that is set (what
    profiles/ragged_conditioning.json quotes)"""
    print(f"{key}: {value}")
    if not os.environ.get("NS2_RECORD_DIR"):
        return
    path = os.path.join(os.environ["NS2_RECORD_DIR"], "ragged_conditioning_tests.json")
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


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (5, 130, 512): cg = 64 -> statistics chunks of 64 rows, column-sum chunks of 32 rows: a full utterance, a ragged chunk, exactly one
# statistics chunk, one column-sum chunk plus a row, a single row.  (3, 600, 64): cg = 8 -> statistics chunks of 512 rows: one row into the
# second chunk, exactly one chunk.  (2, 1, 32): n = 1.
GN_CASES = [((5, 130, 512), [130, 97, 64, 33, 1]), ((3, 600, 64), [600, 513, 512]), ((2, 1, 32), [1, 1])]
GROUPS, EPS = 8, 1e-5


def _gn_operands(B, n, C, lens, with_resid, nan=True):
    x = make_input("gn_x", (B, n, C), seed=301).to(DEV)
    dy = make_input("gn_dy", (B, n, C), seed=302).to(DEV)
    resid = make_input("gn_resid", (B, n, C), seed=303).to(DEV) if with_resid else None
    gamma = (1.0 + 0.3 * make_input("gn_gamma", (C,), seed=304)).to(DEV)
    beta = (0.3 * make_input("gn_beta", (C,), seed=305)).to(DEV)
    if nan:
        for b, l in enumerate(lens):
            for t in (x, dy, resid):
                if t is not None:
                    t[b, l:] = NAN
    return x, dy, resid, gamma, beta


def _gn_run(x, dy, resid, gamma, beta, B, n, lens=None):
    """forward + backward through the backend: with `lens` the two entries with lengths, without the entries that exist"""
    C = x.shape[-1]
    kw = {} if lens is None else dict(row_lens=lens)
    y, rows, stats = HB.groupnorm_silu_fwd(x.reshape(B * n, C), B, n, gamma, beta, GROUPS, EPS,
                                           resid=None if resid is None else resid.reshape(B * n, C), **kw)
    dx, dw, db = HB.groupnorm_silu_bwd(dy.reshape(B * n, C), rows, stats, B, n, gamma, beta, GROUPS, EPS, **kw)
    return y.reshape(B, n, C), dx.reshape(B, n, C), dw.clone(), db.clone()


@pytest.mark.parametrize("with_resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("shape,lens", GN_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _ in GN_CASES])
def test_groupnorm_silu_backward_with_lengths(shape, lens, with_resid):
    B, n, C = shape
    x, dy, resid, gamma, beta = _gn_operands(B, n, C, lens, with_resid)
    y, dx, dw, db = _gn_run(x, dy, resid, gamma, beta, B, n, _i32(lens))
    y2, dx2, dw2, db2 = _gn_run(x, dy, resid, gamma, beta, B, n, _i32(lens))
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in (y, dx, dw, db)), "NaN behind a length reached a result"
    assert _same_bits(dx, dx2) and _same_bits(dw, dw2) and _same_bits(db, db2), "two runs differ"
    refs = {k: torch.zeros(C, dtype=torch.float64, device=DEV) for k in ("dw64", "db64", "dw32", "db32")}
    for b, l in enumerate(lens):
        cut = lambda t: None if t is None else t[b:b + 1, :l].contiguous()                # noqa: E731
        ys, dxs, dws, dbs = _gn_run(cut(x), cut(dy), cut(resid), gamma, beta, 1, l)       # the entries that exist, the utterance alone
        assert _same_bits(y[b, :l], ys[0]), f"y of utterance {b} (length {l})"
        assert _same_bits(dx[b, :l], dxs[0]), f"dx of utterance {b} (length {l})"
        assert torch.count_nonzero(dx[b, l:].contiguous().view(torch.int32)) == 0, f"dx rows beyond length {l} must be zero bits"
        assert torch.count_nonzero(y[b, l:].contiguous().view(torch.int32)) == 0
        for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):                    # fp64 / fp32 torch autograd, the utterance alone
            xx, g, bb = (t.detach().to(dt).clone().requires_grad_(True) for t in (cut(x), gamma, beta))
            yy = F.silu(F.group_norm(xx.transpose(1, 2), GROUPS, g, bb, EPS)).transpose(1, 2)
            (yy * cut(dy).to(dt)).sum().backward()
            refs["dw" + tag] += g.grad.double()
            refs["db" + tag] += bb.grad.double()
    res = {}
    for k, got in (("dw", dw), ("db", db)):
        e_hip, e_torch = rel(got, refs[k + "64"]), rel(refs[k + "32"], refs[k + "64"])
        res[k] = dict(hip=e_hip, torch_fp32=e_torch)
        assert e_hip < max(1e-5, 4 * e_torch), (k, res[k])
    _record(f"kernel/groupnorm_bwd_lens/{B}x{n}x{C}/{'resid' if with_resid else 'plain'}", res)


def test_groupnorm_silu_backward_with_lengths_batch_of_one_is_the_existing_entry():
    """dweight | dbias of a batch of one, bit for bit (dx: the test above)"""
    n, C, l = 130, 512, 97
    x, dy, _, gamma, beta = _gn_operands(1, n, C, [l], False)
    _, _, dw, db = _gn_run(x, dy, None, gamma, beta, 1, n, _i32([l]))
    _, _, dws, dbs = _gn_run(x[:, :l].contiguous(), dy[:, :l].contiguous(), None, gamma, beta, 1, l)
    assert _same_bits(dw, dws) and _same_bits(db, dbs)


def test_groupnorm_silu_backward_clamps_lengths_and_null_lengths_are_the_existing_entry():
    B, n, C = 3, 130, 512
    x, dy, resid, gamma, beta = _gn_operands(B, n, C, [n] * B, True, nan=False)
    a = _gn_run(x, dy, resid, gamma, beta, B, n, _i32([0, 9999, 70]))
    b = _gn_run(x, dy, resid, gamma, beta, B, n, _i32([1, n, 70]))
    assert all(_same_bits(p, q) for p, q in zip(a, b)) and all(torch.isfinite(t).all() for t in a)
    # row_lens = NULL through the new entry: the launches of the entry that exists
    lib = HB.lib
    y, rows, stats = HB.groupnorm_silu_fwd(x.reshape(B * n, C), B, n, gamma, beta, GROUPS, EPS)
    dyr = dy.reshape(B * n, C)
    dx0, dw0, db0 = HB.groupnorm_silu_bwd(dyr, rows, stats, B, n, gamma, beta, GROUPS, EPS)
    dx, dwb = torch.empty_like(dx0), torch.empty(2 * C, device=DEV)
    nbytes = lib.ns2_groupnorm_silu_bwd_workspace_bytes(B, n, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def entry(dy_p=dyr.data_ptr(), x_p=rows.data_ptr(), st_p=stats.data_ptr(), lens_p=None, dx_p=dx.data_ptr(), dwb_p=dwb.data_ptr(),
              ws_p=ws.data_ptr(), ws_bytes=nbytes, st_bytes=stats.numel()):
        return lib.ns2_groupnorm_silu_bwd_lens(dy_p, C, x_p, B, n, C, GROUPS, gamma.data_ptr(), beta.data_ptr(), EPS, st_p, st_bytes, lens_p, dx_p,
                                               dwb_p, ws_p, ws_bytes, stream)
    assert entry() == _lib.NS2_OK
    assert _same_bits(dx, dx0) and _same_bits(dwb[:C], dw0) and _same_bits(dwb[C:], db0)
    # refused before any device call: null pointers, a workspace or a statistics buffer too small -- with and without lengths
    lens = _i32([n, 70, 1])
    for lp in (None, lens.data_ptr()):
        for bad in (dict(dy_p=None), dict(x_p=None), dict(st_p=None), dict(dx_p=None), dict(dwb_p=None), dict(ws_p=None),
                    dict(ws_bytes=nbytes - 1), dict(st_bytes=stats.numel() - 1)):
            assert entry(lens_p=lp, **bad) == _lib.NS2_ERR_ARG, bad
    assert "ns2_groupnorm_silu_bwd" in lib.ns2_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the passes
from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, NaturalSpeech2, SpeechPromptEncoder  # noqa: E402
from naturalspeech2_pytorch_amd import autograd_path  # noqa: E402
from tests.golden.gen import make_weights  # noqa: E402

PB, PN = 4, 24                                             # b, n = n_p
TEXT_LENS, PROMPT_LENS = [24, 13, 9, 1], [24, 10, 4, 1]    # prompt lengths 4 and 1 lie inside the k = 9 convolutions' padding of 4
OUT_TOL, GRAD_TOL = 1e-4, 1e-3
# Batch against the utterances alone, worst tensor (output rows per utterance, every parameter gradient as the sum of the solo gradients),
# relative Frobenius error.  The yardstick is that comparison with no lengths anywhere -- the equal-length batch through the pass that
# exists against its utterances alone: accumulation order across the batch in the weight-gradient GEMMs -- re-measured in the test and
# recorded on the MI355X (profiles/ragged_conditioning.json "tests").  The bound on the ragged batch is twice the recorded yardstick.
YARDSTICK = {"prompt_enc": 1.51e-7, "predictor_resnet": 5.25e-7, "predictor_convblock_k5": 1.65e-7, "predictor_resnet_tokens": 1.67e-7,
             "model_exact_full": 2.01e-7, "model_exact_lens": 2.01e-7, "model_mixed_full": 1.99e-7, "model_mixed_lens": 1.99e-7}


def _mk(name, shape, seed, **k):
    return make_input(name, shape, seed=seed, **k).to(DEV)


def _load(m, seed):
    gc.collect()                                           # (modules of earlier cases: their entries leave the backend's pack cache now, not mid-pass)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    return m.to(DEV).train()


def _pad(t, lens, value, dim=1):
    """a copy of t [b, n, ...] (dim = 1) or [b, ..., n] (dim = -1) with `value` at or beyond each length"""
    t = t.clone()
    for i, l in enumerate(lens):
        if dim == 1:
            t[i, l:] = value
        else:
            t[i, ..., l:] = value
    return t


class Subject:
    """one module under test: `call(m, inputs, lens)` -> tuple of outputs; inputs = dict of tensors; lens = dict of length lists / tensors
    or None (the pass that exists); `cut(inputs, i)` -> the inputs of utterance i alone, cut to its lengths; `composite(m, inputs, lens)`"""
    out_lens = None          # per output: the lengths its rows are cut to (None: not cut)

    def grads(self, m, fn, inputs, cots):
        for p in m.parameters():
            p.grad = None
        outs = fn(m, inputs)
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        return [o.detach().clone() for o in outs], {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


class PromptEnc(Subject):
    name = "prompt_enc"

    def build(self, switch=True, dropout=0.):
        return _load(SpeechPromptEncoder(dim_codebook=32, dims=(64, 96, 64), depth=2, heads=2, dim_head=64, dropout=dropout, train_backend="hip",
                                         ragged_conditioning=switch), 85)

    def inputs(self):
        return dict(x=_mk("x", (PB, PN, 32), 86)), [_mk("proj", (PB, PN, 64), 87)]

    lens = dict(lens=PROMPT_LENS)
    pads = dict(x=PROMPT_LENS)
    out_lens = [PROMPT_LENS]

    def call(self, m, inp, lens):
        return (m(inp["x"], **({} if lens is None else dict(lens=lens["lens"]))),)

    def composite(self, m, inp, lens):
        return (autograd_path.speech_prompt_encoder_autograd(m, inp["x"], lens=lens["lens"]),)

    def cut(self, inp, i, lens):
        return dict(x=inp["x"][i:i + 1, :lens["lens"][i]].contiguous())

    def set_seed(self, m, seed):
        m.transformer.dropout_seed = seed

    patch = "speech_prompt_encoder_autograd"


class Predictor(Subject):
    def __init__(self, name, ids=False, **kw):
        self.name, self.ids, self.kw = f"predictor_{name}", ids, kw

    def build(self, switch=True, dropout=0.):
        kw = dict(dim=64, dim_hidden=64, heads=2, dim_head=64, depth=2, dropout=dropout)
        kw.update(self.kw)
        return _load(DurationPitchPredictor(**kw, train_backend="hip", ragged_conditioning=switch), 91)

    def inputs(self):
        if self.ids:
            x = torch.randint(0, 40, (PB, PN), generator=torch.Generator().manual_seed(92)).to(DEV)
        else:
            x = _mk("phoneme_enc", (PB, PN, 64), 92)
        return dict(x=x, pr=_mk("prompt_enc", (PB, PN, 64), 93)), [_mk("proj0", (PB, PN), 94), _mk("proj1", (PB, PN), 95)]

    lens = dict(text_lens=TEXT_LENS, prompt_lens=PROMPT_LENS)
    pads = dict(x=TEXT_LENS, pr=PROMPT_LENS)
    out_lens = [TEXT_LENS, TEXT_LENS]

    def call(self, m, inp, lens):
        return m(inp["x"], inp["pr"], **(lens or {}))

    def composite(self, m, inp, lens):
        return autograd_path.duration_pitch_autograd(m, inp["x"], inp["pr"], **lens)

    def cut(self, inp, i, lens):
        return dict(x=inp["x"][i:i + 1, :lens["text_lens"][i]].contiguous(), pr=inp["pr"][i:i + 1, :lens["prompt_lens"][i]].contiguous())

    def set_seed(self, m, seed):
        m.dropout_seed = seed

    patch = "duration_pitch_autograd"


MN, MLENS = 32, [32, 19, 8, 3]


class Denoiser(Subject):
    def __init__(self, tprec, with_lens):
        self.name, self.tprec, self.with_lens = f"model_{tprec}_{'lens' if with_lens else 'full'}", tprec, with_lens
        self.lens = dict(prompt_lens=PROMPT_LENS, **(dict(lens=MLENS) if with_lens else {}))
        self.pads = dict(prompt=PROMPT_LENS, **(dict(x=MLENS) if with_lens else {}))
        self.out_lens = [MLENS if with_lens else None]

    def build(self, switch=True, dropout=0.):
        m = _load(Model(dim=64, depth=1, dim_prompt=48, condition_on_prompt=True, num_latents_m=16, ragged_training=True, ragged_conditioning=switch), 1)
        m.train_backend, m.train_precision = "hip", self.tprec
        return m

    def inputs(self):
        return (dict(x=_mk("x", (PB, MN, 64), 2), t=_mk("times", (PB,), 2, uniform=True), prompt=_mk("prompt", (PB, PN, 48), 2),
                     cond=_mk("cond", (PB, 48, MN), 2)), [_mk("gw", (PB, MN, 64), 3)])

    def call(self, m, inp, lens):
        return (m(inp["x"], inp["t"], prompt=inp["prompt"], cond=inp["cond"], cond_drop_prob=0., **(lens or {})),)

    def composite(self, m, inp, lens):
        kw = dict(prompt=inp["prompt"], cond=inp["cond"], cond_drop_prob=0., prompt_lens=lens["prompt_lens"])
        if "lens" in lens:
            return (autograd_path.model_forward_autograd_ragged(m, inp["x"], inp["t"], lens["lens"], **kw),)
        return (autograd_path.model_forward_autograd(m, inp["x"], inp["t"], **kw),)

    def cut(self, inp, i, lens):
        n = lens["lens"][i] if "lens" in lens else MN
        return dict(x=inp["x"][i:i + 1, :n].contiguous(), t=inp["t"][i:i + 1], prompt=inp["prompt"][i:i + 1, :lens["prompt_lens"][i]].contiguous(),
                    cond=inp["cond"][i:i + 1, :, :n].contiguous())

    patch = None


SUBJECTS = [PromptEnc(), Predictor("resnet"), Predictor("convblock_k5", use_resnet_block=False, kernel_size=5, depth=1),
            Predictor("resnet_tokens", ids=True, num_phoneme_tokens=40, depth=1, num_convolutions_per_block=1),
            Denoiser("exact", False), Denoiser("exact", True), Denoiser("mixed", False), Denoiser("mixed", True)]
IDS = [s.name for s in SUBJECTS]


def _padded(s, inp, value):
    """the inputs with `value` at or beyond the lengths (ids: another valid id; cond follows the frames of x)"""
    out = dict(inp)
    for k, lens in s.pads.items():
        if inp[k].is_floating_point():
            out[k] = _pad(inp[k], lens, value)
        else:
            out[k] = _pad(inp[k], lens, 7 if value != value else 3)
    if "cond" in inp and "x" in s.pads:
        out["cond"] = _pad(inp["cond"], s.pads["x"], value, dim=-1)
    return out


def _dev_lens(lens):
    return {k: _i32(v) for k, v in lens.items()}


def _assert_same(a, b):
    (oa, ga), (ob, gb) = a, b
    assert all(_same_bits(x, y) for x, y in zip(oa, ob)), "outputs differ"
    for k, v in ga.items():
        assert (v is None and gb[k] is None) or _same_bits(v, gb[k]), k


@pytest.fixture()
def no_composite(monkeypatch):
    """a silent fall-back to the PyTorch composite fails the test"""
    def refuse(*a, **k):
        raise AssertionError("the PyTorch composite was entered: the HIP training path did not run")
    for name in ("speech_prompt_encoder_autograd", "duration_pitch_autograd", "model_forward_autograd", "model_forward_autograd_ragged"):
        monkeypatch.setattr(autograd_path, name, refuse)


@pytest.mark.parametrize("s", SUBJECTS, ids=IDS)
def test_padding_does_not_matter_bit_for_bit(no_composite, s):
    inp, cots = s.inputs()
    lens = _dev_lens(s.lens)
    for dropout in ((0., 0.3) if hasattr(s, "set_seed") else (0.,)):
        m = s.build(dropout=dropout)
        if dropout:
            s.set_seed(m, torch.tensor([1234], dtype=torch.int64, device=DEV))
        a = s.grads(m, lambda mm, ii: s.call(mm, ii, lens), _padded(s, inp, NAN), cots)
        b = s.grads(m, lambda mm, ii: s.call(mm, ii, lens), _padded(s, inp, 2.5), cots)
        assert all(torch.isfinite(o).all() for o in a[0]) and all(v is None or torch.isfinite(v).all() for v in a[1].values())
        _assert_same(a, b)
        for o, ol in zip(a[0], s.out_lens):
            if ol is not None:
                assert all(torch.count_nonzero(o[i, l:]) == 0 for i, l in enumerate(ol)), "returned rows at or beyond a length must be exact 0"
        if dropout:                                        # the dropout did act
            assert not _same_bits(a[0][0], s.grads(s.build(), lambda mm, ii: s.call(mm, ii, lens), inp, cots)[0][0])


def _solo_sum(s, m, inp, cots, lens):
    """every utterance alone, cut to its lengths, through the pass that exists (no lengths) -> (outputs per utterance, the sum of the gradients)"""
    outs, total = [], None
    for i in range(PB):
        cc = [c[i:i + 1] if ol is None else c[i:i + 1, :ol[i]].contiguous() for c, ol in zip(cots, lens["out"])]
        o, g = s.grads(m, lambda mm, ii: s.call(mm, ii, None), s.cut(inp, i, lens["in"]), cc)
        outs.append(o)
        total = g if total is None else {k: (v if g[k] is None else (g[k] if v is None else v + g[k])) for k, v in total.items()}
    return outs, total


def _worst(got, outs, total, out_lens):
    y, g = got
    worst = ("", 0.0)
    for i in range(PB):
        for j, ol in enumerate(out_lens):
            yi = y[j][i:i + 1] if ol is None else y[j][i:i + 1, :ol[i]]
            if outs[i][j].norm() > 0:
                worst = max(worst, (f"out{j}[{i}]", rel(yi, outs[i][j])), key=lambda z: z[1])
            else:
                assert yi.norm() == 0
    for k, ref in total.items():
        if ref is None or ref.norm() == 0:
            assert g[k] is None or g[k].norm() == 0, k
            continue
        worst = max(worst, (k, rel(g[k], ref)), key=lambda z: z[1])
    return worst


@pytest.mark.parametrize("s", SUBJECTS, ids=IDS)
def test_ragged_batch_against_the_utterances_alone(no_composite, s):
    """the ragged batch, NaN behind every length, against its utterances alone on the pass that exists, within twice the equal-length
    yardstick.  Two things this rests on: at dropout 0 the backward of a key-mask attention runs the plain backward kernel over
    zero rows (the key-mask backward instantiation gives other last bits than the plain one: the `Transformer` that exists, all-ones mask=
    against no mask, has bit-equal outputs and gradients 3.9e-6 apart), and the predictor orders its context rows as they are alone."""
    inp, cots = s.inputs()
    m = s.build()
    # the yardstick, re-measured: the equal-length batch against its utterances alone on the pass that exists, no lengths anywhere
    full = {k: [PN if k != "lens" else MN] * PB for k in s.lens}
    full_out = [None if ol is None else [c.shape[1]] * PB for ol, c in zip(s.out_lens, cots)]
    outs, total = _solo_sum(s, m, inp, cots, dict({"in": full}, out=full_out))
    who_y, yard = _worst(s.grads(m, lambda mm, ii: s.call(mm, ii, None), inp, cots), outs, total, full_out)
    # the ragged batch, NaN behind the lengths, against its utterances alone cut to their lengths
    outs, total = _solo_sum(s, m, inp, cots, dict({"in": s.lens}, out=s.out_lens))
    lens = _dev_lens(s.lens)
    ragged = s.grads(m, lambda mm, ii: s.call(mm, ii, lens), _padded(s, inp, NAN), cots)
    who, e = _worst(ragged, outs, total, s.out_lens)
    _record(f"tests/batch_vs_solo/{s.name}", dict(yardstick_equal_length=yard, yardstick_tensor=who_y, ragged=e, ragged_tensor=who,
                                                  yardstick_recorded=YARDSTICK.get(s.name), bound=2 * YARDSTICK.get(s.name, float("nan"))))
    assert e <= 2 * YARDSTICK[s.name], (who, e, YARDSTICK[s.name])


@pytest.mark.parametrize("s", SUBJECTS, ids=IDS)
def test_agreement_with_the_composite_and_full_lengths_change_nothing(s):
    inp, cots = s.inputs()
    m = s.build()
    lens = _dev_lens(s.lens)
    padded = _padded(s, inp, NAN)
    (y, g), (yc, gc) = s.grads(m, lambda mm, ii: s.call(mm, ii, lens), padded, cots), s.grads(m, lambda mm, ii: s.composite(mm, ii, lens), padded, cots)
    errs = {k: rel(g[k], v) for k, v in gc.items() if v is not None and v.norm() > 0}
    worst = max(errs.items(), key=lambda kv: kv[1])
    out_rel = max(rel(a, b) for a, b in zip(y, yc))
    _record(f"tests/vs_composite/{s.name}", dict(out_rel=out_rel, worst_param=worst[0], worst_rel=worst[1]))
    assert out_rel < OUT_TOL and worst[1] < GRAD_TOL, (out_rel, worst)
    # full lengths through the switch: the pass without lengths, bit for bit.  Lengths the host can see (a list, a CPU tensor) take the call
    # without lengths; a device tensor is never read on the host and runs the length path -- the key-mask forward kernel, whose all-ones mask
    # gives the plain kernel's bits, and at dropout 0 the plain backward the pass without lengths runs -- to the same bits.
    plain = s.grads(m, lambda mm, ii: s.call(mm, ii, None), inp, cots)
    full = {k: [PN if k != "lens" else MN] * PB for k in s.lens}
    for fl in (full, {k: torch.tensor(v) for k, v in full.items()}, _dev_lens(full)):
        _assert_same(s.grads(m, lambda mm, ii: s.call(mm, ii, fl), inp, cots), plain)
    # ... and without the switch the lengths raise under autograd, as before
    with pytest.raises(NotImplementedError):
        off = s.build(switch=False)
        s.call(off, inp, {k: v for k, v in lens.items() if k != "lens" or not isinstance(s, Denoiser)})      # (Model: lens= is ragged_training's)


def test_the_hip_path_really_ran(no_composite, monkeypatch):
    counts = {}

    def counted(name):
        real = getattr(training.HipBackend, name)

        def f(self, *a, **k):
            counts[name] = counts.get(name, 0) + 1
            if name in ("groupnorm_silu_fwd", "groupnorm_silu_bwd") and k.get("row_lens") is not None:
                counts[name + ":row_lens"] = counts.get(name + ":row_lens", 0) + 1
            if name in ("attention", "attention_bwd") and k.get("lens") is not None:
                counts[name + ":lens"] = counts.get(name + ":lens", 0) + 1
            return real(self, *a, **k)
        monkeypatch.setattr(training.HipBackend, name, f)
    for name in ("groupnorm_silu_fwd", "groupnorm_silu_bwd", "attention", "attention_masked", "attention_bwd", "attention_bwd_masked", "keep_rows"):
        counted(name)
    for s in SUBJECTS[:4]:
        counts.clear()
        inp, cots = s.inputs()
        m = s.build()
        s.grads(m, lambda mm, ii: s.call(mm, ii, _dev_lens(s.lens)), _padded(s, inp, NAN), cots)
        print(s.name, counts)
        # (dropout 0: the forward on the key-mask kernel, the backward on the plain one -- what the utterance alone runs -- over zero rows)
        assert counts["attention_masked"] > 0 and counts["attention_bwd"] == counts["attention_masked"], (s.name, counts)
        assert counts.get("attention_bwd_masked", 0) == 0
        assert counts.get("attention", 0) == 0 and counts.get("attention:lens", 0) == 0 and counts.get("attention_bwd:lens", 0) == 0, (s.name, counts)
        m = s.build(dropout=0.3)                           # ... with dropout both directions run the key-mask / dropout kernels
        counts.clear()
        s.grads(m, lambda mm, ii: s.call(mm, ii, _dev_lens(s.lens)), _padded(s, inp, NAN), cots)
        assert counts["attention_masked"] > 0 and counts["attention_bwd_masked"] == counts["attention_masked"], (s.name, counts)
        assert counts["keep_rows"] > 0
        if s.name in ("predictor_resnet", "predictor_resnet_tokens"):
            n_gn = counts["groupnorm_silu_fwd"]
            assert n_gn > 0 and counts["groupnorm_silu_fwd:row_lens"] == n_gn and counts["groupnorm_silu_bwd:row_lens"] == n_gn, counts
        else:
            assert counts.get("groupnorm_silu_fwd", 0) == 0
    for s in SUBJECTS[4:]:                                 # Model: the resampler's attentions under the key mask; lens= stays with the self-attention
        counts.clear()
        inp, cots = s.inputs()
        m = s.build()
        s.grads(m, lambda mm, ii: s.call(mm, ii, _dev_lens(s.lens)), _padded(s, inp, NAN), cots)
        print(s.name, counts)
        assert counts["attention_masked"] == 2 and counts.get("attention_bwd_masked", 0) == 0, (s.name, counts)      # resampler_depth = 2
        assert counts.get("attention:lens", 0) == (1 if s.with_lens else 0), (s.name, counts)


# ------------------------------------------------------------------------------------------------ 3. the wrapper
from naturalspeech2_pytorch_amd import PhonemeEncoder  # noqa: E402
from naturalspeech2_pytorch_amd.training import GraphedTrainStep, Trainer  # noqa: E402

WB, WN_PH, WT, WN_P = 3, 12, 48, 16
W_TEXT, W_PROMPT, W_MEL = [12, 7, 3], [16, 9, 2], [48, 31, 14]


def _wrapper(switch=True, seed=131):
    """a small text-conditioned wrapper, every trainable member on the HIP training kernels, all dropouts 0"""
    torch.manual_seed(seed)                                 # PyTorch's default initialisation under a fixed seed
    model = Model(dim=64, depth=1, dim_prompt=64, condition_on_prompt=True, num_latents_m=8, cond_drop_prob=0., ragged_training=True)
    d = NaturalSpeech2(model, codec=None, target_sample_hz=24000, timesteps=2, build_aligner=True, build_duration_pitch=True, dim_codebook=64,
                       aligner_dim_hidden=64, pitch_emb_pp_hidden_dim=64, encoder_train_backend="hip", duration_pitch_train_backend="hip",
                       aligner_train_backend="hip", ragged_conditioning=switch)
    d.phoneme_enc = PhonemeEncoder(num_tokens=150, dim=64, dim_hidden=64, depth=1, heads=1, conv_dropout=0., attn_dropout=0., train_backend="hip")
    d.prompt_enc = SpeechPromptEncoder(dim_codebook=64, dims=(64, 64), depth=1, heads=1, dropout=0., train_backend="hip")
    d.duration_pitch = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=1, dropout=0., train_backend="hip")
    for mod in (d.phoneme_enc, d.prompt_enc, d.duration_pitch):
        mod.ragged_conditioning = switch
    return d.to(DEV).train()


def _wbatch(seed=140):
    g = torch.Generator().manual_seed(seed)
    return dict(audio=_mk("audio", (WB, WT, 64), seed), text=torch.randint(0, 150, (WB, WN_PH), generator=g).to(DEV),
                mel=_mk("mel", (WB, 80, WT), seed + 1), pitch=(80 + 300 * _mk("pitch", (WB, 1, WT), seed + 2, uniform=True)),
                prompt=_mk("prompt", (WB, WN_P, 64), seed + 3), times=_mk("times", (WB,), seed + 4, uniform=True),
                noise=_mk("noise", (WB, WT, 64), seed + 5))


def _wlens(text=W_TEXT, prompt=W_PROMPT, mel=W_MEL):
    return dict(text_lens=torch.tensor(text, device=DEV), prompt_lens=_i32(prompt), mel_lens=torch.tensor(mel, device=DEV), audio_lens=_i32(mel))


def _wstep(d, batch, lens):
    d.zero_grad(set_to_none=True)
    loss, aux = d(batch["audio"], return_aux_losses=True, **{k: v for k, v in batch.items() if k != "audio"}, **lens)
    (loss + aux["aux"]).backward()
    terms = dict(loss=loss.detach().clone(), **{k: v.detach().clone() for k, v in aux.items() if v is not None})
    return terms, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in d.named_parameters()}


def _wbehind(batch, value):
    """the batch with `value` behind every length: other ids, and value in prompt, latents, noise, mel and pitch"""
    out = dict(batch)
    out["text"] = _pad(batch["text"], W_TEXT, 7 if value != value else 3)
    out["prompt"] = _pad(batch["prompt"], W_PROMPT, value)
    for k in ("audio", "noise"):
        out[k] = _pad(batch[k], W_MEL, value)
    for k in ("mel", "pitch"):
        out[k] = _pad(batch[k], W_MEL, value, dim=-1)
    return out


def test_wrapper_loss_and_gradients_do_not_depend_on_the_padding(no_composite):
    d, batch, lens = _wrapper(), _wbatch(), _wlens()
    (ta, ga), (tb, gb) = _wstep(d, _wbehind(batch, NAN), lens), _wstep(d, _wbehind(batch, 2.5), lens)
    assert all(torch.isfinite(v).all() for v in ta.values()), ta
    for k in ta:
        assert _same_bits(ta[k], tb[k]), k
    n_grads = 0
    for k, v in ga.items():
        assert (v is None and gb[k] is None) or (torch.isfinite(v).all() and _same_bits(v, gb[k])), k
        n_grads += v is not None
    assert n_grads > 50 and all(ga[k] is not None for k in ("prompt_enc.conv.1.weight", "phoneme_enc.token_emb.weight", "duration_pitch.to_pitch_pred.to_pred.0.weight"))
    # the duration and pitch terms: the mean over the utterances of each one's own term alone (the existing pass, no lengths, cut inputs)
    solo = {"duration": [], "pitch": []}
    for i in range(WB):
        cut = dict(audio=batch["audio"][i:i + 1, :W_MEL[i]].contiguous(), text=batch["text"][i:i + 1, :W_TEXT[i]].contiguous(),
                   mel=batch["mel"][i:i + 1, :, :W_MEL[i]].contiguous(), pitch=batch["pitch"][i:i + 1, :, :W_MEL[i]].contiguous(),
                   prompt=batch["prompt"][i:i + 1, :W_PROMPT[i]].contiguous(), times=batch["times"][i:i + 1], noise=batch["noise"][i:i + 1, :W_MEL[i]].contiguous())
        t, _ = _wstep(d, cut, {})
        for k in solo:
            solo[k].append(t[k].double())
    for k in solo:
        want = torch.stack(solo[k]).mean()
        _record(f"tests/wrapper/{k}_vs_solo_mean", dict(batch=float(ta[k]), solo_mean=float(want), rel=abs(float(ta[k]) - float(want)) / abs(float(want))))
        assert abs(float(ta[k]) - float(want)) <= GRAD_TOL * abs(float(want)), (k, float(ta[k]), float(want))


def test_wrapper_prompt_lens_with_audio_lens_needs_the_switch():
    batch, lens = _wbatch(), _wlens()
    loss, _ = _wrapper()(batch["audio"], return_aux_losses=True, **{k: v for k, v in batch.items() if k != "audio"}, **lens)
    assert torch.isfinite(loss)
    with pytest.raises(NotImplementedError, match="prompt_lens in training"):
        _wrapper(switch=False)(batch["audio"], return_aux_losses=True, **{k: v for k, v in batch.items() if k != "audio"}, **lens)


def test_graphed_train_step_follows_text_and_prompt_lengths_rewritten_between_replays():
    d, batch = _wrapper(), _wbatch()
    keys = ("audio", "text", "mel", "pitch", "prompt", "times", "noise", "text_lens", "prompt_lens", "mel_lens", "audio_lens")

    def fn(*ts):
        kw = dict(zip(keys, ts))
        loss, aux = d(kw.pop("audio"), return_aux_losses=True, **kw)
        return loss + aux["aux"]

    captured, other = _wlens(), _wlens(text=[5, 12, 9], prompt=[3, 16, 11])
    args = lambda ln: tuple(batch[k] if k in batch else ln[k] for k in keys)          # noqa: E731
    step = GraphedTrainStep(fn, args(captured), d)
    for ln in (other, captured):
        loss = step(*args(ln)).detach().clone()
        grads = [None if g is None else g.detach().clone() for g in step.grads]
        d.zero_grad(set_to_none=True)
        loss_e = fn(*args(ln))
        loss_e.backward()
        assert torch.isfinite(loss) and _same_bits(loss, loss_e.detach())
        for p, g in zip(step.params, grads):
            assert (g is None and p.grad is None) or _same_bits(g, p.grad)
    assert float(step(*args(other))) != float(step(*args(captured)))                    # the lengths do reach the loss


def test_trainer_takes_dict_batches_with_text_and_prompt_lens(tmp_path):
    d = _wrapper()
    data = [dict(_wbatch(150 + i), **_wlens()) for i in range(2)]
    tr = Trainer(d, dataloader=data, train_lr=1e-3, train_num_steps=2, use_ema=False, save_and_sample_every=0, results_folder=tmp_path / "run",
                 use_graph=False)
    for _ in range(2):
        tr.train_step()
        assert bool(torch.isfinite(tr.last_loss))
    assert int(tr.opt.steps_taken) == 2
