"""Skipping the hidden row tiles of a ragged TRAINING batch on the MI355X (include/ns2hip_train.h): the two kernels entries
bit for bit against the entries without lengths, `Model(ragged_skip_training=True)` against the same call with the switch off, and a
captured step whose lengths are rewritten between replays.  The reference is never the skipping code itself.

Kernel batch: 3 utterances x 512 rows, lens [300, 256, 7] -> computed extents H = [512, 256, 256]: no hidden tile, one behind an exact
granule, one behind a short utterance.  Model batch: 6 x 512, lens [512, 300, 256, 130, 7, 257] -> H = [512, 512, 256, 256, 256, 512]."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd.training import HipBackend  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
KB, KN, KLENS, KK = 3, 512, [300, 256, 7], 128
KM = KB * KN
ROUTES = dict(splitk=0, tile128=1, tile256=2, ffconv3=3, linear3=4, wavenet3=5)


def extent(l, n):
    return min(n, 256 * ((min(max(l, 1), n) + 255) // 256))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _force_gemm(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


def _skip_launches():
    return int(_lib.load().ns2_debug_train_skip_launches())


def _route_counts():
    lib = _lib.load()
    return [int(lib.ns2_debug_gemm_route_launches(r)) for r in range(6)]


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _hidden_rows(B, N, lens):
    """bool [B N]: True on the rows at or behind their utterance's computed extent"""
    h = torch.tensor([extent(l, N) for l in lens])
    return (torch.arange(N)[None] >= h[:, None]).reshape(B * N).to(DEV)


def _planes_like(p, fill_hidden=None, hidden=None):
    """a copy of the planes p; fill_hidden: that byte into every byte of the hidden rows"""
    q = ops.Planes(p.buf.clone(), p.rows, p.ld, p.has_lo, p.fmt)
    if fill_hidden is not None:
        q.buf.view(torch.uint8).view(p.rows, -1)[hidden] = fill_hidden
    return q


def _ff_planes(rows, cols, precision, attention_operand=False):
    lo, fmt = ops._fmt_of(precision, attention_operand)
    p = ops.empty_planes(rows, cols, DEV, lo, fmt=fmt)
    p.buf.view(torch.uint8).fill_(0xFF)
    return p


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _finite_planes(buf, fmt):
    """every 16-bit value of bf16 / f16 planes is finite; the half part of FMT_H8 lines is (its bytes are e5m2: 0xFF would be a NaN too)"""
    if fmt == "bf16":
        return bool(torch.isfinite(buf.float()).all())
    if fmt == "f16":
        return bool(torch.isfinite(buf.float()).all())
    lines = buf.view(buf.shape[0], -1, 2, 32)
    half_ok = torch.isfinite(lines[:, :, 0].float()).all()
    e5m2 = lines[:, :, 1].contiguous().view(torch.uint8)
    return bool(half_ok) and bool(((e5m2 & 0x7C) != 0x7C).all())


# ------------------------------------------------------------------------------------------------ 1. ns2_linear_lens_zero
def _linear(w, a, precision, lens, **fields):
    args = _lib.LinearArgs(w=w.handle, a_hi=a.hi, a_lo=a.lo, lda=a.ld, M=KM, precision=precision, **fields)
    lib = _lib.load()
    if lens is None:
        _lib.check(lib.ns2_linear(args, _stream()), "ns2_linear")
    else:
        _lib.check(lib.ns2_linear_lens_zero(ctypes.byref(args), lens.data_ptr(), KN, _stream()), "ns2_linear_lens_zero")


VARIANTS = {"plain": {}, "causal": dict(conv_taps=3, dilation=2, seq_len=KN, pad_left=-1), "anticausal": dict(conv_taps=3, dilation=2, seq_len=KN, pad_left=0)}


@pytest.mark.parametrize("mode", [1, 2, 5])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("ncol", [96, 512])
@pytest.mark.parametrize("precision", [3, 4])
def test_linear_lens_zero_keeps_visible_bits_and_zeroes_hidden_tiles(precision, ncol, variant, mode):
    """rows before H_i: the bits of ns2_linear on the operand with its hidden rows zeroed; rows from H_i on: zero bits in every output --
    fp32, fp32 + residual, operand planes, attention planes of a precision-4 product -- although each output buffer came full of 0xFF.
    The operand's hidden rows hold 0xFF for the causal and plain products (never read from a visible row) and zeros for the anticausal
    one (the contract of include/ns2hip_train.h)."""
    hidden = _hidden_rows(KB, KN, KLENS)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    taps = 3 if variant != "plain" else 0
    x = _rand((KM, KK), 11)
    x[hidden] = 0.
    w = ops.PackedWeight(_rand((ncol, KK, 3) if taps else (ncol, KK), 12, 0.1), precision=precision)
    if precision == 4 and not taps:
        w.tile_linear()
    a_ref = ops.split(x, precision=precision)
    a_got = a_ref if variant == "anticausal" else _planes_like(a_ref, 0xFF, hidden)
    bias, res = _rand((ncol,), 13), _rand((KM, ncol), 14)
    ldo = ops.round_up(ncol, 32)
    outputs = ["f32", "f32_resid", "planes"] + (["attn_planes"] if precision == 4 else [])

    def run(kind, a, with_lens):
        common = dict(bias=bias.data_ptr(), **VARIANTS[variant])
        if kind.startswith("f32"):
            out = torch.empty(KM, ncol, device=DEV)
            out.view(torch.uint8).fill_(0xFF)
            r = res if kind == "f32_resid" else None
            _linear(w, a, precision, lens if with_lens else None, out_f32=out.data_ptr(), ldo_f=ncol, resid=ops._p(r), ldr=ncol if r is not None else 0,
                    **common)
            return out, "f32"
        op = 3 if kind == "attn_planes" else precision
        out = _ff_planes(KM, ldo, op)
        _linear(w, a, precision, lens if with_lens else None, out_hi=out.hi, out_lo=out.lo, ldo=ldo, out_precision=op if op != precision else 0,
                **common)
        return out.buf, out.fmt

    try:
        _force_gemm(mode)
        before, n0 = _route_counts(), _skip_launches()
        pairs = {kind: (run(kind, a_ref, False), run(kind, a_got, True)) for kind in outputs}
        torch.cuda.synchronize()
        taken = {r: n - b for r, (n, b) in enumerate(zip(_route_counts(), before)) if n != b}
        sent = _skip_launches() - n0
    finally:
        _force_gemm(0)
    # the kernel under test ran, with and without lengths: mode 5 = the lean linear kernel for a plain FMT_H8 product, else chosen by
    # shape (12 blocks of 256 x 256: the 128 x 128 kernel)
    want = {1: "tile128", 2: "tile256", 5: "linear3" if (precision == 4 and not taps) else "tile128"}[mode]
    assert taken == {ROUTES[want]: 2 * len(outputs)}, (taken, want)
    assert sent == len(outputs)
    assert bool(hidden.any()) and not bool(hidden.all())
    for kind, ((ref, _), (got, fmt)) in pairs.items():
        what = f"{kind} p{precision} {ncol} columns {variant} mode {mode}"
        r2, g2 = _bits(ref).view(KM, -1), _bits(got).view(KM, -1)
        assert torch.equal(g2[~hidden], r2[~hidden]), f"{what}: rows before an extent differ from ns2_linear"
        if fmt == "f32":
            assert torch.count_nonzero(got[hidden]) == 0 and torch.count_nonzero(g2[hidden]) == 0, f"{what}: hidden rows are not zero bits"
            assert bool(torch.isfinite(got).all()), what
        else:
            # zero bits in the columns the product owns ([0, ldo): every plane of the lines); finite everywhere
            assert torch.count_nonzero(g2[hidden]) == 0, f"{what}: hidden rows are not zero bits"
            assert _finite_planes(got, fmt), what


def test_linear_lens_zero_refuses_what_linear_lens_refuses():
    lib = _lib.load()
    w = ops.PackedWeight(_rand((96, KK), 12, 0.1), precision=3)
    a = ops.split(_rand((KM, KK), 11), precision=3)
    out = torch.empty(KM, 96, device=DEV)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    args = _lib.LinearArgs(w=w.handle, a_hi=a.hi, a_lo=a.lo, lda=a.ld, M=KM, precision=3, out_f32=out.data_ptr(), ldo_f=96)
    for ln, n, word in ((None, KN, "row_lens is null"), (lens.data_ptr(), 384, "multiple of 256"), (lens.data_ptr(), 1024, "whole utterances")):
        rc = lib.ns2_linear_lens_zero(ctypes.byref(args), ln, n, _stream())
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith("ns2_linear_lens_zero:") and word in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ 2. ns2_wgrad_rows_lens
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("R", [96, 256])
@pytest.mark.parametrize("precision", [3, 4])
def test_wgrad_rows_lens_skips_hidden_k_tiles(precision, R, T):
    """dY and X hold 0xFF in every byte of their hidden rows: bit-equal to ns2_wgrad_rows on operands with those rows zeroed, and
    finite -- the hidden tiles were not multiplied (0xFF is a NaN in every format).  Full lengths: bit-equal to ns2_wgrad_rows."""
    hb = HipBackend(precision)
    hidden = _hidden_rows(KB, KN, KLENS)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    dy, x = _rand((KM, R), 41), _rand((KM, KK), 42)
    dy[hidden] = 0.
    x[hidden] = 0.
    dy_ref, x_ref = ops.split(dy, precision=precision), ops.split(x, precision=precision)
    dy_ff, x_ff = _planes_like(dy_ref, 0xFF, hidden), _planes_like(x_ref, 0xFF, hidden)
    dil = 2 if T > 1 else 1
    n0 = _skip_launches()
    ref = hb.wgrad_rows(dy_ref, x_ref, R, T, KK, dil, KN)
    assert _skip_launches() == n0
    got = hb.wgrad_rows(dy_ff, x_ff, R, T, KK, dil, KN, row_lens=(lens, KN))
    assert _skip_launches() == n0 + 1
    full = hb.wgrad_rows(dy_ref, x_ref, R, T, KK, dil, KN, row_lens=(torch.full((KB,), KN, dtype=torch.int32, device=DEV), KN))
    torch.cuda.synchronize()
    assert got.shape == (R, KK, T) and bool(torch.isfinite(got).all())
    assert torch.equal(_bits(got), _bits(ref)), "visible tokens: the bits of ns2_wgrad_rows on zeroed hidden rows"
    assert torch.equal(_bits(full), _bits(ref)), "full lengths: the bits of ns2_wgrad_rows"
    assert float(ref.abs().max()) > 0


def test_wgrad_rows_lens_slices_that_straddle_an_extent():
    """the batch of the model tests with a gradient wide enough (24 tiles of 256 x 256) that the slice plan takes 8 slices of 12 K tiles
    = 384 tokens: slices begin and end inside hidden runs and step over them in mid-loop (the cases above have slices of one granule)"""
    B, N, lens_l, R, K, T = 6, 512, [512, 300, 256, 130, 7, 257], 1024, 512, 3
    for precision in (3, 4):
        hb = HipBackend(precision)
        hidden = _hidden_rows(B, N, lens_l)
        lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
        dy, x = _rand((B * N, R), 43, 0.5), _rand((B * N, K), 44, 0.5)
        dy[hidden] = 0.
        x[hidden] = 0.
        dy_ref, x_ref = ops.split(dy, precision=precision), ops.split(x, precision=precision)
        ref = hb.wgrad_rows(dy_ref, x_ref, R, T, K, 2, N)
        got = hb.wgrad_rows(_planes_like(dy_ref, 0xFF, hidden), _planes_like(x_ref, 0xFF, hidden), R, T, K, 2, N, row_lens=(lens, N))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(ref)), precision


def test_wgrad_rows_lens_refuses():
    lib = _lib.load()
    hb = HipBackend(3)
    p = ops.split(_rand((KM, KK), 42), precision=3)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    dw = torch.empty(KK, KK, 1, device=DEV)
    nbytes = lib.ns2_wgrad_workspace_bytes(KK, KK, KM)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for ln, n, word in ((None, KN, "row_lens is null"), (lens.data_ptr(), 384, "multiple of 256"), (lens.data_ptr(), 1024, "whole utterances")):
        rc = lib.ns2_wgrad_rows_lens(p.hi, p.lo, p.ld, p.hi, p.lo, p.ld, KM, KK, 1, KK, KK, 1, n, dw.data_ptr(), ws.data_ptr(), nbytes, 3, ln, _stream())
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith("ns2_wgrad_rows_lens:") and word in msg, (rc, msg)
    del hb


# ------------------------------------------------------------------------------------------------ 3. the model
MB, MN, MLENS = 6, 512, [512, 300, 256, 130, 7, 257]
CFG = {"d128": dict(dim=128, depth=2), "d512": dict(dim=512, depth=1),
       "cond": dict(dim=256, depth=1, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}


def _model(name, tprec):
    m = Model(**CFG[name], ragged_training=True)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    return m


def _inputs(name, n=MN):
    d = CFG[name]["dim"]
    mk = lambda nm, shape, seed, **k: make_input(nm, shape, seed=seed, **k).to(DEV)      # noqa: E731
    x, t, cot = mk("x", (MB, n, d), 2), mk("times", (MB,), 2, uniform=True), mk("gw", (MB, n, d), 3)
    prompt = cond = None
    if CFG[name].get("condition_on_prompt"):
        prompt, cond = mk("prompt", (MB, 7, 48), 2), mk("cond", (MB, 48, n), 2)
    return x, t, prompt, cond, cot


def _run(m, lens, x, t, prompt, cond, cot):
    """-> (loss, output, {parameter: gradient}) of sum(m(x, lens=) * cot)"""
    for p in m.parameters():
        p.grad = None
    kw = {} if prompt is None else dict(prompt=prompt, cond=cond, cond_drop_prob=0.)
    y = m(x, t, lens=lens, **kw)
    loss = (y * cot).sum()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), y.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _same(a, b, what):
    (la, ya, ga), (lb, yb, gb) = a, b
    assert bool(torch.isfinite(la)) and torch.equal(la, lb), f"{what}: loss"
    assert bool(torch.isfinite(ya).all()) and torch.equal(ya, yb), f"{what}: output"
    for k, v in gb.items():
        assert (v is None) == (ga[k] is None), (what, k)
        if v is not None:
            assert bool(torch.isfinite(ga[k]).all()) and torch.equal(ga[k], v), f"{what}: gradient of {k}"


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
@pytest.mark.parametrize("name", sorted(CFG))
def test_model_with_the_switch_on_has_the_bits_of_the_switch_off(name, tprec):
    """loss, output and every parameter gradient torch.equal to the same call with the switch off; NaN lies behind each length in x and
    cond.  The counter rises with the switch on and not at all with it off.  Full lengths and n = 384 change nothing and raise nothing.
    Mode 3 of the GEMM hook (never split K) for both runs, so that batch size alone does not pick another kernel."""
    m = _model(name, tprec)
    assert m.ragged_skip_training is False
    x, t, prompt, cond, cot = _inputs(name)
    lens = torch.tensor(MLENS, dtype=torch.int32, device=DEV)
    for i, n in enumerate(MLENS):
        x[i, n:] = float("nan")
        if cond is not None:
            cond[i, :, n:] = float("nan")
    try:
        _force_gemm(3)
        n0 = _skip_launches()
        off = _run(m, lens, x, t, prompt, cond, cot)
        assert _skip_launches() == n0, "the switch is off: no launch may carry lengths"
        m.ragged_skip_training = True                       # a plain attribute
        on = _run(m, lens, x, t, prompt, cond, cot)
        sent = _skip_launches() - n0
        assert sent > 0, "the switch is on: the products must have been handed the lengths"
        _same(on, off, f"{name} {tprec}")
        assert all(torch.count_nonzero(on[1][i, n:]) == 0 for i, n in enumerate(MLENS))
        # full lengths: the same bits as the switch off at full lengths
        full = torch.full((MB,), MN, dtype=torch.int32, device=DEV)
        xf, tf, pf, cf, cotf = _inputs(name)
        on_full = _run(m, full, xf, tf, pf, cf, cotf)
        m.ragged_skip_training = False
        _same(on_full, _run(m, full, xf, tf, pf, cf, cotf), f"{name} {tprec} full lengths")
        # n = 384 is no multiple of 256: the switch does nothing (no launch with lengths) and raises nothing
        x3, t3, p3, c3, cot3 = _inputs(name, 384)
        l3 = lens.clamp(max=384)
        off3 = _run(m, l3, x3, t3, p3, c3, cot3)
        m.ragged_skip_training = True
        n1 = _skip_launches()
        on3 = _run(m, l3, x3, t3, p3, c3, cot3)
        assert _skip_launches() == n1
        _same(on3, off3, f"{name} {tprec} n = 384")
    finally:
        _force_gemm(0)
    print(f"{name} {tprec}: {sent} launches carried lengths")


def test_the_switch_does_nothing_without_lens_and_is_a_keyword():
    m = Model(dim=128, depth=1, ragged_training=True, ragged_skip_training=True)
    assert m.ragged_skip_training is True
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    m = m.to(DEV).train()
    x, t, cot = make_input("x", (2, 256, 128), seed=2).to(DEV), make_input("times", (2,), seed=2, uniform=True).to(DEV), make_input("gw", (2, 256, 128), seed=3).to(DEV)
    n0 = _skip_launches()
    on = _run(m, None, x, t, None, None, cot)
    assert _skip_launches() == n0
    m.ragged_skip_training = False
    _same(on, _run(m, None, x, t, None, None, cot), "no lens")


# ------------------------------------------------------------------------------------------------ 4. the captured step
@pytest.mark.parametrize("tprec", ["exact", "mixed"])
def test_graphed_train_step_follows_lengths_rewritten_between_replays(tprec):
    """only kernels read the lengths: two replays are bit-equal to the eager pass at each set of lengths"""
    m = Model(dim=256, depth=1, ragged_training=True, ragged_skip_training=True)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=71))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2).to(DEV)
    mk = lambda name, shape, **k: make_input(name, shape, seed=80, **k).to(DEV)    # noqa: E731
    a, t, z = mk("audio", (4, 512, 256)), mk("times", (4,), uniform=True), mk("noise", (4, 512, 256))
    captured, other = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([512, 40, 256, 300], [33, 512, 257, 256]))
    try:
        _force_gemm(3)
        step = training.GraphedTrainStep(lambda au, ln, ts, no: d(au, audio_lens=ln, times=ts, noise=no), (a, captured, t, z), m)
        for lens in (other, captured):
            loss = step(a, lens, t, z).detach().clone()
            grads = [None if gr is None else gr.detach().clone() for gr in step.grads]
            for p in m.parameters():
                p.grad = None
            n0 = _skip_launches()
            loss_e = d(a, audio_lens=lens, times=t, noise=z)
            loss_e.backward()
            assert _skip_launches() > n0
            assert torch.isfinite(loss) and torch.equal(loss, loss_e.detach())
            for p, gr in zip(step.params, grads):
                assert (gr is None and p.grad is None) or torch.equal(gr, p.grad)
        assert float(step(a, other, t, z)) != float(step(a, captured, t, z))        # the lengths do reach the loss
    finally:
        _force_gemm(0)
