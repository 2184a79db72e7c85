"""The feed-forward fold (include/ns2hip.h): FeedForward's CausalConv1d(f, f, 3) and the Linear(f, dim) behind it (NS2:1016-1024) as
ONE causal conv f -> dim.

  * op level: the fold kernel against torch.einsum in fp64; the dedicated FF conv kernel's fp32 output mode (csrc/ffconv_kernel.h) against
    the general kernel on the same operands, bit for bit;
  * model level: a folded model against the fp32 oracle under the ceilings of tests/test_parity_r2_gpu.py, against the unfolded model
    (the triangle inequality), the switch, the content fingerprint, and batches cut differently.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, _lib, ops  # noqa: E402
from oracle import ns2_oracle as O  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")


def _force_gemm(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


def _force_fold(k):
    _lib.check(_lib.load().ns2_debug_force_fold(k), "ns2_debug_force_fold")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _fold(w_out, w_conv, b_conv, b_out):
    dim, f = w_out.shape
    wf = torch.empty(dim, f, 3, dtype=torch.float32, device=DEV)
    bf = torch.empty(dim, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().ns2_ff_fold(w_out.data_ptr(), w_conv.data_ptr(), b_conv.data_ptr(), b_out.data_ptr(), dim, f, wf.data_ptr(),
                                      bf.data_ptr(), torch.cuda.current_stream().cuda_stream), "ns2_ff_fold")
    return wf, bf


# ---------------------------------------------------------------------------------------------- the fold kernel
@pytest.mark.parametrize("dim,f", [(64, 170), (128, 341)])
def test_fold_kernel_against_fp64_einsum(dim, f):
    """W'[n, c, t] = sum_j W_out[n, j] W_conv[j, c, t], b' = W_out b_conv + b_out: bit-identical from run to run, and as close to fp64 as
    an fp32 sum of f terms is -- under 10 x the 3.4e-7 measured for the fp32 fold at dim 512 / f 1365 (the sums here are shorter)"""
    g = torch.Generator().manual_seed(dim + f)
    w_out = (torch.randn(dim, f, generator=g) * f ** -0.5).to(DEV)
    w_conv = (torch.randn(f, f, 3, generator=g) * (3 * f) ** -0.5).to(DEV)
    b_conv, b_out = torch.randn(f, generator=g).to(DEV), torch.randn(dim, generator=g).to(DEV)
    wf, bf = _fold(w_out, w_conv, b_conv, b_out)
    wf2, bf2 = _fold(w_out, w_conv, b_conv, b_out)
    assert torch.equal(wf, wf2) and torch.equal(bf, bf2)
    ref_w = torch.einsum("nj,jct->nct", w_out.double(), w_conv.double())
    ref_b = w_out.double() @ b_conv.double() + b_out.double()
    ew, eb = _rel(wf, ref_w), _rel(bf, ref_b)
    print(f"fold kernel dim {dim} f {f}: rel err W' {ew:.3e}, b' {eb:.3e}")
    assert ew < 3.4e-6 and eb < 3.4e-6, (ew, eb)


# ---------------------------------------------------------------------------------------------- the conv kernel's fp32 output
def _conv_ref64(xh, wh, bias, B, N):
    x = xh.double().reshape(B, N, -1).transpose(1, 2)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (2, 0)), wh.double(), bias.double())
    return y.transpose(1, 2).reshape(B * N, -1)


@pytest.mark.parametrize("with_resid", [True, False], ids=["resid", "no_resid"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("R", [512, 384, 64])
def test_folded_conv_kernel_equals_the_general_kernel(R, B, with_resid):
    """R = 512: two full column tiles; 384: a full and a half-valid one; 64: a quarter tile.  f = 170: Cp = 192 in rows of 256, so the last K
    tile is padding (kv < lda).  Utterances of 256 frames: every row tile is the first of its utterance, and with B = 2 the second
    must not see the first -- its rows equal the rows of that utterance run alone."""
    N, C = 256, 170
    g = torch.Generator().manual_seed(2000 + R + B)
    x = torch.randn(B * N, C, generator=g)
    w = torch.randn(R, C, 3, generator=g) * (3 * C) ** -0.5
    bias = torch.randn(R, generator=g)
    resid = torch.randn(B * N, R, generator=g).to(DEV) if with_resid else None
    ld = ops.conv3_input_ld(C)
    assert ld == 256
    a = ops.split(x.to(DEV), ldo=ld, precision=2)
    a.buf.view(B * N, ld)[:, ops.round_up(C, 32):] = float("nan")          # padding: fetched, never multiplied
    pw = ops.PackedWeight(w.to(DEV), precision=2).tile_conv3()
    bd = bias.to(DEV)

    def run(aa=a, rr=resid):
        return ops.linear_f32(pw, aa, bias=bd, resid=rr, conv_taps=3, dilation=1, seq_len=N, precision=2)

    try:
        _force_gemm(5)               # the dedicated kernel whatever the size
        new, new2 = run(), run()
        alone = None
        if B == 2:
            a1 = ops.Planes(a.buf[N:].contiguous(), N, ld, False, "f16")
            alone = run(a1, resid[N:].contiguous() if with_resid else None)
        _force_gemm(2)               # gemm2_kernel, the general route of the half plans
        old = run()
    finally:
        _force_gemm(0)
    assert torch.isfinite(new).all()
    assert torch.equal(new, new2), "two launches of the dedicated kernel differ"
    assert torch.equal(new, old), "the conv kernel's fp32 output differs from the general kernel's"
    if alone is not None:
        assert torch.equal(new[N:], alone), "the second utterance saw the first"
    ref = _conv_ref64(x.half().float(), w.half().float(), bias, B, N)
    if with_resid:
        ref = ref + resid.cpu().double()
    assert _rel(new.cpu(), ref) < 1e-5      # fp32 accumulation of K = 510 half products


# ---------------------------------------------------------------------------------------------- the model
CEIL = {"exact": 1e-4, "mixed": 5e-4, "hybrid": 5e-4, "half": 5e-3}       # tests/test_parity_r2_gpu.py
_COND = dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True)
MODELS = [(dict(dim=64, depth=2), p) for p in CEIL] + [(dict(dim=256, depth=1), p) for p in CEIL] + [(_COND, "hybrid")]
_REF = {}


def _setup(kw, seed=21):
    key = tuple(sorted(kw.items()))
    if key not in _REF:                      # one oracle run per architecture serves every plan
        m = Model(**kw)
        sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
        B, N, d = 2, 256, kw["dim"]
        ins = dict(x=make_input("x", (B, N, d), seed=seed + 1), times=make_input("times", (B,), seed=seed + 1, uniform=True))
        if kw.get("condition_on_prompt"):
            ins.update(prompt=make_input("prompt", (B, 37, kw["dim_prompt"]), seed=seed + 2),
                       cond=make_input("cond", (B, kw["dim_prompt"], N), seed=seed + 3))
        with torch.no_grad():
            ref = O.model_forward(sd, ins["x"], ins["times"], ins.get("prompt"), ins.get("cond"))
        _REF[key] = (sd, ins, ref)
    return _REF[key]


def _run(m, ins):
    extra = {k: v.to(DEV) for k, v in ins.items() if k in ("prompt", "cond")}
    with torch.no_grad():
        return m(ins["x"].to(DEV), ins["times"].to(DEV), **extra).clone()


@pytest.mark.parametrize("kw,precision", MODELS, ids=[f"d{k['dim']}{'c' if k.get('condition_on_prompt') else ''}-{p}" for k, p in MODELS])
def test_folded_model_against_the_oracle_and_the_unfolded_model(kw, precision):
    sd, ins, ref = _setup(kw)
    m = Model(**kw, precision=precision)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    try:
        _force_fold(1)
        y_on = _run(m, ins)
        _force_fold(0)
        m.invalidate()
        y_off = _run(m, ins)
        m.invalidate()                        # a second finalize with the fold off: the parent's arithmetic, the same bits
        y_off2 = _run(m, ins)
    finally:
        _force_fold(1)
    e_on, e_off = _rel(y_on.cpu(), ref), _rel(y_off.cpu(), ref)
    diff = ((y_on.double() - y_off.double()).norm().item() / ref.double().norm().item())      # relative to the oracle's norm, like e_on and e_off
    print(f"fold {kw} {precision}: vs oracle on {e_on:.3e} off {e_off:.3e}; on vs off {diff:.3e}")
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_off, y_off2)
    assert not torch.equal(y_on, y_off), "the switch changed nothing"
    assert e_on < CEIL[precision], (precision, e_on)
    assert diff <= (e_on + e_off) * (1 + 1e-9), (diff, e_on, e_off)       # |on - off| <= |on - ref| + |off - ref|: no invented number


def test_a_data_write_yields_a_new_fold():
    """ema_pytorch writes through `.data`: the content fingerprint re-finalizes, and W' is folded from the new weights"""
    kw = dict(dim=64, depth=2)
    sd, ins, _ = _setup(kw)
    m = Model(**kw, precision="hybrid")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    y0 = _run(m, ins)
    params = dict(m.named_parameters())
    params["transformer.layers.0.5.2.1.weight"].data.mul_(1.5)          # the causal conv of layer 0's feed-forward
    params["transformer.layers.1.5.3.weight"].data.mul_(0.5)            # FF-out of layer 1
    assert m.refresh_weights() is True
    y1 = _run(m, ins)
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref2 = O.model_forward(sd2, ins["x"], ins["times"])
    assert not torch.equal(y1, y0)
    assert _rel(y1.cpu(), ref2) < CEIL["hybrid"], _rel(y1.cpu(), ref2)


def test_folded_model_computes_the_same_rows_however_the_batch_is_cut():
    """a split batch, a doubled batch (classifier-free guidance as one 2 B batch) and a one-utterance batch: the same rows, bit for bit,
    where every batch takes the same kernels (ns2_debug_force_gemm(5): the dedicated kernels whatever the size, never split K)"""
    kw = dict(dim=64, depth=2)
    m = Model(**kw, precision="hybrid")
    sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=41)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    B, N = 4, 256
    x = make_input("x", (B, N, 64), seed=42).to(DEV)
    t = torch.full((B,), 0.37, device=DEV)
    try:
        _force_gemm(5)
        with torch.no_grad():
            y = m(x, t).clone()
            halves = torch.cat([m(x[:2], t[:2]), m(x[2:], t[2:])])
            one = m(x[1:2], t[1:2]).clone()
            twice = m(torch.cat([x, x]), torch.cat([t, t])).clone()
    finally:
        _force_gemm(0)
    assert torch.equal(halves, y)
    assert torch.equal(one, y[1:2])
    assert torch.equal(twice[:B], y) and torch.equal(twice[B:], y)


def test_cfg_as_one_batch_equals_two_passes_with_the_fold():
    """NS2:914-927 on a conditioned model: the conditioned and the null forward as ONE batch of 2 B utterances against two passes"""
    sd, ins, _ = _setup(_COND)
    m = Model(**_COND, precision="hybrid")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    args = dict(prompt=ins["prompt"].to(DEV), cond=ins["cond"].to(DEV), cond_scale=1.3)
    x, t = ins["x"].to(DEV), ins["times"].to(DEV)
    try:
        _force_gemm(5)
        with torch.no_grad():
            assert x.shape[0] <= m.CFG_ONE_BATCH_MAX
            y1 = m.forward_with_cond_scale(x, t, **args).clone()
            old, m.CFG_ONE_BATCH_MAX = m.CFG_ONE_BATCH_MAX, 0
            try:
                y2 = m.forward_with_cond_scale(x, t, **args).clone()
            finally:
                m.CFG_ONE_BATCH_MAX = old
    finally:
        _force_gemm(0)
    with torch.no_grad():
        ref = O.model_forward_with_cond_scale(sd, ins["x"], ins["times"], ins["prompt"], ins["cond"], 1.3)
    assert torch.equal(y1, y2)
    assert _rel(y1.cpu(), ref) < CEIL["hybrid"]
