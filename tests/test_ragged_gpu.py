"""Ragged batches on the MI355X (include/ns2hip.h): per-utterance lengths in the two attention forward kernels, through the
executor, Model.forward(lens=) and the sampler.  The definition under test: utterance i of a ragged batch equals utterance i alone at its
own length -- so what lies at or beyond a length (NaN included, at kernel level) must not reach the frames before it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, ops  # noqa: E402
from oracle import ns2_oracle as O  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")


def _force_attention(k):
    _lib.check(_lib.load().ns2_debug_force_attention(k), "ns2_debug_force_attention")


def _fast_launches():
    return int(_lib.load().ns2_debug_attention_fast_launches())


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
def _operands(B, H, N, D, prec, lens, seed):
    """q, k, V^T planes of a self-attention over B utterances of N frames; K rows and V^T columns at or beyond each utterance's length are
    NaN in every plane (written into the packed buffers: the conversions never see them)"""
    a = H * D
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B * N, a, generator=g).to(DEV) for _ in range(3))
    sp = 2 if prec == 4 else prec
    qp, kp = ops.split(q, precision=sp), ops.split(k, precision=sp)
    vt = ops.split(v.reshape(B, N, a).transpose(1, 2).reshape(B * a, N).contiguous(), ldo=N, precision=sp)
    nan = float("nan")
    for b, n in enumerate(lens):
        n = min(max(n, 1), N)
        kp.buf.view(B, N, -1)[b, n:] = nan
        if vt.has_lo:                                     # interleaved lines [hi(32) | lo(32)] per 32 logical columns
            cols = (torch.arange(N, device=DEV) >= n).view(N // 32, 1, 32).expand(N // 32, 2, 32)
            vt.buf.view(B, a, N // 32, 2, 32)[b][:, cols] = nan
        else:
            vt.buf.view(B, a, N)[b, :, n:] = nan
    return qp, kp, vt


def _rows(p, r0, n):
    return ops.Planes(p.buf[r0:r0 + n], n, p.ld, p.has_lo, p.fmt)


def _alone(qp, kp, vt, b, H, N, D, n, prec):
    """utterance b by the call that exists without this feature: its own slices, Nk = its length"""
    a = H * D
    return ops.attention(_rows(qp, b * N, N), _rows(kp, b * N, n), _rows(vt, b * a, a), 1, H, N, n, k_col0=0, precision=prec, head_dim=D)


def _check_against_alone(out, qp, kp, vt, B, H, N, D, lens, prec):
    assert torch.isfinite(ops.join(out)).all()
    for b, n in enumerate(lens):
        solo = _alone(qp, kp, vt, b, H, N, D, min(max(n, 1), N), prec)
        assert torch.equal(_bits(out.buf[b * N:(b + 1) * N]), _bits(solo.buf)), f"utterance {b} (length {n})"


@pytest.mark.parametrize("prec", [2, 4])
def test_fast_kernel_takes_lengths_and_equals_attn_kernel_and_the_utterance_alone(prec):
    """full; partial last tile; one tile plus one key; exactly one tile; one key"""
    B, H, N, D, lens = 5, 2, 512, 64, [512, 447, 65, 64, 1]
    qp, kp, vt = _operands(B, H, N, D, prec, lens, seed=60)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    try:
        _force_attention(0)
        n0 = _fast_launches()
        new = ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_lens=kl)
        n1 = _fast_launches()
        _force_attention(1)
        old = ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_lens=kl)
        n2 = _fast_launches()
        torch.cuda.synchronize()
    finally:
        _force_attention(0)
    assert n1 - n0 == 1 and n2 == n1, "lengths must take attn_fast_kernel by eligibility, and attn_kernel when forced"
    assert torch.equal(_bits(new.buf), _bits(old.buf))
    _check_against_alone(new, qp, kp, vt, B, H, N, D, lens, prec)
    # a byte mask still keeps the generic kernel, and lengths with a mask are refused
    n0 = _fast_launches()
    ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_mask=torch.ones(B, N, dtype=torch.bool, device=DEV))
    assert _fast_launches() == n0
    with pytest.raises(_lib.Ns2Error, match="ns2_attention_fwd_lens: key_mask"):
        ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_lens=kl, key_mask=torch.ones(B, N, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("prec,D", [(3, 64), (2, 32), (3, 32), (2, 128), (3, 128), (4, 64)])
def test_attn_kernel_takes_lengths_for_every_head_dim(prec, D):
    """shapes attn_fast_kernel does not take (96 keys: a partial tile also at full length)"""
    B, H, N, lens = 2, 2, 96, [96, 33]
    qp, kp, vt = _operands(B, H, N, D, prec, lens, seed=61)
    n0 = _fast_launches()
    out = ops.attention(qp, kp, vt, B, H, N, N, precision=prec, head_dim=D, key_lens=torch.tensor(lens, device=DEV))
    assert _fast_launches() == n0
    _check_against_alone(out, qp, kp, vt, B, H, N, D, lens, prec)


@pytest.mark.parametrize("forced", [0, 1])
def test_lengths_outside_the_range_are_clamped(forced):
    """0 counts as 1 and Nk + 5 as Nk: no read out of bounds, no empty softmax, in either kernel"""
    B, H, N, D, prec = 3, 2, 256, 64, 2
    bad, good = [0, N + 5, 70], [1, N, 70]
    qp, kp, vt = _operands(B, H, N, D, prec, good, seed=62)
    try:
        _force_attention(forced)
        a = ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_lens=torch.tensor(bad, device=DEV))
        b = ops.attention(qp, kp, vt, B, H, N, N, precision=prec, key_lens=torch.tensor(good, device=DEV))
        torch.cuda.synchronize()
    finally:
        _force_attention(0)
    assert torch.isfinite(ops.join(a)).all() and torch.equal(_bits(a.buf), _bits(b.buf))
    _check_against_alone(a, qp, kp, vt, B, H, N, D, good, prec)


# ------------------------------------------------------------------------------------------------ 2 - 4, 7. the model
LENS = [256, 100, 30, 200]
CFG = {"uncond": dict(dim=64, depth=2), "cond": dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}


def _build(name, precision, seed=1):
    m = Model(**CFG[name], precision=precision)
    sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


@pytest.fixture(scope="module")
def uncond():
    """the unconditioned model in both precisions, its inputs, and the ragged forward -- computed once, shared, left unchanged"""
    x = make_input("x", (4, 256, 64), seed=2).to(DEV)
    t = make_input("times", (4,), seed=2, uniform=True).to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    out = {}
    for precision in ("exact", "hybrid"):
        m, sd = _build("uncond", precision)
        with torch.no_grad():
            out[precision] = (m, sd, m(x, t, lens=lens).clone())
    return dict(x=x, t=t, lens=lens, by=out)


def _edited(x, lens, seed, dim=1):
    """x with everything at or beyond each utterance's length (along `dim`) replaced by other finite random values"""
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(x.device) * 3
    keep = torch.arange(x.shape[dim], device=x.device)[None] < torch.as_tensor(lens, device=x.device)[:, None]
    keep = keep[:, :, None] if dim == 1 else keep[:, None, :]
    return torch.where(keep, x, other)


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_model_later_frames_cannot_be_seen(uncond, precision):
    m, _, y = uncond["by"][precision]
    x, t, lens = uncond["x"], uncond["t"], uncond["lens"]
    x2 = _edited(x, LENS, seed=70)
    assert not torch.equal(x2, x)
    with torch.no_grad():
        y2 = m(x2, t, lens=lens)
        leaky, leaky2 = m(x, t), m(x2, t)
    assert torch.isfinite(y).all() and torch.isfinite(y2).all()
    for i, n in enumerate(LENS):
        assert torch.equal(y2[i, :n], y[i, :n]), f"utterance {i}: frames before {n} changed with the frames behind them"
    for i, n in enumerate(LENS):
        if n < 256:                                       # without lengths the same edit reaches the frames before it
            assert not torch.equal(leaky2[i, :n], leaky[i, :n]), i


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_conditioned_guidance_batch_later_frames_cannot_be_seen(precision):
    """cond_scale 1.5 at B = 3: the one-batch guidance path doubles the lengths with x"""
    m, _ = _build("cond", precision)
    lens_l = LENS[:3]
    x = make_input("x", (3, 256, 64), seed=3).to(DEV)
    t = make_input("times", (3,), seed=3, uniform=True).to(DEV)
    prompt = make_input("prompt", (3, 7, 48), seed=3).to(DEV)
    cond = make_input("cond", (3, 48, 256), seed=3).to(DEV)
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    x2, cond2 = _edited(x, lens_l, seed=71), _edited(cond, lens_l, seed=72, dim=2)
    with torch.no_grad():
        y = m.forward_with_cond_scale(x, t, prompt=prompt, cond=cond, cond_scale=1.5, lens=lens).clone()
        y2 = m.forward_with_cond_scale(x2, t, prompt=prompt, cond=cond2, cond_scale=1.5, lens=lens).clone()
        leaky = m.forward_with_cond_scale(x, t, prompt=prompt, cond=cond, cond_scale=1.5).clone()
        leaky2 = m.forward_with_cond_scale(x2, t, prompt=prompt, cond=cond2, cond_scale=1.5).clone()
    assert torch.isfinite(y).all()
    for i, n in enumerate(lens_l):
        assert torch.equal(y2[i, :n], y[i, :n]), i
        if n < 256:
            assert not torch.equal(leaky2[i, :n], leaky[i, :n]), i


@pytest.mark.parametrize("precision,tol", [("exact", 1e-4), ("hybrid", 1e-3)])
def test_model_utterance_equals_the_oracle_alone(uncond, precision, tol):
    """tolerances: those of tests/test_model_gpu.py"""
    _, sd, y = uncond["by"][precision]
    x, t = uncond["x"].cpu(), uncond["t"].cpu()
    for i, n in enumerate(LENS):
        with torch.no_grad():
            ref = O.model_forward(sd, x[i:i + 1, :n], t[i:i + 1])
        e = rel(y[i:i + 1, :n].cpu(), ref)
        print(f"{precision} utterance {i} ({n} frames) vs the oracle alone: {e:.3e}")
        assert e < tol, (i, e)


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_two_chains_read_their_own_lengths(uncond, precision):
    m, _, y = uncond["by"][precision]
    lib = _lib.load()
    try:
        _lib.check(lib.ns2_debug_force_gemm(5), "ns2_debug_force_gemm")       # no split-K: the chain rule accepts 4 x 256 at dim 64
        _lib.check(lib.ns2_debug_force_chains(1), "ns2_debug_force_chains")
        with torch.no_grad():
            one = m(uncond["x"], uncond["t"], lens=uncond["lens"]).clone()
            ran_one = int(lib.ns2_debug_chains_last())
            _lib.check(lib.ns2_debug_force_chains(2), "ns2_debug_force_chains")
            two = m(uncond["x"], uncond["t"], lens=uncond["lens"]).clone()
            ran_two = int(lib.ns2_debug_chains_last())
        torch.cuda.synchronize()
    finally:
        lib.ns2_debug_force_chains(0)
        lib.ns2_debug_force_gemm(0)
    assert (ran_one, ran_two) == (1, 2)
    assert torch.equal(one, two)                           # chain 1 holds utterances 2 and 3: their own lengths, not chain 0's
    tol = 1e-4 if precision == "exact" else 1e-3           # (another GEMM hook than the fixture's forward: test_model_gpu.py's tolerances)
    assert all(rel(two[i, :n], y[i, :n]) < tol for i, n in enumerate(LENS))


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_no_lengths_and_full_lengths_change_nothing(uncond, precision):
    m, _, _ = uncond["by"][precision]
    x, t = uncond["x"], uncond["t"]
    with torch.no_grad():
        plain = m(x, t).clone()
        assert torch.equal(m(x, t, lens=None), plain)
        assert torch.equal(m(x, t, lens=torch.full((4,), 256, dtype=torch.int32, device=DEV)), plain)
        assert torch.equal(m(x, t, lens=[256] * 4), plain)
    m.train()
    try:
        with pytest.raises(NotImplementedError, match="lens"):
            m(x, t, lens=uncond["lens"])
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------ 5. the sampler
# Batch against solo over 8 DDIM steps.  The yardstick is the same comparison with no lengths involved, on the code before this feature:
# sample(length=256) of the batch [4, 256, 64] against each of its utterances sampled alone, worst utterance (a reduction-order effect:
# the solo run's GEMMs see another M).  Allowed: twice that.  Figures (profiles/ragged_sampling.json, "sampler_batch_vs_solo"):
#   exact:  yardstick 0.0 for every utterance, ragged batch vs solo at its own length 0.0 for every utterance
#   hybrid: yardstick 0.0 for every utterance, ragged batch vs solo at its own length 0.0 for every utterance
# The kernels are row-local with a fixed order of every sum, so a batch and its utterances alone agree bit for bit -- and twice nothing
# is nothing: the ragged batch has to agree bit for bit too, which it does (also where the solo run has 100 or 30 frames).
SAMPLER_YARDSTICK = {"exact": 0.0, "hybrid": 0.0}


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_sampler_ragged_batch(uncond, precision):
    m, _, _ = uncond["by"][precision]
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=8)
    noise = make_input("noise", (4, 256, 64), seed=5)
    out, lens = d.sample(length=LENS, batch_size=4, noise=noise, return_lens=True)
    assert out.shape == (4, 256, 64) and lens.tolist() == LENS and torch.isfinite(out).all()
    for i, n in enumerate(LENS):
        assert torch.count_nonzero(out[i, n:]) == 0 and torch.count_nonzero(out[i, :n]) > 0
    graph = d.sample(length=torch.tensor(LENS), batch_size=4, noise=noise, use_graph=True)
    assert torch.equal(graph, out)
    assert m.precision == precision                        # no demotion: the range guard saw nothing
    worst = 0.
    for i, n in enumerate(LENS):
        alone = d.sample(length=n, batch_size=1, noise=noise[i:i + 1, :n])
        e = rel(out[i:i + 1, :n], alone)
        print(f"{precision} utterance {i} ({n} frames): ragged batch vs alone over 8 steps {e:.3e}")
        worst = max(worst, e)
    assert worst <= 2 * SAMPLER_YARDSTICK[precision], (worst, SAMPLER_YARDSTICK[precision])


# ------------------------------------------------------------------------------------------------ 6. the codec
def test_codec_decoder_does_not_see_later_latent_frames():
    """sample() decodes the padded latents in one batch: right only if the 24 kHz SEANet decoder is causal, as seanet.py asserts"""
    tf = pytest.importorskip("transformers")
    from naturalspeech2_pytorch_amd import EncodecWrapperHIP
    torch.manual_seed(0)
    hf = tf.EncodecModel(tf.EncodecConfig()).eval().to(DEV)
    with torch.no_grad():
        codec = EncodecWrapperHIP.from_hf(hf, hip_seanet=True).to(DEV).eval()
        lens = [24, 9]
        emb = make_input("emb", (2, 24, 128), seed=6).to(DEV)
        a = codec.decode(emb).clone()
        b = codec.decode(_edited(emb, lens, seed=73)).clone()
    hop = codec.seq_len_multiple_of
    assert a.shape[-1] == 24 * hop
    for i, n in enumerate(lens):
        assert torch.equal(a[i, ..., :n * hop], b[i, ..., :n * hop]), i
    assert not torch.equal(a[1], b[1])
