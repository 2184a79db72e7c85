"""Two utterance chains (csrc/model_exec.cpp forward_impl): the row-dependent part of a step enqueued as two halves of the batch on
two streams gives the bits of the whole batch on one stream.

Every case runs the same forward with ns2_debug_force_chains(1) (one chain) and (2) (two chains wherever the chain rule allows),
compares the outputs with torch.equal and reads ns2_debug_chains_last() to see what really ran -- the outputs cannot tell.  The
small shapes used here split K by default (a product that splits K keeps one chain), so the cases that must run two chains switch
the split off with ns2_debug_force_gemm (5: the dedicated kernels whatever the size, as at the headline shape; 3: by shape).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, _lib  # noqa: E402
from naturalspeech2_pytorch_amd.model import _MODEL_PRECISIONS  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")


def _chains(k):
    _lib.check(_lib.load().ns2_debug_force_chains(k), "ns2_debug_force_chains")


def _gemm(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


def _last():
    return int(_lib.load().ns2_debug_chains_last())


def _model(**kw):
    m = Model(**kw)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def d512():
    return _model(dim=512, depth=1, precision="hybrid")


@pytest.fixture(scope="module")
def d64():
    return _model(dim=64, depth=2, precision="hybrid")


@pytest.fixture(scope="module")
def d64_cond():
    return _model(dim=64, depth=2, precision="hybrid", dim_prompt=64, condition_on_prompt=True)


def _rule(m, B, N):
    """the chain rule evaluated on the host for this model's configuration"""
    c = m._hip_cfg
    cfg = _lib.ModelConfig(dim=c["dim"], depth=c["depth"], dim_head=c["dim_head"], heads=c["heads"], ff_mult=c["ff_mult"],
                           wavenet_layers=c["wavenet_layers"], wavenet_stacks=c["wavenet_stacks"], dim_cond_mult=c["dim_cond_mult"],
                           condition_on_prompt=int(bool(c["condition_on_prompt"])), dim_prompt=int(c["dim_prompt"] or 0),
                           num_latents_m=c["num_latents_m"], resampler_depth=c["resampler_depth"], precision=_MODEL_PRECISIONS[m.precision])
    n = ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_chain_rule(ctypes.byref(cfg), B, N, ctypes.byref(n)), "ns2_debug_chain_rule")
    return n.value


def _both(fn, gemm, expect, rule):
    """fn() under one chain and under two-where-allowed; `expect`: the chains the second run must really have used, which is also
    what the host-only rule (ns2_debug_chain_rule) says for rule = (model, B, N) under the same GEMM hook"""
    try:
        _gemm(gemm)
        assert _rule(*rule) == expect
        _chains(1)
        one = fn()
        ran_one = _last()
        _chains(2)
        two = fn()
        ran_two = _last()
        torch.cuda.synchronize()
    finally:
        _chains(0)
        _gemm(0)
    assert ran_one == 1 and ran_two == expect, (ran_one, ran_two)
    assert torch.isfinite(one).all() and one.abs().max() > 0
    assert torch.equal(one, two)
    return one


def _xt(B, N, dim, seed=2):
    return make_input("x", (B, N, dim), seed=seed).to(DEV), make_input("times", (B,), seed=seed, uniform=True).to(DEV)


@pytest.mark.parametrize("precision", ["hybrid", "exact"])
@pytest.mark.parametrize("B", [2, 3])
def test_two_chains_equal_one_chain_d512(d512, precision, B):
    """d512 / depth 1 at B x 256 frames: one utterance per chain (B = 2), uneven chains 2 + 1 (B = 3); hybrid runs the dedicated kernels"""
    d512.precision = precision
    x, t = _xt(B, 256, 512)
    with torch.no_grad():
        _both(lambda: d512(x, t), gemm=5, expect=2, rule=(d512, B, 256))


def test_rule_refuses_where_the_whole_batch_splits_k(d64):
    """d64 / depth 2 at 4 x 256: the out-projection (K = 512) of the whole batch splits K, so force 2 still runs one chain"""
    x, t = _xt(4, 256, 64)
    with torch.no_grad():
        _both(lambda: d64(x, t), gemm=0, expect=1, rule=(d64, 4, 256))


def test_conditioned_model_offsets_into_the_cond_state(d64_cond):
    """prompt of 40 frames + aligned cond at 2 x 256: condadd, the cross-attention K / V^T and the prompt half of the conditioning
    projections are read per utterance"""
    x, t = _xt(2, 256, 64)
    prompt, cond = make_input("prompt", (2, 40, 64), seed=3).to(DEV), make_input("cond", (2, 64, 256), seed=3).to(DEV)
    with torch.no_grad():
        _both(lambda: d64_cond(x, t, prompt=prompt, cond=cond, cond_drop_prob=0.), gemm=3, expect=2, rule=(d64_cond, 2, 256))
        # the time table's row in place of the times: the hoisted time half + the per-utterance prompt half
        row = d64_cond.time_table(t[:1], 2)[0]
        _both(lambda: d64_cond(x, t, prompt=prompt, cond=cond, cond_drop_prob=0., cond_row=row), gemm=3, expect=2, rule=(d64_cond, 2, 256))


def test_cfg_as_one_batch_of_2b(d64_cond):
    """classifier-free guidance as one batch of [B conditioned | B null] utterances, B = 2: chains of 2 + 2"""
    x, t = _xt(2, 256, 64)
    prompt, cond = make_input("prompt", (2, 40, 64), seed=4).to(DEV), make_input("cond", (2, 64, 256), seed=4).to(DEV)
    with torch.no_grad():
        _both(lambda: d64_cond.forward_with_cond_scale(x, t, cond_scale=2.0, prompt=prompt, cond=cond), gemm=3, expect=2,
              rule=(d64_cond, 4, 256))


def test_times_and_cond_row_entry_points(d512):
    d512.precision = "hybrid"
    x, t = _xt(2, 256, 512)
    t = t[:1].expand(2).contiguous()                    # a table row stands for one time shared by the batch
    with torch.no_grad():
        by_times = _both(lambda: d512(x, t), gemm=5, expect=2, rule=(d512, 2, 256))
        try:
            _gemm(5)
            row = d512.time_table(t[:1], 2)[0]
        finally:
            _gemm(0)
        by_row = _both(lambda: d512(x, t, cond_row=row), gemm=5, expect=2, rule=(d512, 2, 256))
    assert torch.equal(by_times, by_row)


def test_captured_step_keeps_one_chain(d512):
    """a forward captured into a graph under force 2 runs one chain (no parallel branches in the graph); its replay equals eager"""
    d512.precision = "hybrid"
    x, t = _xt(2, 256, 512)
    try:
        _gemm(5)
        _chains(2)
        with torch.no_grad():
            eager = d512(x, t).clone()
            assert _last() == 2
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                y = d512(x, t)
            assert _last() == 1
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
        assert torch.equal(y, eager)
    finally:
        _chains(0)
        _gemm(0)


def test_profile_counts_logical_products(d512):
    """ns2_model_profile_begin / _end around one forward: `launches` is the number of products, one chain or two"""
    d512.precision = "hybrid"
    x, t = _xt(2, 256, 512)
    lib = _lib.load()
    h = d512._ensure_native().handle
    counts, ran = {}, {}
    try:
        _gemm(5)
        for k in (1, 2):
            _chains(k)
            with torch.no_grad():
                d512(x, t)                               # (warm: nothing of the timed forward is a first call)
                _lib.check(lib.ns2_model_profile_begin(h, 0xFF), "profile_begin")
                d512(x, t)
                ran[k] = _last()
                ms, n = ctypes.c_double(0), ctypes.c_int64(0)
                _lib.check(lib.ns2_model_profile_end(h, ctypes.byref(ms), ctypes.byref(n)), "profile_end")
            counts[k] = n.value
            assert ms.value > 0
    finally:
        _chains(0)
        _gemm(0)
    assert ran == {1: 1, 2: 2}
    assert counts[1] == counts[2] > 0, counts


def test_join_orders_the_callers_stream(d512):
    """two forwards back to back on a non-default stream, the second reading the first's output, then a read on that stream: only
    the stream is waited for, so the copy sees chain 1's rows only if the join ordered the caller's stream behind it"""
    d512.precision = "hybrid"
    x, t = _xt(2, 256, 512)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def run():
        with torch.no_grad(), torch.cuda.stream(s):
            y = d512(d512(x, t), t)
            z = y.clone()
        s.synchronize()
        return z

    _both(run, gemm=5, expect=2, rule=(d512, 2, 256))
