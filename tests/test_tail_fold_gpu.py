"""The Wavenet tail fold (include/ns2hip.h): the sum of the last stack's skip convs and final_conv behind it (NS2:725) as ONE
Linear of K = L * dim.

  * op level: the fold kernel against torch.einsum in fp64;
  * model level: a folded model against the fp32 oracle under the ceilings of tests/test_parity_r2_gpu.py, the switch, the split-K route
    of a small batch, batches cut differently, and the content fingerprint.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, _lib  # noqa: E402
from oracle import ns2_oracle as O  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
SPLIT_K = 0                                   # ns2_debug_gemm_route_launches


def _force_gemm(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


def _force_tail(k):
    _lib.check(_lib.load().ns2_debug_force_tail_fold(k), "ns2_debug_force_tail_fold")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _fold(w_final, w_skip, b_skip, b_final):
    L, dim = b_skip.shape
    wf = torch.empty(dim, L * dim, dtype=torch.float32, device=DEV)
    bf = torch.empty(dim, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().ns2_tail_fold(w_final.data_ptr(), w_skip.data_ptr(), b_skip.data_ptr(), b_final.data_ptr(), dim, L, wf.data_ptr(),
                                        bf.data_ptr(), torch.cuda.current_stream().cuda_stream), "ns2_tail_fold")
    return wf, bf


# ---------------------------------------------------------------------------------------------- the fold kernel
@pytest.mark.parametrize("dim", [128, 512])
def test_fold_kernel_against_fp64_einsum(dim):
    """W'[n, l * dim + c] = sum_j W_final[n, j] W_skip[l][j, c], b' = W_final sum_l b_skip[l] + b_final: bit-identical from run to run,
    and under the bound tests/test_ff_fold_gpu.py sets for the feed-forward fold (10 x the 3.4e-7 measured for an fp32 sum of 1365 terms;
    the sums here have dim <= 512 terms)"""
    L = 8
    g = torch.Generator().manual_seed(dim + L)
    w_final = (torch.randn(dim, dim, generator=g) * dim ** -0.5).to(DEV)
    w_skip = (torch.randn(L, dim, dim, generator=g) * dim ** -0.5).to(DEV)
    b_skip, b_final = torch.randn(L, dim, generator=g).to(DEV), torch.randn(dim, generator=g).to(DEV)
    wf, bf = _fold(w_final, w_skip, b_skip, b_final)
    wf2, bf2 = _fold(w_final, w_skip, b_skip, b_final)
    assert torch.equal(wf, wf2) and torch.equal(bf, bf2)
    ref_w = torch.einsum("nj,ljc->nlc", w_final.double(), w_skip.double()).reshape(dim, L * dim)
    ref_b = w_final.double() @ b_skip.double().sum(0) + b_final.double()
    ew, eb = _rel(wf, ref_w), _rel(bf, ref_b)
    print(f"tail fold kernel dim {dim} L {L}: rel err W' {ew:.3e}, b' {eb:.3e}")
    assert ew < 3.4e-6 and eb < 3.4e-6, (ew, eb)


# ---------------------------------------------------------------------------------------------- the model
CEIL = {"exact": 1e-4, "mixed": 5e-4, "hybrid": 5e-4, "half": 5e-3}       # tests/test_parity_r2_gpu.py
ARCHS = [dict(dim=128, depth=2), dict(dim=512, depth=1)]
MODELS = [(kw, p) for kw in ARCHS for p in CEIL]
_REF = {}


def _setup(kw, B=2, seed=31):
    key = (tuple(sorted(kw.items())), B)
    if key not in _REF:                      # one oracle run per architecture and batch serves every plan
        m = Model(**kw)
        sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed)
        x = make_input("x", (B, 256, kw["dim"]), seed=seed + 1)
        t = make_input("times", (B,), seed=seed + 1, uniform=True)
        with torch.no_grad():
            ref = O.model_forward(sd, x, t)
        _REF[key] = (sd, x, t, ref)
    return _REF[key]


def _model(kw, sd, precision):
    m = Model(**kw, precision=precision)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _run(m, x, t):
    with torch.no_grad():
        return m(x.to(DEV), t.to(DEV)).clone()


@pytest.mark.parametrize("kw,precision", MODELS, ids=[f"d{k['dim']}-{p}" for k, p in MODELS])
def test_folded_model_against_the_oracle_and_the_switch(kw, precision):
    sd, x, t, ref = _setup(kw)
    m = _model(kw, sd, precision)
    try:
        _force_tail(1)
        y_on = _run(m, x, t)
        m.invalidate()                        # a second finalize with the fold on: stacking, fold and pack give the same W', b', the same bits
        y_on2 = _run(m, x, t)
        _force_tail(0)
        m.invalidate()
        y_off = _run(m, x, t)
        m.invalidate()                        # a second finalize with the fold off: the parent's arithmetic, the same bits
        y_off2 = _run(m, x, t)
    finally:
        _force_tail(1)
    e_on, e_off = _rel(y_on.cpu(), ref), _rel(y_off.cpu(), ref)
    diff = ((y_on.double() - y_off.double()).norm().item() / ref.double().norm().item())
    print(f"tail fold {kw} {precision}: vs oracle on {e_on:.3e} off {e_off:.3e}; on vs off {diff:.3e}")
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_on2), "two finalizes with the fold on differ"
    assert torch.equal(y_off, y_off2)
    assert not torch.equal(y_on, y_off), "the switch changed nothing"
    assert e_on < CEIL[precision], (precision, e_on)
    assert diff <= (e_on + e_off) * (1 + 1e-9), (diff, e_on, e_off)       # |on - off| <= |on - ref| + |off - ref|: no invented number


def _splits(M, N, k_tiles, fp32_epilogue):
    """1 if the planner splits K for this product (ns2_debug_splitk_plan: pure host arithmetic), else 0"""
    import ctypes
    S, c = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().ns2_debug_splitk_plan(M, N, k_tiles, k_tiles, int(fp32_epilogue), ctypes.byref(S), ctypes.byref(c)), "ns2_debug_splitk_plan")
    return int(S.value >= 2)


@pytest.mark.parametrize("kw", ARCHS, ids=[f"d{k['dim']}" for k in ARCHS])
def test_one_utterance_splits_k_in_the_folded_tail_and_still_matches(kw):
    """1 x 256 frames: 2 ... 8 output tiles, so the tail (K = 8 dim) splits K and runs the RMSNorm in its finishing launch; the folded step
    sends as many products fewer down the split-K route than the two-product step as the planner says (at dim 512 the skip sum and
    final_conv both split: one fewer; at dim 128 final_conv, K = 128, does not: as many)"""
    sd, x, t, ref = _setup(kw, B=1)
    lib = _lib.load()
    counts = {}
    try:
        for fold in (1, 0):
            _force_tail(fold)
            m = _model(kw, sd, "hybrid")
            _run(m, x, t)                     # (finalize, and whatever a first forward sets up)
            n0 = lib.ns2_debug_gemm_route_launches(SPLIT_K)
            y = _run(m, x, t)
            counts[fold] = lib.ns2_debug_gemm_route_launches(SPLIT_K) - n0
            if fold:
                y_on = y
    finally:
        _force_tail(1)
    dim = kw["dim"]
    tail, skip, final = _splits(256, dim, 8 * dim // 32, True), _splits(256, dim, 8 * dim // 32, False), _splits(256, dim, dim // 32, True)
    assert tail and skip, "the planner no longer splits the tail at 1 x 256"
    assert counts[1] > 0 and counts[0] - counts[1] == skip + final - tail, (counts, tail, skip, final)
    e = _rel(y_on.cpu(), ref)
    print(f"tail fold {kw} 1 x 256: split-K products {counts}, vs oracle {e:.3e}")
    assert e < CEIL["hybrid"], e


def test_folded_model_computes_the_same_rows_however_the_batch_is_cut():
    """a batch cut in halves and a one-utterance batch: the same rows, bit for bit, where every batch takes the same kernels
    (ns2_debug_force_gemm(5): the dedicated kernels whatever the size, never split K)"""
    kw = dict(dim=128, depth=2)
    m = Model(**kw, precision="hybrid")
    sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=41)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    B, N = 4, 256
    x = make_input("x", (B, N, 128), seed=42).to(DEV)
    t = torch.full((B,), 0.37, device=DEV)
    try:
        _force_tail(1)
        _force_gemm(5)
        with torch.no_grad():
            y = m(x, t).clone()
            halves = torch.cat([m(x[:2], t[:2]), m(x[2:], t[2:])])
            one = m(x[1:2], t[1:2]).clone()
    finally:
        _force_gemm(0)
    assert torch.equal(halves, y)
    assert torch.equal(one, y[1:2])


def test_a_data_write_yields_a_new_fold():
    """ema_pytorch writes through `.data`: the content fingerprint re-finalizes, and W' is folded from the new weights"""
    kw = dict(dim=128, depth=2)
    sd, x, t, _ = _setup(kw)
    m = _model(kw, sd, "hybrid")
    y0 = _run(m, x, t)
    params = dict(m.named_parameters())
    params["wavenet.final_conv.weight"].data.mul_(1.5)
    params["wavenet.stacks.3.blocks.2.skip_conv.bias"].data.add_(0.25)
    assert m.refresh_weights() is True
    y1 = _run(m, x, t)
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref2 = O.model_forward(sd2, x, t)
    assert not torch.equal(y1, y0)
    assert _rel(y1.cpu(), ref2) < CEIL["hybrid"], _rel(y1.cpu(), ref2)
