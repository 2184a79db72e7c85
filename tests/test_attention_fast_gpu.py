"""The two-block self-attention forward (csrc/attn_fast_kernel.h) against attn_kernel, the kernel it stands in for.

Both kernels do the same arithmetic in the same order, so wherever the new one takes a call (one IEEE-half product, head
dimension 64, whole 64-key tiles, whole 256-row workgroups, no mask) the packed outputs with the switch at 0 (by eligibility)
and at 1 (attn_kernel for every call, ns2_debug_force_attention) are equal bit for bit, and both meet test_attention's
tolerances against an fp64 softmax on the operand values the kernels see.  Calls the new kernel must not take give the same
bits either way because both settings run attn_kernel.  Which kernel a call took cannot be read from its output, so every case
also reads ns2_debug_attention_fast_launches() around each call: one more launch of the new kernel where it must take the call,
none where it must not.  Operands are built as in tests/test_kernels_gpu.py::test_attention.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, _lib, ops  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
QB = 256                                   # query rows per workgroup of attn_fast_kernel (AF_QB)
TOL = {2: 8e-4, 4: 5e-4}                   # test_attention's tolerances for the one-half-product precisions
FMT = {3: "bf16", 2: "f16", 4: "h8"}


def _force(k):
    _lib.check(_lib.load().ns2_debug_force_attention(k), "ns2_debug_force_attention")


def _fast_launches():
    return int(_lib.load().ns2_debug_attention_fast_launches())


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _asplit(x, prec, ldo=None):
    return ops.split(x, ldo=ldo, precision=2 if prec == 4 else prec)


def _operands(q, k, v, B, H, Nq, Nk, prec, D=64):
    a_dim = H * D
    vt_ld = ops.round_up(Nk, 32)
    vt_f = torch.full((B, a_dim, vt_ld), float("nan"), device=DEV)          # poisoned padding, as in test_attention
    vt_f[:, :, :Nk] = v.reshape(B, Nk, a_dim).transpose(1, 2)
    return _asplit(q, prec), _asplit(k, prec), _asplit(vt_f.reshape(B * a_dim, vt_ld), prec, ldo=vt_ld)


def _both(qp, kp, vt, B, H, Nq, Nk, prec, fast, **kw):
    """the packed output by eligibility (switch 0) and from attn_kernel (switch 1); `fast`: must switch 0 take the new kernel?"""
    try:
        _force(0)
        n0 = _fast_launches()
        new = ops.attention(qp, kp, vt, B, H, Nq, Nk, precision=prec, **kw)
        n1 = _fast_launches()
        _force(1)
        old = ops.attention(qp, kp, vt, B, H, Nq, Nk, precision=prec, **kw)
        n2 = _fast_launches()
        torch.cuda.synchronize()
    finally:
        _force(0)
    assert n1 - n0 == (1 if fast else 0), "switch 0: the call took the wrong kernel"
    assert n2 == n1, "switch 1: attn_fast_kernel took a call"
    assert new.fmt == old.fmt == FMT[prec]
    return new, old


def _ref64(qp, kp, vt, B, H, Nq, Nk):
    def heads(p, n):
        return ops.join(p).double().reshape(B, n, H, 64).permute(0, 2, 1, 3)
    ve = ops.join(vt).double().reshape(B, H * 64, vt.ld)[:, :, :Nk].reshape(B, H, 64, Nk).transpose(2, 3)
    s = torch.einsum("bhid,bhjd->bhij", heads(qp, Nq), heads(kp, Nk)) * 0.125
    return torch.einsum("bhij,bhjd->bhid", s.softmax(-1), ve).permute(0, 2, 1, 3).reshape(B * Nq, H * 64)


def _check(q, k, v, B, H, Nq, Nk, prec):
    qp, kp, vt = _operands(q, k, v, B, H, Nq, Nk, prec)
    new, old = _both(qp, kp, vt, B, H, Nq, Nk, prec, fast=True)
    assert torch.equal(new.buf, old.buf)
    got, ref = ops.join(new).double(), _ref64(qp, kp, vt, B, H, Nq, Nk)
    assert torch.isfinite(got).all()
    e = ((got - ref).norm() / ref.norm()).item()
    print(f"B{B} H{H} Nq{Nq} Nk{Nk} precision {prec}: rel err {e:.3e}")
    assert e < TOL[prec], f"rel err {e}"


@pytest.mark.parametrize("prec", [2, 4])
@pytest.mark.parametrize("B,H,Nq,Nk", [
    (1, 1, QB, 64),             # one tile: prologue and epilogue, no steady state
    (2, 3, QB, 192),            # an odd tile count: both stage parities; a head count that is no power of two
    (1, 8, 2 * QB, 1024),       # 16 tiles, two query tiles per head
    (3, 8, 2 * QB, 1024),       # 48 workgroups: a grid the XCD remap does not divide evenly
])
def test_fast_kernel_equals_attn_kernel_bit_for_bit(B, H, Nq, Nk, prec):
    a = H * 64
    _check(_rnd(B * Nq, a, seed=20), _rnd(B * Nk, a, seed=21), _rnd(B * Nk, a, seed=22), B, H, Nq, Nk, prec)


@pytest.mark.parametrize("prec", [2, 4])
@pytest.mark.parametrize("rising", [True, False])
def test_running_maximum_paths(rising, prec):
    """Four tiles that hold the SAME 64 keys times a factor per tile.  Every row's largest raw score is positive (64 random keys), so
    factors 1, 2, 3, 4 raise the running maximum of every row in every tile (alpha != 1 each time: O and l are rescaled), and
    factors 1, 1/2, 1/2, 1/2 leave it in tile 0 (alpha == 1 exactly: the skip is taken in tiles 1 ... 3)."""
    B, H, Nq, Nk = 1, 2, QB, 256
    a = H * 64
    base = _rnd(64, a, seed=31)
    fac = [1.0, 2.0, 3.0, 4.0] if rising else [1.0, 0.5, 0.5, 0.5]
    k = torch.cat([base * f for f in fac], 0)
    _check(_rnd(B * Nq, a, seed=30), k, _rnd(B * Nk, a, seed=32), B, H, Nq, Nk, prec)


@pytest.mark.parametrize("case", ["ragged_keys", "partial_query_tile", "key_mask", "head_dim_32", "precision_3"])
def test_calls_the_fast_kernel_must_not_take(case):
    """both switch settings run attn_kernel: same bits, and a finite result (the poisoned V^T padding stays masked)"""
    B, H, Nq, Nk, prec, D, kw = 2, 2, QB, 64, 2, 64, {}
    if case == "ragged_keys":
        Nk = 200
    elif case == "partial_query_tile":
        Nq = QB + 32
    elif case == "key_mask":
        mask = torch.rand(B, Nk, generator=torch.Generator().manual_seed(41)) > 0.4
        mask[0, :5] = False
        kw = dict(key_mask=mask.to(DEV))
    elif case == "head_dim_32":
        D, kw = 32, dict(head_dim=32)
    else:
        prec = 3
    a = H * D
    q, k, v = _rnd(B * Nq, a, seed=50), _rnd(B * Nk, a, seed=51), _rnd(B * Nk, a, seed=52)
    qp, kp, vt = _operands(q, k, v, B, H, Nq, Nk, prec, D=D)
    new, old = _both(qp, kp, vt, B, H, Nq, Nk, prec, fast=False, **kw)
    assert torch.equal(new.buf, old.buf)
    assert torch.isfinite(ops.join(new)).all()


def test_model_forward_is_bit_identical_with_and_without_the_fast_kernel():
    """the executor's call: q and k are column ranges of one q | k buffer, V^T has the executor's row length"""
    kw, B, N = dict(dim=128, depth=2), 2, 256
    m = Model(**kw, precision="hybrid")
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=3))
    m = m.to(DEV).eval()
    x = make_input("x", (B, N, kw["dim"]), seed=4).to(DEV)
    t = make_input("times", (B,), seed=4, uniform=True).to(DEV)
    with torch.no_grad():
        try:
            _force(0)
            n0 = _fast_launches()
            y_new = m(x, t).clone()
            n1 = _fast_launches()
            _force(1)
            y_old = m(x, t).clone()
            n2 = _fast_launches()
        finally:
            _force(0)
    assert n1 - n0 == kw["depth"], "one self-attention per layer takes the new kernel"
    assert n2 == n1
    assert torch.isfinite(y_new).all()
    assert torch.equal(y_new, y_old)
