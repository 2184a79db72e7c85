"""The float64 references of tests/backward_ref64.py, checked without a GPU:

  * every backward reference equals torch.autograd (float64) of its own forward formula at random inputs, to 1e-12 relative;
  * K_EMU: what a plain fp32 torch evaluation of the same formula makes of K in `|got - ref| <= K 2^-24 A + 2^-120` at the GPU test's
    own inputs (tests/test_backward_pointwise_gpu.py takes its bounds from this table) -- `EmuBackend` where it has the operation, a
    direct fp32 restatement for SiLU, the embedding gradient and the slot reduction.  Each test prints what it measured and asserts
    that it stays at or under the pinned value;
  * the plane formats' half-ulp (`fmt_half_ulp`) against the rounding helpers of tests/emu_backend.py;
  * the training entry points refuse bad arguments on the host, before any device call.
"""
import pytest
import torch

from naturalspeech2_pytorch_amd import _lib
from tests import backward_ref64 as R
from tests.emu_backend import EP, EmuBackend, _h8_parts

EB = EmuBackend()


def close(a, b, tol=1e-12):
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item() <= tol


def rnd64(name, shape, scale=1.0):
    return (R.rnd("cpu64_" + name, shape).double() * scale)


# ------------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("B,N,d", [(1, 5, 8), (3, 7, 12)])
def test_film_gate_reference_is_the_autograd_of_its_forward(B, N, d):
    h, film, dg = (rnd64(n, s).requires_grad_(g) for n, s, g in (("h", (B * N, d), True), ("film", (B, 2 * d), True), ("dg", (B * N, d), False)))
    out, _ = R.film_gate_fwd(h, film, B, N, d)
    (out * dg).sum().backward()
    (dh, _), (dfilm, _) = R.film_gate_bwd(dg, h.detach(), film.detach(), B, N, d)
    assert close(dh, h.grad) and close(dfilm, film.grad)


@pytest.mark.parametrize("M,f", [(1, 1), (6, 9)])
def test_geglu_reference_is_the_autograd_of_its_forward(M, f):
    pre, dh = rnd64("pre", (M, 2 * f), 2.0).requires_grad_(True), rnd64("dh", (M, f))
    out, _ = R.geglu_fwd(pre, f)
    (out * dh).sum().backward()
    assert close(R.geglu_bwd(dh, pre.detach(), f)[0], pre.grad)
    assert close(out.detach(), torch.nn.functional.gelu(pre[:, f:]).detach() * pre[:, :f].detach())


@pytest.mark.parametrize("with_gamma,with_cond", R.RMSNORM_COMBOS)
def test_rmsnorm_reference_is_the_autograd_of_its_forward(with_gamma, with_cond):
    B, N, d = 2, 5, 12
    x, dy, add = rnd64("x", (B * N, d)).requires_grad_(True), rnd64("dy", (B * N, d)), rnd64("add", (B * N, d))
    gamma = (1 + 0.2 * rnd64("g", (d,))).requires_grad_(True) if with_gamma else None
    cond = torch.cat((1 + 0.3 * rnd64("cg", (B, d)), 0.3 * rnd64("cb", (B, d))), -1).requires_grad_(True) if with_cond else None
    (R.rmsnorm_fwd(x, B, N, d, gamma, cond) * dy).sum().backward()
    det = lambda t: t.detach() if t is not None else None          # noqa: E731
    (dx, _), dcond, dgamma = R.rmsnorm_bwd(x.detach(), dy, B, N, d, det(gamma), det(cond))
    assert close(dx, x.grad)
    assert (dcond is None) == (not with_cond) and (dgamma is None) == (not with_gamma)
    if with_cond:
        assert close(dcond[0], cond.grad)
    if with_gamma:
        assert close(dgamma[0], gamma.grad)
    (dx2, a2), _, _ = R.rmsnorm_bwd(x.detach(), dy, B, N, d, det(gamma), det(cond), dx_add=add)
    assert torch.equal(dx2, dx + add) and bool((a2 >= dx2.abs()).all())


def test_silu_and_embedding_references_are_the_autograd_of_their_forwards():
    x, dy = rnd64("sx", (7, 5), 3.0).requires_grad_(True), rnd64("sdy", (7, 5))
    y, _ = R.silu_fwd(x)
    (y * dy).sum().backward()
    assert close(R.silu_bwd(dy, x.detach())[0], x.grad)
    assert close(y.detach(), torch.nn.functional.silu(x.detach()))
    rows, d, pad = 6, 4, 2
    ids = torch.tensor([0, -1, 5, 5, 2, -7, 3, 0])
    table, g = rnd64("tab", (rows, d)).requires_grad_(True), rnd64("eg", (8, d))
    (R.embedding_fwd(ids, table, pad) * g).sum().backward()
    ref, A = R.embedding_bwd(ids, g, rows, d, pad)
    assert close(ref, table.grad) and torch.equal(ref[1], torch.zeros(d, dtype=torch.float64)) and bool((A >= ref.abs()).all())
    assert close(ref[pad], g[1] + g[4] + g[5])                       # negative ids count as pad_id


def test_every_magnitude_bounds_its_reference():
    B, N, d = 3, 65, 64
    h, dg, film = R.film_inputs(B, N, d)
    x, dy, add, gamma, cond = R.rmsnorm_inputs(B, N, d)
    pre, dh = R.geglu_inputs(300, 33)
    sx, sdy = R.silu_inputs(257, 33)
    do, o = R.delta_inputs(2, 9, 3)
    pairs = [R.film_gate_fwd(h, film, B, N, d), *R.film_gate_bwd(dg, h, film, B, N, d), R.geglu_fwd(pre, 33), R.geglu_bwd(dh, pre, 33),
             *R.rmsnorm_bwd(x, dy, B, N, d, gamma, cond, add), R.silu_fwd(sx), R.silu_bwd(sdy, sx), R.attention_delta(do, o, 2, 9, 3),
             R.reduce_slices(*R.reduce_inputs(3, 9, 33))]
    for ref, A in pairs:
        assert ref.dtype == A.dtype == torch.float64 and bool(torch.isfinite(ref).all()) and bool((A >= ref.abs()).all())


# ------------------------------------------------------------------------------------------------ K_EMU
class _Worst:
    def __init__(self):
        self.k = {}

    def add(self, key, got, ref_a):
        self.k[key] = max(self.k.get(key, 0.0), R.k_of(got, *ref_a)[0])

    def settle(self):
        for key, v in self.k.items():
            print(f"K_EMU measured {key}: {v:.3f} (pinned {R.K_EMU[key]})")
        for key, v in self.k.items():
            assert v <= R.K_EMU[key], (key, v)


def test_k_emu_film_gate():
    w = _Worst()
    for B, N, d in R.FILM_CASES:
        h, dg, film = R.film_inputs(B, N, d)
        w.add("film_gate_fwd", EB.film_gate_fwd(h, film, N, d), R.film_gate_fwd(h, film, B, N, d))
        dh, dfilm = EB.film_gate_bwd(dg, h, film, B, N, d)
        rdh, rdfilm = R.film_gate_bwd(dg, h, film, B, N, d)
        w.add("film_gate_dh", dh, rdh)
        w.add("film_gate_dfilm", dfilm, rdfilm)
    w.settle()


def test_k_emu_geglu():
    w = _Worst()
    for f in R.GEGLU_F:
        for M in R.GEGLU_M:
            pre, dh = R.geglu_inputs(M, f)
            w.add("geglu_fwd", EB.geglu_fwd(pre, f).t[:, :f], R.geglu_fwd(pre, f))
            w.add("geglu_bwd", EB.geglu_bwd(dh, pre, f)[:, :2 * f], R.geglu_bwd(dh, pre, f))
    w.settle()


def test_k_emu_rmsnorm():
    w = _Worst()
    for B, N, d in R.RMSNORM_CASES:
        x, dy, add, gamma, cond = R.rmsnorm_inputs(B, N, d)
        for with_gamma, with_cond in R.RMSNORM_COMBOS:
            kw = dict(gamma=gamma if with_gamma else None, cond=cond if with_cond else None)
            for a in (None, add):
                dx, dcond, dgamma = EB.rmsnorm_bwd(x, dy, B, N, d, dx_add=a, **kw)
                rdx, rdcond, rdgamma = R.rmsnorm_bwd(x, dy, B, N, d, dx_add=a, **kw)
                w.add("rmsnorm_dx", dx, rdx)
                if with_cond:
                    w.add("rmsnorm_dcond", dcond, rdcond)
                if with_gamma:
                    w.add("rmsnorm_dgamma", dgamma, rdgamma)
    w.settle()


def plane_values(x, precision):
    """what operand planes of `precision` hold of fp32 x: bf16 hi + bf16 lo, resp. half + e5m2 of the 2^12-scaled remainder"""
    if precision == 4:
        h, l, _ = _h8_parts(x)
        return (h + l).float()
    hi = x.to(torch.bfloat16).float()
    return hi + (x - hi).to(torch.bfloat16).float()


def test_k_emu_attention_delta():
    w = _Worst()
    for H in R.DELTA_H:
        for Nq in R.DELTA_NQ:
            for B in R.DELTA_B:
                do, o = R.delta_inputs(B, H, Nq)
                for prec in (3, 4):
                    ov = plane_values(o, prec)
                    w.add("attention_delta", EB.attention_delta(do, EP(ov), B, H, Nq), R.attention_delta(do, ov, B, H, Nq))
    w.settle()


def test_k_emu_silu():
    w = _Worst()
    for C in R.SILU_C:
        for M in R.SILU_M:
            x, dy = R.silu_inputs(M, C)
            y, dx = R.silu_fwd_f32(x), R.silu_bwd_f32(dy, x)
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
            w.add("silu_fwd", y, R.silu_fwd(x))
            w.add("silu_bwd", dx, R.silu_bwd(dy, x))
    w.settle()


def test_k_emu_embedding_and_its_restated_order():
    w = _Worst()
    for rows in R.EMBED_ROWS:
        for d in R.EMBED_D:
            for M in R.EMBED_M:
                for kind in R.EMBED_IDS:
                    ids, pad, dy = R.embedding_inputs(rows, d, M, kind)
                    got = R.embedding_bwd_f32(ids, dy, rows, d, pad)
                    ref, A = R.embedding_bwd(ids, dy, rows, d, pad)
                    w.add("embedding_bwd", got, (ref, A))
                    if kind == "sparse" and rows > 1:
                        assert bool((A[1] == 0).all()) and bool((got[1] == 0).all())        # an untouched table row
                    if kind == "negatives":
                        assert bool((ids < 0).any())
    w.settle()


def test_k_emu_reduce_slices_and_its_restated_order():
    w = _Worst()
    for S in R.REDUCE_S:
        for inner in R.REDUCE_INNER:
            p, prev = R.reduce_inputs(3, S, inner)
            for acc in (None, prev):
                got = R.reduce_slices_f32(p, acc)
                w.add("reduce_slices", got, R.reduce_slices(p, acc))
                one = torch.cat([R.reduce_slices_f32(p[o:o + 1], acc[o:o + 1] if acc is not None else None) for o in range(3)])
                assert torch.equal(got, one)
    w.settle()
    # the order is what the text says: S = 9 -> group 0 holds slots 0 and 8, then the groups in order
    p = torch.tensor([1e8, 1.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0]).reshape(1, 9, 1)
    f = torch.float32
    want = torch.tensor(1e8, dtype=f) + torch.tensor(3.0, dtype=f)
    for v in (1.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0):
        want = want + torch.tensor(v, dtype=f)
    assert R.reduce_slices_f32(p).item() == want.item()


def test_gpu_bounds_are_derived_and_capped():
    for key in R.K_EMU:
        k = R.k_gpu(key)
        assert k <= R.K_CAP and (k & (k - 1)) == 0 and (k >= 4 * R.K_EMU[key] or k == R.K_CAP) and (k < 8 * R.K_EMU[key] or k == 1)


@pytest.mark.parametrize("precision", [3, 4])
def test_format_half_ulp_covers_the_rounding_helpers(precision):
    pre, _ = R.geglu_inputs(300, 341)
    v = torch.cat((R.geglu_fwd(pre, 341)[0].float().reshape(-1), torch.tensor([1.0, 1.0 + 2.0 ** -9, 3e-6, -5e-8, 2.0 ** -14, 1e-9, 0.0])))
    err = (plane_values(v, precision).double() - v.double()).abs()
    assert bool((err <= R.fmt_half_ulp(v.double(), precision)).all())
    # ... and what was rounded to a stored value lay within the half-ulp AT that value
    assert bool((err <= R.stored_half_ulp(plane_values(v, precision), precision)).all())


# ------------------------------------------------------------------------------------------------ host refusals
def test_training_pointwise_entries_refuse_bad_arguments_before_any_device_call():
    """Each call comes back non-zero with the launcher's own `invalid argument` (there is no GPU here: a call that got as far as a
    launch would name another error), and the dummy pointers are never dereferenced."""
    lib = _lib.load()
    p = [4096 * (i + 1) for i in range(8)]              # dummy, 16-byte aligned

    def refused(rc, launcher):
        msg = (lib.ns2_last_error() or b"").decode()
        return rc != 0 and launcher in msg and "invalid argument" in msg

    for outer, S, inner in ((65536, 4, 8), (2, 0, 8), (2, 4, 0)):
        assert refused(lib.ns2_reduce_slices(p[0], outer, S, inner, p[1], 0, None), "launch_reduce_slices")
    # SiLU: ld < C, a row stride that is no multiple of 4, a pointer that is not 16-byte aligned
    for x, ldx, out, ldo in ((p[0], 8, p[1], 12), (p[0], 12, p[1], 8), (p[0], 14, p[1], 12), (p[0], 12, p[1], 13), (p[0] + 4, 12, p[1], 12),
                             (p[0], 12, p[1] + 8, 12)):
        assert refused(lib.ns2_silu_fwd(x, ldx, 4, 10, out, ldo, None), "launch_silu_fwd")
    for dy, lddy, x, ldx, dx, lddx in ((p[0], 8, p[1], 12, p[2], 12), (p[0], 12, p[1], 8, p[2], 12), (p[0], 12, p[1], 12, p[2], 8),
                                       (p[0], 13, p[1], 12, p[2], 12), (p[0], 12, p[1], 12, p[2], 14), (p[0] + 4, 12, p[1], 12, p[2], 12),
                                       (p[0], 12, p[1] + 4, 12, p[2], 12), (p[0], 12, p[1], 12, p[2] + 8, 12)):
        assert refused(lib.ns2_silu_bwd(dy, lddy, x, ldx, 4, 10, dx, lddx, None), "launch_silu_bwd")

    def rms(d, cond=None, cpart=None):
        ld = (d + 3) // 4 * 4                           # a leading dimension the launcher accepts: the refusal is the rule on d (or on cond)
        return lib.ns2_rmsnorm_bwd(p[0], ld, p[1], ld, None, cond, 2 * d, 1, 8, d, None, p[2], ld, cpart, None, None)
    assert refused(rms(2052), "launch_rmsnorm_bwd") and refused(rms(66), "launch_rmsnorm_bwd")
    assert refused(rms(64, cond=p[3]), "launch_rmsnorm_bwd")
    assert refused(lib.ns2_embedding_bwd(p[0], 8, 5, p[1], 16, 5, 16, p[2], None), "launch_embedding_bwd")          # pad_id >= rows
    assert refused(lib.ns2_embedding_bwd(p[0], 8, 0, p[1], 15, 5, 16, p[2], None), "launch_embedding_bwd")          # lddy < d
    assert refused(lib.ns2_geglu_bwd(p[0], 32, p[1], 64, 4, 32, p[2], 63, None), "launch_geglu_bwd")               # lddp < 2 f
    assert refused(lib.ns2_film_gate_fwd(p[0], 68, p[1], 132, 4, 8, 66, p[2], 68, None), "launch_film_gate_fwd")    # d = 66
    # attention delta, H = 2: ldo < 64 H, ldo no multiple of 32, o_lo != o_hi + 32 elements (64 bytes)
    for o_lo, ldo in ((p[1] + 64, 96), (p[1] + 64, 144), (p[1] + 128, 128)):
        assert refused(lib.ns2_attention_delta(p[0], 128, p[1], o_lo, ldo, 1, 2, 8, p[2], 3, None), "launch_attn_delta")
