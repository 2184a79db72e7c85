"""The pointwise and fixed-order reduction kernels of csrc/backward.hip on the MI355X, element by element against the float64
references of tests/backward_ref64.py:

    |got - ref| <= K 2^-24 A + 2^-120        A = the magnitude of the terms the formula adds (backward_ref64.py),
                                              K = 4 K_EMU rounded up to a power of two, never above 64 (backward_ref64.k_gpu)

reduce_slices_kernel, film_gate_fwd / _bwd, geglu_fwd / _bwd, rmsnorm_bwd_kernel<1 | 2 | 4 | 8>, attn_delta_kernel, silu_kernel<false | true>
and embedding_bwd_kernel, through the raw `ns2_*` entry points: every input has a row stride larger than its width with NaN beyond,
every output is prefilled with NaN and must still hold it wherever the contract says nothing is written (and in one guard row
behind the last).  The shapes are the smallest that reach each template instantiation, chunk boundary and pass of the kernels; the
lists, with the reason for every size, are in backward_ref64.py.  The two fixed-order sums (slot reduction, embedding gradient) must
also equal an fp32 restatement of their documented order bit for bit.

Worst K seen on an MI355X, per output (its bound), recorded as backward_pointwise/<output> through tests/parity_record.py on every run:
    reduce_slices 2.41 (16), embedding_bwd 3.62 (16), silu_fwd 2.38 (16), silu_bwd 3.35 (16), film_gate_fwd 3.53 (16),
    film_gate_dh 5.97 (64), film_gate_dfilm 5.28 (32), geglu_fwd 4.67 (64), geglu_bwd 7.24 (16), rmsnorm_dx 5.00 (32),
    rmsnorm_dcond 3.53 (16), rmsnorm_dgamma 3.42 (16), attention_delta 1.34 (8).
geglu_fwd's bound sits at the cap only because torch's own fp32 gelu is 9 ulp off near gate = 0.05 (K_EMU 10); gelu_erf with the plane
store needs 4.7, far below it.
The first run found one defect: film_gate_fwd needed K = 23.5 at B = 1, N = 255, d = 64 -- the gate's `1 - exp(-|z|)` lost the rounding of
the exponential near z = 0 (a relative error of 2e-5 at |z| = 1.4e-3); the kernel now takes that factor from expm1 and needs 3.5.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import ops, training  # noqa: E402
from naturalspeech2_pytorch_amd._lib import check  # noqa: E402
from tests import backward_ref64 as R  # noqa: E402
from tests.backward_ref64 import NAN, pad_cols, rup  # noqa: E402
from tests.parity_record import record  # noqa: E402

DEV = torch.device("cuda:0")
HB = {3: training.HipBackend(3), 4: training.HipBackend(4)}
lib = HB[3].lib
WORST = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinel(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def untouched(t):
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def bound(key, got, ref_a, what, extra=None):
    """assert (*) element by element with the output's K; print and record the worst K seen"""
    ref, A = ref_a
    got = got.cpu()
    assert got.shape == ref.shape, (key, what, got.shape, ref.shape)
    k, i = R.k_of(got, ref, A, extra)
    print(f"backward_pointwise/{key} {what}: K = {k:.3f} (bound {R.k_gpu(key)})")
    if k > WORST.get(key, -1.0):
        WORST[key] = k
        record(f"backward_pointwise/{key}", round(min(k, 1e30), 3))
    assert k <= R.k_gpu(key), (key, what, f"K = {k}", f"flat index {i}", got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), A.reshape(-1)[i].item())


def reduce_on_device(part, outer, S, inner, out, accumulate=0):
    check(lib.ns2_reduce_slices(part.data_ptr(), outer, S, inner, out.data_ptr(), accumulate, stream()), "ns2_reduce_slices")


# ------------------------------------------------------------------------------------------------ reduce_slices_kernel
@pytest.mark.parametrize("inner", R.REDUCE_INNER)
@pytest.mark.parametrize("S", R.REDUCE_S)
def test_reduce_slices(S, inner):
    """32 columns per workgroup (inner = 31 / 32 / 33), 8 row groups (S = 7 / 8 / 9: a group without a slot, one each, one with two)"""
    for outer in R.REDUCE_OUTER:
        p, prev = R.reduce_inputs(outer, S, inner)
        pd = p.to(DEV)
        for acc in (0, 1):
            what = f"outer={outer} S={S} inner={inner} accumulate={acc}"
            out = sentinel(outer + 1, inner)
            if acc:
                out[:outer] = prev.to(DEV)
            reduce_on_device(pd, outer, S, inner, out, acc)
            got = out[:outer].cpu()
            assert untouched(out[outer]), what
            bound("reduce_slices", got, R.reduce_slices(p, prev if acc else None), what)
            assert torch.equal(bits(got), bits(R.reduce_slices_f32(p, prev if acc else None))), what          # the documented order, bit for bit
            one = sentinel(outer, inner)
            if acc:
                one[:] = prev.to(DEV)
            for o in range(outer):
                reduce_on_device(pd[o], 1, S, inner, one[o], acc)
            assert torch.equal(bits(one.cpu()), bits(got)), what


# ------------------------------------------------------------------------------------------------ embedding_bwd_kernel
@pytest.mark.parametrize("d", R.EMBED_D)
@pytest.mark.parametrize("rows", R.EMBED_ROWS)
def test_embedding_bwd(rows, d):
    """a workgroup per table row and 256 columns (d = 255 / 256 / 257); dy with a row stride > d"""
    for M in R.EMBED_M:
        for kind in R.EMBED_IDS:
            what = f"rows={rows} d={d} M={M} ids={kind}"
            ids, pad, dy = R.embedding_inputs(rows, d, M, kind)
            dyd, idd = pad_cols(dy, d + 3).to(DEV), ids.to(DEV)
            runs = []
            for _ in range(2):
                dw = sentinel(rows + 1, d)
                check(lib.ns2_embedding_bwd(idd.data_ptr(), M, pad, dyd.data_ptr(), d + 3, rows, d, dw.data_ptr(), stream()), "ns2_embedding_bwd")
                assert untouched(dw[rows]), what
                runs.append(dw[:rows].cpu())
            got = runs[0]
            assert torch.equal(bits(got), bits(runs[1])), what
            bound("embedding_bwd", got, R.embedding_bwd(ids, dy, rows, d, pad), what)
            assert torch.equal(bits(got), bits(R.embedding_bwd_f32(ids, dy, rows, d, pad))), what            # ascending m, bit for bit
            hit = torch.zeros(rows, dtype=torch.bool)
            hit[torch.where(ids < 0, torch.full_like(ids, pad), ids)] = True
            assert bool((bits(got[~hit]) == 0).all()), what                                                   # untouched table rows: exactly zero
            if kind == "sparse" and rows > 1:
                assert not bool(hit.all())


# ------------------------------------------------------------------------------------------------ silu_kernel<false | true>
@pytest.mark.parametrize("C", R.SILU_C)
def test_silu_fwd_bwd(C):
    """a thread owns 4 columns: C = 4 / 512 float4 only, 1 / 3 the scalar tail only, 5 / 30 / 33 both; M = 257: more than one workgroup"""
    for M in R.SILU_M:
        what = f"M={M} C={C}"
        x, dy = R.silu_inputs(M, C)
        ldx, lddy, ldo = rup(C, 4) + 4, rup(C, 4) + 8, rup(C, 4) + 12
        xd, dyd = pad_cols(x, ldx).to(DEV), pad_cols(dy, lddy).to(DEV)
        y, dx = sentinel(M + 1, ldo), sentinel(M + 1, ldo)
        check(lib.ns2_silu_fwd(xd.data_ptr(), ldx, M, C, y.data_ptr(), ldo, stream()), "ns2_silu_fwd")
        check(lib.ns2_silu_bwd(dyd.data_ptr(), lddy, xd.data_ptr(), ldx, M, C, dx.data_ptr(), ldo, stream()), "ns2_silu_bwd")
        for name, out, ref_a in (("silu_fwd", y, R.silu_fwd(x)), ("silu_bwd", dx, R.silu_bwd(dy, x))):
            assert untouched(out[:M, C:]) and untouched(out[M]), (name, what)                                # columns >= C are not written
            assert bool(torch.isfinite(out[:M, :C]).all()), (name, what)
            bound(name, out[:M, :C], ref_a, what)


# ------------------------------------------------------------------------------------------------ film_gate_fwd / film_gate_bwd
@pytest.mark.parametrize("B,N,d", R.FILM_CASES)
def test_film_gate_fwd_bwd(B, N, d):
    what = f"B={B} N={N} d={d}"
    M = B * N
    h, dg, film = R.film_inputs(B, N, d)
    ldh, lddg, ldf, lddh = d + 4, d + 8, 2 * d + 4, d + 12
    hd, dgd, fd = pad_cols(h, ldh).to(DEV), pad_cols(dg, lddg).to(DEV), pad_cols(film, ldf).to(DEV)
    if d % 4 == 0:
        out = sentinel(M + 1, ldh)
        check(lib.ns2_film_gate_fwd(hd.data_ptr(), ldh, fd.data_ptr(), ldf, N, M, d, out.data_ptr(), ldh, stream()), "ns2_film_gate_fwd")
        assert untouched(out[:M, d:]) and untouched(out[M]), what
        bound("film_gate_fwd", out[:M, :d], R.film_gate_fwd(h, film, B, N, d), what)
    S = lib.ns2_film_gate_slices(N)
    assert S == (N + 255) // 256
    dh, part, dfilm = sentinel(M + 1, lddh), sentinel(B * S + 1, 2 * d), sentinel(B + 1, 2 * d)
    check(lib.ns2_film_gate_bwd(dgd.data_ptr(), lddg, hd.data_ptr(), ldh, fd.data_ptr(), ldf, B, N, d, dh.data_ptr(), lddh, part.data_ptr(),
                                stream()), "ns2_film_gate_bwd")
    reduce_on_device(part, B, S, 2 * d, dfilm)
    assert untouched(dh[:M, d:]) and untouched(dh[M]) and untouched(part[B * S]) and untouched(dfilm[B]), what
    rdh, rdfilm = R.film_gate_bwd(dg, h, film, B, N, d)
    bound("film_gate_dh", dh[:M, :d], rdh, what)
    bound("film_gate_dfilm", dfilm[:B], rdfilm, what)
    # the kernel's own slots: slot b * S + s holds the rows 256 s .. of utterance b, and their sum in the restated order is dfilm
    slots = part[:B * S].cpu().reshape(B, S, 2 * d)
    assert torch.equal(bits(dfilm[:B].cpu()), bits(R.reduce_slices_f32(slots))), what
    h3, dg3 = h.reshape(B, N, d), dg.reshape(B, N, d)
    for s in range(S):
        lo, hi = 256 * s, min(N, 256 * s + 256)
        _, rslot = R.film_gate_bwd(dg3[:, lo:hi].reshape(-1, d), h3[:, lo:hi].reshape(-1, d), film, B, hi - lo, d)
        bound("film_gate_dfilm", slots[:, s], rslot, f"{what} slot {s}")


# ------------------------------------------------------------------------------------------------ geglu_fwd / geglu_bwd
@pytest.mark.parametrize("M", R.GEGLU_M)
@pytest.mark.parametrize("f", R.GEGLU_F)
def test_geglu_fwd_bwd(f, M):
    what = f"M={M} f={f}"
    pre, dh = R.geglu_inputs(M, f)
    ldp, lddh, lddp, ldo = 2 * f + 5, f + 3, rup(2 * f, 32) + 7, rup(f, 32) + 32
    pred, dhd = pad_cols(pre, ldp).to(DEV), pad_cols(dh, lddh).to(DEV)
    ref, A = R.geglu_fwd(pre, f)
    for prec in (3, 4):
        out = ops._out_planes(M + 1, ldo, DEV, prec)
        out.buf.fill_(NAN)
        check(lib.ns2_geglu_fwd(pred.data_ptr(), ldp, M, f, out.hi, out.lo, ldo, prec, stream()), "ns2_geglu_fwd")
        j = ops.join(out).cpu()
        assert untouched(j[M]), (what, prec)
        assert bool((j[:M, f:] == 0).all()), (what, prec)                                                    # the planes are zero beyond f
        # the planes hold the fp32 result rounded as the format rounds: the format's half-ulp at the stored value on top of K
        hu = R.stored_half_ulp(j[:M, :f], prec)
        bound("geglu_fwd", j[:M, :f], (ref, A), f"{what} precision={prec}", extra=hu)
    dpre = sentinel(M + 1, lddp)
    check(lib.ns2_geglu_bwd(dhd.data_ptr(), lddh, pred.data_ptr(), ldp, M, f, dpre.data_ptr(), lddp, stream()), "ns2_geglu_bwd")
    assert untouched(dpre[:M, 2 * f:]) and untouched(dpre[M]), what                                          # columns >= 2 f are not written
    bound("geglu_bwd", dpre[:M, :2 * f], R.geglu_bwd(dh, pre, f), what)


# ------------------------------------------------------------------------------------------------ rmsnorm_bwd_kernel<1 | 2 | 4 | 8>
@pytest.mark.parametrize("B,N,d", R.RMSNORM_CASES)
def test_rmsnorm_bwd(B, N, d):
    """every combination of gamma / cond given or absent (neither: both partial pointers null) x dx_add absent, separate, aliased with dx"""
    M = B * N
    x, dy, add, gamma, cond = R.rmsnorm_inputs(B, N, d)
    ldx, lddy, lddx, ldc = d + 4, d + 8, d + 12, 2 * d + 4
    xd, dyd, addd = pad_cols(x, ldx).to(DEV), pad_cols(dy, lddy).to(DEV), pad_cols(add, lddx).to(DEV)
    gd, cd = gamma.to(DEV), pad_cols(cond, ldc).to(DEV)
    S = lib.ns2_rmsnorm_bwd_slices(N)
    assert S == (N + 63) // 64
    for with_gamma, with_cond in R.RMSNORM_COMBOS:
        kw = dict(gamma=gamma if with_gamma else None, cond=cond if with_cond else None)
        (rdx, adx), rdcond, rdgamma = R.rmsnorm_bwd(x, dy, B, N, d, **kw)
        for mode in ("absent", "separate", "aliased"):
            what = f"B={B} N={N} d={d} gamma={with_gamma} cond={with_cond} dx_add={mode}"
            dx = sentinel(M + 1, lddx)
            if mode == "aliased":
                dx[:M] = addd
            pa = None if mode == "absent" else (addd if mode == "separate" else dx).data_ptr()
            cpart = sentinel(B * S + 1, 2 * d) if with_cond else None
            gpart = sentinel(B * S + 1, d) if with_gamma else None
            check(lib.ns2_rmsnorm_bwd(xd.data_ptr(), ldx, dyd.data_ptr(), lddy, gd.data_ptr() if with_gamma else None,
                                      cd.data_ptr() if with_cond else None, ldc, B, N, d, pa, dx.data_ptr(), lddx,
                                      cpart.data_ptr() if with_cond else None, gpart.data_ptr() if with_gamma else None, stream()), "ns2_rmsnorm_bwd")
            assert untouched(dx[:M, d:]) and untouched(dx[M]), what
            ref_dx = (rdx, adx) if mode == "absent" else (rdx + add.double(), adx + add.double().abs())
            bound("rmsnorm_dx", dx[:M, :d], ref_dx, what)
            if with_cond:
                dcond = sentinel(B + 1, 2 * d)
                reduce_on_device(cpart, B, S, 2 * d, dcond)
                assert untouched(cpart[B * S]) and untouched(dcond[B]), what
                bound("rmsnorm_dcond", dcond[:B], rdcond, what)
            if with_gamma:
                dgamma = sentinel(2, d)
                reduce_on_device(gpart, 1, B * S, d, dgamma)
                assert untouched(gpart[B * S]) and untouched(dgamma[1]), what
                bound("rmsnorm_dgamma", dgamma[0], rdgamma, what)


# ------------------------------------------------------------------------------------------------ attn_delta_kernel
@pytest.mark.parametrize("prec", [3, 4])
@pytest.mark.parametrize("H", R.DELTA_H)
def test_attention_delta(H, prec):
    """H = 1 / 8: one 512-feature pass (8 / 64 lanes); 9 / 12: a second one in which only 8 / 32 lanes of a wave loop again; 16: two full;
    20: a third for 32 lanes.  Nq = 1 / 3 / 130: row counts that are no multiple of the 4 rows of a workgroup."""
    for Nq in R.DELTA_NQ:
        for B in R.DELTA_B:
            what = f"B={B} H={H} Nq={Nq} precision={prec}"
            M, a = B * Nq, 64 * H
            do, o = R.delta_inputs(B, H, Nq)
            dod = pad_cols(do, a + 4).to(DEV)
            op = HB[prec].split(o.to(DEV))                       # ld = 64 H + 32: a block of finite values behind the heads
            assert op.ld == a + 32 and op.precision == prec
            ov = ops.join(op).cpu()                              # the values the planes hold
            assert bool(((ov.double() - o.double()).abs() <= R.fmt_half_ulp(o.double(), prec)).all()), what
            delta = sentinel(B * H * Nq + 1)
            check(lib.ns2_attention_delta(dod.data_ptr(), a + 4, op.hi, op.lo, op.ld, B, H, Nq, delta.data_ptr(), prec, stream()), "ns2_attention_delta")
            assert untouched(delta[-1:]), what
            bound("attention_delta", delta[:-1].reshape(B, H, Nq), R.attention_delta(do, ov, B, H, Nq), what)
