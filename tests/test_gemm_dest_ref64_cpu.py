"""tests/gemm_dest_ref64.py checked without a GPU:

  * K_EMU: the plain fp32 restatements of the four arithmetics (`emulate`) stay at or under the pinned K of
    `|got - ref| <= K u_p A + half_ulp + 2^-120` at every input of the table (tests/test_gemm_dest_gpu.py takes its bounds from it),
    and no kernel bound exceeds the cap of 4;
  * the layout helpers: what an encoder of each format stores at `Dest.offsets` decodes to the value the parts stand for, and each
    checker flags a planted violation -- one sentinel overwritten in a guard row, in a pad column and in the V^T tail, one flipped bit
    inside the owned region, one store left out;
  * through ns2_debug_splitk_plan (host arithmetic): every case the table marks split-K plans at least 2 slices, every other one 1;
  * every dispatcher condition is made false by one table entry and true by another;
  * ns2_linear refuses ldo < split_col on the host, before it reads the weight.
"""
import ctypes

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib
from tests import gemm_dest_ref64 as G


def _linear_inputs():
    """the distinct inputs of the cases under the element bound: (precision, epilogue, rows, N, K, taps) -> a Case"""
    seen = {}
    for c in G.CASES:
        if c.variant in G.ELEMENT_BOUND.get(c.epi, ()):
            seen.setdefault((c.prec, c.epi, c.rows, c.N, c.K, G.taps_of(c)), c)
    return seen


@pytest.mark.parametrize("prec", [3, 4, 2, 1])
def test_k_emu(prec):
    worst, at = 0.0, None
    for (p, epi, rows, N, K, taps), c in _linear_inputs().items():
        if p != prec:
            continue
        x, w, b, r = G.inputs(c)
        a, wp = G.operand_parts(x, prec), G.operand_parts(G.flat_weight(w), prec)
        if taps > 1:
            a = {k: G.unfold_causal(v, rows[0], rows[1], taps) for k, v in a.items()}
        bias, resid = (b, r) if epi == "f32" else (b, None) if epi == "split" else (None, None)
        ref, A = G.product(a["seen"], G.flat_weight(w), bias, resid)
        k, i = G.k_of(G.emulate(a, wp, prec, bias, resid), ref, A, prec, "f32")
        if k > worst:
            worst, at = k, (epi, rows, N, K, taps, i)
    print(f"K_EMU precision {prec}: measured {worst:.3f} at {at}, pinned {G.K_EMU[prec]}, kernels get {G.k_gpu(prec)}")
    assert at is not None and worst <= G.K_EMU[prec]


def test_k_gpu_stays_under_the_cap():
    for prec in G.K_EMU:
        k = G.k_gpu(prec)
        assert 4 * G.K_EMU[prec] <= k <= G.K_CAP == 4 and k & (k - 1) == 0
    # what the cap means at K = 64 terms: one dropped term is about A / 64; the widest allowance (precision 1) stays a factor 2 under it
    assert max(G.k_gpu(p) * G.U_P[p] for p in G.U_P) <= 2.0 ** -7


def _encode(x, fmt):
    """fp32 values -> the bytes [..., nb] a kernel stores for them (csrc/ns2_common.h split2 / cvt2h / cvt2_h8)"""
    u8 = lambda t: t.contiguous().view(torch.uint8).reshape(*x.shape, -1)          # noqa: E731
    if fmt == "f32":
        return u8(x.float())
    if fmt == "f16":
        return u8(x.to(torch.float16))
    if fmt == "bf16d":
        return u8(x.to(torch.bfloat16))
    if fmt == "bf16":
        p = G.operand_parts(x, 3)
        return torch.cat((u8(p["hi"].to(torch.bfloat16)), u8(p["lo"].to(torch.bfloat16))), -1)
    p = G.operand_parts(x, 4)
    return torch.cat((u8(p["hi"].to(torch.float16)), u8(p["h8"].to(torch.float8_e5m2)), u8(p["l8"].to(torch.float8_e5m2))), -1)


def _seen(x, fmt):
    return {"f32": x.float(), "f16": x.to(torch.float16).float(), "bf16d": x.to(torch.bfloat16).float(),
            "bf16": G.operand_parts(x, 3)["seen"], "h8": G.operand_parts(x, 4)["seen"]}[fmt].double()


def _stored(case):
    """an arena on the host after a well-behaved kernel: every owned element written (zero bits beyond the values' columns)"""
    dests = G.destinations(case)
    ar = G.Arena(list(dests.values()))
    host = ar.bytes()
    vals = {}
    for name, d in dests.items():
        if not d.written:
            continue
        ncols = d.own_cols
        v = G.rnd(f"cpu_{name}_{d.rows}_{ncols}", (d.rows, ncols), 3.0)
        if case.epi not in ("f32", "qkv"):
            v[:, case.N:] = 0.0
        host[d.offsets(0, ncols).reshape(-1)] = _encode(v, d.fmt).reshape(-1)
        vals[name] = v
    return ar, dests, host, vals


LAYOUT_CASES = [c for c in G.CASES if c.hook == "gemm128" and c.rows == (2, 200) and c.variant != "P4" and c.N in (203, 200, 85, 384) and
                (c.epi, c.prec) in (("f32", 3), ("split", 3), ("split", 4), ("split", 2), ("split", 1), ("qkv", 3), ("qkv", 2), ("qkv", 1))]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: f"{c.epi}-p{c.prec}-N{c.N}-{c.variant}")
def test_layout_helpers_decode_and_flag_planted_violations(case):
    ar, dests, host, vals = _stored(case)
    before = ar.bytes()
    owned = ar.owned_mask()
    assert G.check_untouched(before, host, owned) == (0, -1)
    for name, v in vals.items():
        d = dests[name]
        reg = G.owned_region(host, d)
        assert reg.shape == (d.rows, d.own_cols, d.nb) and G.unstored(reg, d.fmt) == 0
        assert torch.equal(G.decode(reg, d.fmt), _seen(v, d.fmt))
        assert G.unstored(G.owned_region(before, d), d.fmt) == d.rows * d.own_cols      # the untouched arena reads as "nothing stored"
    out = dests["out"]

    def planted(offset):
        h = host.clone()
        h[offset] ^= 0x10
        return h

    # a guard row: the first byte behind the last physical row; the last byte in front of the region
    behind = out.base + out.phys_rows * out.row_bytes
    assert G.check_untouched(before, planted(behind), owned) == (1, behind)
    assert G.check_untouched(before, planted(out.base - 1), owned) == (1, out.base - 1)
    # a pad column: the first element behind the owned columns of row 0, where the stride leaves one
    if out.ld > out.own_cols:
        pad = int(G._offsets(out.fmt, out.base, out.ld, 1, out.own_cols, out.own_cols + 1, None)[0, 0, 0])
        assert G.check_untouched(before, planted(pad), owned) == (1, pad)
    # the V^T tail: key seq_len of feature 0 of utterance 0 (Q1 leaves more than the canonical round_up(seq_len, 32))
    if "vt" in dests:
        vt = dests["vt"]
        assert vt.ld > case.rows[1]
        tail = int(G._offsets(vt.fmt, vt.base, vt.ld, 1, case.rows[1], case.rows[1] + 1, None)[0, 0, 0])
        assert not owned[tail] and G.check_untouched(before, planted(tail), owned) == (1, tail)
    # the residual belongs to the call's inputs: a store into it is a violation although it holds no sentinel
    if "resid" in dests:
        r = dests["resid"]
        ar.put_f32(r, G.rnd("cpu_resid", (r.rows, r.own_cols)))
        b2 = ar.bytes()
        h2 = b2.clone()
        h2[r.base + 5] ^= 1
        assert G.check_untouched(b2, h2, owned) == (1, r.base + 5)
    # one flipped bit inside the owned region: invisible to the sentinels, seen by the bit comparison; one store left out
    inside = int(out.offsets(0, out.own_cols)[out.rows // 2, out.own_cols // 2, 0])
    flipped = planted(inside)
    assert G.check_untouched(before, flipped, owned) == (0, -1)
    assert not torch.equal(G.owned_region(flipped, out), G.owned_region(host, out))
    missing = host.clone()
    missing[out.offsets(0, out.own_cols)[3, 1]] = before[out.offsets(0, out.own_cols)[3, 1]]
    assert G.unstored(G.owned_region(missing, out), out.fmt) == 1


def test_split_k_cases_plan_slices_and_the_others_do_not():
    lib = _lib.load()
    n = {True: 0, False: 0}
    for c in G.CASES:
        if c.epi == "wavenet":          # never split (plan_gemm): there is no plan to ask for
            continue
        M = c.rows[0] * c.rows[1]
        N = 2 * G.rup(c.N, 32) if c.epi == "geglu" else c.N
        kpt = (c.K + 31) // 32
        S, per = ctypes.c_int(-1), ctypes.c_int(-1)
        _lib.check(lib.ns2_debug_splitk_plan(M, N, kpt * G.taps_of(c), kpt, int(c.epi == "f32"), ctypes.byref(S), ctypes.byref(per)), "plan")
        assert (S.value >= 2) == G.splits_k(c) and S.value >= 1, (c, S.value)
        n[G.splits_k(c)] += 1
    assert n[True] > 0 and n[False] > 0


def test_every_dispatcher_condition_is_made_true_and_false():
    true, false = set(), set()
    for c in G.CASES:
        assert G._WHY[c.variant] in c.why
        for name, v in G.conditions(c).items():
            if v is not None:
                (true if v else false).add(name)
    aligned = {"out_f & 15", "ldo_f & 3", "resid & 15", "ldr & 3", "out_hi & 15", "ldo_s & 31", "vt_hi & 15"}
    assert aligned | {"interior"} <= true & false
    assert "vt_ld & 7" in true and "vt_ld & 7" not in false             # ns2_linear refuses such a stride: no call reaches the dispatcher with it
    assert {"format " + f for f in ("f32", "f16", "bf16", "h8", "bf16d")} <= true
    assert {"route " + r for r in G.ROUTES} <= true
    # the variants are what they say: the strides and shifts of the issue's list
    g = G.f32_geometry
    assert g("D0", 203)["ldo_f"] == 204 and g("D1", 203)["ldo_f"] == 216 and g("D1", 203)["ldr"] == 208 and g("D2", 256)["ldo_f"] & 3 == 1
    assert g("D3", 32)["out_shift"] == 4 and g("D4", 48)["resid_shift"] == 4 and g("D4", 48)["ldr"] & 1 and g("D5", 48)["act"] == 1
    p = G.plane_geometry
    assert p("P1", 200)["ldo"] == 256 and p("P1", 85)["ldo"] == 128 and p("P2", 85)["ldo"] == 86 and p("P2", 200)["ldo"] % 32 == 8
    assert p("P3", 200)["shift"] == 8 and p("P4", 85)["ldo"] == 160 and p("P4", 256)["ldo"] == 288
    q = G.qkv_geometry
    assert q("Q1", 200, False) == dict(ldo=288, vt_ld=208, vt_shift=0, dense=False) and q("Q1", 255, True)["vt_ld"] == 288


def test_linear_refuses_overlapping_qkv_rows_before_it_reads_the_weight():
    """no GPU here and `w` is no weight: a refusal that came after the first read of *w, or after a device call, would not come back
    as this argument error"""
    lib = _lib.load()
    fake = 1 << 20
    block = _lib.LinearArgs(w=fake, a_hi=fake, a_lo=fake + 64, lda=64, M=64, precision=3, out_hi=fake, out_lo=fake + 64, ldo=32,
                            seq_len=32, split_col=64, vt_hi=fake, vt_lo=fake + 64, vt_ld=32)
    rc = lib.ns2_linear(ctypes.byref(block), None)
    msg = (lib.ns2_last_error() or b"").decode()
    assert rc == _lib.NS2_ERR_ARG and msg.startswith("ns2_linear:") and "ldo" in msg and "split_col" in msg, (rc, msg)
