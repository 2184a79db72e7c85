"""The destinations of the GEMM family on the MI355X: every (epilogue, precision, hook) of tests/gemm_dest_ref64.py's table runs its
row shapes, widths and destination variants through ns2_linear / ns2_wavenet_block with addresses from a sentinel arena
(csrc/gemm_epi_dispatch.h picks the epilogue from exactly these: interior tile, format, alignment, route).  Per group:

  * the canonical run (D0 / D5 / P0 / P0d / Q0 / Q0d) takes the route the table names (ns2_debug_gemm_route_launches);
  * every variant: each byte outside the rectangle the call owns is what it was before the launch -- guard rows, the columns between N
    and ldo_f, the columns at or beyond split_col, the keys in [seq_len, vt_ld), the residual; no owned element is left unstored;
    plane columns [N, ldo) are zero bits;
  * a variant that took its canonical run's route stores the same bits; where the route differs (a misaligned destination makes
    ffconv3_eligible false and the product falls back) the route is printed and only the element bound applies;
  * the linear outputs (fp32 with bias and residual, planes with act = 0, q | k | v) meet, element by element,
    |got - ref| <= K u_p A + half_ulp + 2^-120 with the K of gemm_dest_ref64.k_gpu.  The activated (D5), GEGLU and Wavenet outputs keep
    their value checks in tests/test_kernels_gpu.py and get bit identity and sentinels here.

The worst K per (epilogue, precision) goes to tests/parity_record under "gemm_dest/<epi>_p<prec>".

THE CONTRACT HOLE (P4: ldo = round_up(N, 128) + 32 on ns2_linear planes and on ns2_wavenet_block).  WHICH WAY IT WENT: refused.
EVIDENCE: reading alone -- the call was never run on a GPU with such a width.  set_out_planes sets out_ncols = ldo and GemmArgs
promises zeros in [N, out_ncols), but launch_one (gemm.hip) and splitk_finish_kernel start ceil(N / 128) column tiles, launch2_one
(gemm2.hip) and the lean kernels ceil(N / 256): with N = 85, ldo = 160 the 256-wide tile zeroes columns 128 .. 159 and the 128-wide
ones never reach them; with N = 200 or 256, ldo = 288 no route does.  The result depended on the route and the next GEMM would read
uninitialised K padding.  So ns2_linear and ns2_wavenet_block refuse ldo > round_up(N, 128) before any device call (capi.cpp),
launch_gemm refuses out_ncols > round_up(N, 128) for EPI_SPLIT / EPI_WAVENET from internal callers (gemm2.hip resolve_gemm_args), and
P4 asserts the refusal, that no route counter moved and that not one byte of the arena changed.  No caller in model_exec.cpp,
capi*.cpp or the Python layers passes such a width (read: dp = dim, a, fp = round_up(f, 32) and the Wavenet stack's out_ncols = dp
are all <= round_up(N, 128); ops.linear_split's callers leave ldo at round_up(rows, 32)).  Two more refusals of the same kind, both
also in tests/test_linear_abi_gpu.py: ldo < split_col in the q | k | v form (rows would overlap), and vt_ld % 32 != 0 with vt_lo
(the last interleaved line of a V^T row would overlap the next row; found while laying out Q1).

DEFECTS THE RUN EXPOSED: none in the kernels.  On the MI355X every variant of every group left every sentinel intact, stored every
owned element, wrote zero bits in [N, ldo) and, on the canonical run's route, the canonical run's bits.  The checks do bite: with
the generic fp32 epilogue reading the residual at ldo_f instead of ldr (a scratch change, reverted) D1, D2 and D4 failed on the
128 x 128 kernel and on the split-K finish (the 256 x 256 kernel never takes that epilogue for fp32 and passed).

RESULTS (MI355X): worst K of |got - ref| <= K u_p A + half_ulp + 2^-120 per (epilogue, precision), by hook, with its bound.
                  u_p     bound   gemm128  gemm256  splitk   linear3  ffconv3
    f32    p3     2^-17   4       0.453    0.453    0.154
    f32    p4     2^-13   2       0.151    0.151    0.049    0.113
    f32    p2     2^-11   2       0.326    0.326    0.147             0.203
    f32    p1     2^-9    4       0.963    0.963    0.389
    split  p3     2^-17   4       0.429    0.429    0.154
    split  p4     2^-13   2       0.142    0.142    0.043    0.104
    split  p2     2^-11   2       0.317    0.317    0.120             0.202
    split  p1     2^-9    4       1.065    1.065    0.426
    qkv    p3     2^-17   4       0.408    0.408    0.132
    qkv    p4     2^-13   2       0.121    0.121    0.043    0.095
    qkv    p2     2^-11   2       0.393    0.393    0.122
    qkv    p1     2^-9    4       1.373    1.373    0.443
(gemm128 / gemm256: K = 64; splitk: K = 512; linear3: K = 96; ffconv3: 3 taps of 64.)  Under the ffconv3 hook the variants D2, D3, D4
(fp32) and P2, P3 (planes) make ffconv3_eligible false and take the 128 x 128 kernel: printed as "another route", element bound only.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import _lib, ops  # noqa: E402
from tests import gemm_dest_ref64 as G  # noqa: E402
from tests import parity_record  # noqa: E402

DEV = torch.device("cuda:0")
GROUPS = G.groups()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _routes(lib):
    return [int(lib.ns2_debug_gemm_route_launches(i)) for i in range(len(G.ROUTES))]


class Shape:
    """what the variants of one (rows, N, K) of a group share: the packed weight, the operand planes, the inputs on the device and
    -- where the element bound applies -- the float64 reference, computed once"""

    def __init__(self, case):
        self.B, self.n = case.rows
        self.M = self.B * self.n
        self.op_prec = 4 if case.prec == 5 else case.prec
        self.taps = G.taps_of(case)
        self.ref = self.A = None
        if case.epi == "wavenet":
            x, wc, wr, bc, br, film = (t.to(DEV) for t in G.wavenet_inputs(case))
            self.w = ops.PackedWeight(wc, extra1x1=wr, precision=self.op_prec)
            if case.hook == "wavenet3":
                self.w.tile_wavenet()
            self.a = ops.split(x, precision=self.op_prec)
            self.bias, self.bias2, self.film = bc, br, film
            return
        x, w, b, r = G.inputs(case)
        self.w = ops.PackedWeight(w.to(DEV), geglu=case.epi == "geglu", precision=self.op_prec)
        if case.hook == "linear3":
            self.w.tile_linear()
        if case.hook == "ffconv3":
            self.w.tile_conv3()
        self.a = ops.split(x.to(DEV), ldo=ops.conv3_input_ld(case.K) if case.hook == "ffconv3" else None, precision=self.op_prec)
        self.bias = ops.geglu_pack_bias(b.to(DEV), case.N) if case.epi == "geglu" else b.to(DEV)
        self.resid = r
        if case.epi in G.ELEMENT_BOUND:
            a_seen = ops.join(self.a).cpu()[:, :case.K]
            if self.taps > 1:
                a_seen = G.unfold_causal(a_seen, self.B, self.n, self.taps)
            self.ref, self.A = G.product(a_seen, G.flat_weight(w), b if case.epi != "qkv" else None, r if case.epi == "f32" else None)


def launch(lib, case, sh):
    """one call with every destination in a fresh arena -> (rc, route or None, dests, bytes before, bytes after, owned mask)"""
    dests = G.destinations(case)
    arena = G.Arena(list(dests.values()), DEV)
    if "resid" in dests:
        arena.put_f32(dests["resid"], sh.resid)
    out = dests["out"]
    lo = lambda d: arena.address(d) + 64 if G.is_lines(d.fmt) else None          # noqa: E731
    before, r0 = arena.bytes(), _routes(lib)
    if case.epi == "wavenet":
        rc = lib.ns2_wavenet_block(sh.w.handle, sh.a.hi, sh.a.lo, sh.a.ld, sh.M, sh.n, G.WAVENET_DIL, sh.bias.data_ptr(), sh.bias2.data_ptr(),
                                   sh.film.data_ptr(), sh.film.shape[1], arena.address(out), lo(out), out.ld, case.prec, _stream())
    else:
        f = {}
        if sh.taps > 1:
            f.update(conv_taps=sh.taps, dilation=1, seq_len=sh.n, pad_left=-1)
        if case.epi == "f32":
            g = G.f32_geometry(case.variant, case.N)
            f.update(out_f32=arena.address(out), ldo_f=out.ld, act=g["act"], bias=sh.bias.data_ptr() if g["bias"] else None)
            if "resid" in dests:
                f.update(resid=arena.address(dests["resid"]), ldr=dests["resid"].ld)
        else:
            f.update(out_hi=arena.address(out), out_lo=lo(out), ldo=out.ld)
            if case.epi == "split":
                f.update(bias=sh.bias.data_ptr(), out_precision=2 if case.prec == 4 and out.fmt == "f16" else 0)
            elif case.epi == "geglu":
                f.update(bias=sh.bias.data_ptr())
            else:
                vt = dests["vt"]
                f.update(seq_len=sh.n, split_col=G.QKV_SPLIT, vt_hi=arena.address(vt), vt_lo=lo(vt), vt_ld=vt.ld)
        args = _lib.LinearArgs(w=sh.w.handle, a_hi=sh.a.hi, a_lo=sh.a.lo, lda=sh.a.ld, M=sh.M, precision=sh.op_prec, **f)
        rc = lib.ns2_linear(ctypes.byref(args), _stream())
    torch.cuda.synchronize()
    moved = [i for i, (x, y) in enumerate(zip(r0, _routes(lib))) if y != x]
    after = arena.bytes()
    return rc, (G.ROUTES[moved[0]] if len(moved) == 1 else None), dests, before, after, arena.owned_mask()


@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: f"{g[0]}-p{g[1]}-{g[2]}")
def test_destinations(group):
    epi, prec, hook = group
    lib = _lib.load()
    mode, _, _, lend = G.HOOKS[hook]
    op_prec = 4 if prec == 5 else prec
    bound = G.k_gpu(op_prec)
    worst, worst_at, other_routes, failures = 0.0, None, [], []      # every variant is judged: the failures of a group are listed together
    scratch = None
    _lib.check(lib.ns2_debug_force_gemm(mode), "ns2_debug_force_gemm")
    try:
        if lend:
            nbytes = int(lib.ns2_splitk_scratch_bytes())
            scratch = torch.full((nbytes // 4,), float("nan"), device=DEV)           # a slot read before it is written shows
            _lib.check(lib.ns2_debug_lend_splitk_scratch(scratch.data_ptr(), nbytes), "ns2_debug_lend_splitk_scratch")
        shapes = {}
        for c in GROUPS[group]:
            shapes.setdefault((c.rows, c.N, c.K), []).append(c)
        for cases in shapes.values():
            sh = Shape(cases[0])
            variants = [c.variant for c in cases]
            runs = {}
            for c in cases:
                tag = f"{epi} p{prec} {hook} rows {c.rows} N {c.N} K {c.K} {c.variant}"
                rc, route, dests, before, after, owned = launch(lib, c, sh)
                if c.variant == "P4":
                    msg = (lib.ns2_last_error() or b"").decode()
                    entry = "ns2_wavenet_block:" if epi == "wavenet" else "ns2_linear:"
                    if not (rc == _lib.NS2_ERR_ARG and msg.startswith(entry) and "ldo" in msg):
                        failures.append(f"{tag}: not refused as {entry} ... ldo ...: rc {rc}, {msg!r}")
                    if route is not None or not torch.equal(before, after):
                        failures.append(f"{tag}: a call that should have been refused launched ({route}) or wrote")
                    continue
                assert rc == 0, (tag, rc, (lib.ns2_last_error() or b"").decode())          # (a HIP error ends the group: nothing more is launched)
                nbad, first = G.check_untouched(before, after, owned)
                if nbad:
                    failures.append(f"{tag}: {nbad} bytes outside the owned region changed, the first at arena offset {first} (route {route})")
                regions = {}
                for name, d in dests.items():
                    if not d.written:
                        continue
                    reg = G.owned_region(after, d)
                    if G.unstored(reg, d.fmt):
                        failures.append(f"{tag}: {G.unstored(reg, d.fmt)} owned elements of {name} were not stored (route {route})")
                    regions[name] = reg
                out = dests["out"]
                if epi in ("split", "geglu", "wavenet") and out.ld > c.N:
                    if int(regions["out"][:, c.N:].count_nonzero()):
                        failures.append(f"{tag}: columns [N, ldo) are not zero bits (route {route})")
                base = G.baseline_of(c.variant, variants)
                if base == c.variant:
                    if route != G.canonical_route(c):
                        failures.append(f"{tag}: took {route}, the table says {G.canonical_route(c)}")
                    runs[c.variant] = (route, regions)
                else:
                    b_route, b_regions = runs[base]
                    if route == b_route:
                        for name, reg in regions.items():
                            w = min(reg.shape[1], b_regions[name].shape[1])        # (P1 / P2: another ldo, the same N value columns + zeros)
                            if not torch.equal(reg[:, :w], b_regions[name][:, :w]):
                                failures.append(f"{tag}: {name} differs from {base} in its bits (route {route})")
                    else:
                        other_routes.append(f"{tag}: {route} (canonical: {b_route})")
                if c.variant in G.ELEMENT_BOUND.get(epi, ()):
                    for name, reg in regions.items():
                        d = dests[name]
                        col0 = G.QKV_SPLIT if name == "vt" else 0
                        ncol = min(reg.shape[1], sh.ref.shape[1] - col0)
                        got = G.decode(reg[:, :ncol], d.fmt)
                        k, i = G.k_of(got, sh.ref[:, col0:col0 + ncol], sh.A[:, col0:col0 + ncol], op_prec, d.fmt)
                        if k > worst:
                            worst, worst_at = k, f"{tag} {name}[{i // ncol}, {i % ncol}]"
                        if not k <= bound:
                            failures.append(f"{tag}: {name}[{i // ncol}, {i % ncol}] needs K = {k:.3f} > {bound} (route {route})")
    finally:
        torch.cuda.synchronize()
        lib.ns2_debug_lend_splitk_scratch(None, 0)
        lib.ns2_debug_force_gemm(0)
        del scratch
    for line in other_routes:
        print("another route:", line)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])
    if epi in G.ELEMENT_BOUND:
        print(f"gemm_dest {epi} p{prec} {hook}: worst K {worst:.3f} (bound {bound}) at {worst_at}")
        key = f"gemm_dest/{epi}_p{prec}"
        rec = parity_record.load_current().get(key)
        rec = rec if isinstance(rec, dict) else {}
        rec.update({"bound_k": bound, "u_p": G.U_P[op_prec]})
        rec.setdefault("worst_k", {})[hook] = round(worst, 4)
        parity_record.record(key, rec)
