"""TEST INFRASTRUCTURE: the destinations of the GEMM family (csrc/gemm_epi_dispatch.h wave_tile_epilogue) -- the case table, the
sentinel arena, the float64 reference with the magnitude of its terms, and the element-wise bound that
tests/test_gemm_dest_ref64_cpu.py (here, no GPU) and tests/test_gemm_dest_gpu.py (on the MI355X) share.  Written from
include/ns2hip.h, csrc/ns2_common.h and the dispatcher's own conditions; nothing here comes from tests/emu_backend.py.

WHAT THE TABLE VARIES.  wave_tile_epilogue picks, per wave tile, a staged LDS epilogue or the generic per-value one from: whether
the tile is interior; the output format; whether the destination is aligned (`out_f & 15`, `ldo_f & 3`, `resid & 15`, `ldr & 3`,
`out_hi & 15`, `ldo_s & 31`, `vt_hi & 15`, `vt_ld & 7`); and the route (csrc/gemm_route.h).  CASES lists
(epilogue, precision, hook, row shape, N, K, destination variant), each entry with one line (`why`) naming the condition it makes
true or false; `conditions(case)` evaluates the conditions from the entry's geometry, and the CPU test asserts that every one is
made true by an entry and false by another.  (`vt_ld & 7` is the exception: ns2_linear refuses such a stride, so no call reaches
the dispatcher with it; the table can only make it true.)

SIZES.  Row shapes (B, n): (2, 256) interior tiles, and what the dedicated kernels need; (2, 200) a row edge, an utterance boundary
inside a wave tile, seq_len % 4 == 0 (the 8-byte V^T stores); (1, 255) seq_len & 3 != 0 (the scalar V^T stores).  K: 64 for the
element bound; 512 = 16 K tiles for every split-K case, the least the plane epilogues split at; 96 for the lean linear kernel; 64
per tap for the FF conv kernel.  N for fp32: 256, 203 (N % 4 != 0: the value-by-value tail of f32_store_rows<EDGE>), 32 (the narrow
power-of-two tile of the 128 x 128 kernel), 48 (no power of two: the generic path).  N for planes: 256, 200 (zeros through column
223), 85 (odd: the pair store zeroes only c_hi).  q | k | v: a_dim = 128, split_col = 256.  GEGLU: f = 128 and 85.  Wavenet: C = 256
(the lean block kernel needs N % 256 == 0) and 128.

DESTINATION VARIANTS.  Every output, and the residual, lies in ONE arena of 16-bit words that all hold SENT16 before the launch,
with 4 KiB in front of the first region and at least one row and 256 bytes behind each.
  fp32   D0 canonical: ldo_f = ldr = round_up(N, 4), bases 256-byte aligned;  D1 wide but aligned: ldo_f = round_up(N, 4) + 12,
         ldr = round_up(N, 4) + 4;  D2 ldo_f & 3 == 1;  D3 the out base moved by one float;  D4 out aligned, the resid base moved by
         one float and ldr odd;  D5 no bias, no residual, act = 1 (SiLU) at the canonical layout, D5u the same call at D2's layout
         (its partner for the bit comparison: an activated call never takes the whole-tile staged epilogue).
  planes P0 canonical: ldo = round_up(N, 32);  P1 ldo = min(round_up(N, 32) + 32, round_up(N, 128)): columns [N, ldo) must be zero
         bits (dropped where it equals P0);  P2 dense only (out_lo == NULL): ldo = round_up(N, 2), where that is no multiple of 32
         (N = 200 and 85);  P3 dense only: out_hi moved by 8 bytes;  P4 ldo = round_up(N, 128) + 32: wider than any route's column tiles reach,
         refused by ns2_linear / ns2_wavenet_block (see tests/test_gemm_dest_gpu.py for the evidence);  P0d the canonical layout
         in the dense format, where the precision's own format is interleaved lines (precision 1: dense bf16; precision 4: dense
         IEEE half through out_precision = 2): what P2 / P3 are compared with.
  qkv    Q0 canonical: ldo = split_col, vt_ld = round_up(seq_len, 32);  Q1 ldo = split_col + 32: the sentinel columns at or beyond
         split_col must survive; vt_ld = round_up(seq_len, 8) + 8 (dense V^T; interleaved hi / lo lines come in blocks of 32 keys:
         round_up(seq_len, 32) + 32): the sentinels in [seq_len, vt_ld) must survive;  Q2 dense only: vt_hi moved by 8 bytes;  Q0d as P0d.
  GEGLU takes P0, P0d, P3 (the ABI fixes ldo = round_up(f, 32)); Wavenet takes P0, P0d, P3, P4 (P1 equals P0 at C = 128 and 256).

THE REFERENCE AND THE BOUND.  product(a_seen, w, bias, resid) returns (ref, A), float64: ref = a w^T + bias + resid and
A = |a| |w|^T + |bias| + |resid|, on the operand values the kernel sees (ops.join(a)) and the fp32 weight.  Element by element

    |got - ref| <= K * u_p * A + half_ulp(ref, output format) + 2^-120                                           (*)

with u_p the rounding each arithmetic gives a TERM by construction:
    precision 3   2^-17   hi + lo of the weight is 2^-18 of it; the dropped lo.lo is 2^-18
    precision 4   2^-13   three first-order e5m2 terms of at most 2^-14 each
    precision 2   2^-11   the weight as IEEE half
    precision 1   2^-9    the weight as bf16
(*) applies to the LINEAR outputs: fp32 with bias and residual, planes with act = 0, q | k | v.  The activated (D5), GEGLU and
Wavenet outputs keep their value checks in tests/test_kernels_gpu.py; here they get bit identity across layouts and sentinels only.

K.  K_EMU[precision] is what a plain fp32 torch restatement of the arithmetic (`emulate`, from csrc/ns2_common.h and the
conventions of include/ns2hip.h) makes of K over the table's own inputs; test_gemm_dest_ref64_cpu.py measures it and asserts that
it stays at or under the pinned value.  The kernels get 4 * K_EMU rounded up to a power of two and never above 4 (`k_gpu`).  The cap
is a condition, not a measurement: at K = 64 one dropped or misplaced term moves an element by about A / 64 = 2^-6 A; precision 1
at K = 4 allows 2^-7 A -- the thinnest case --, precision 2 at K = 2 2^-10 A, precision 3 at K = 4 2^-15 A, precision 4 at K = 2 2^-12 A.
"""
import functools
from collections import namedtuple

import torch

from tests.backward_ref64 import FLOOR, fmt_half_ulp, rup
from tests.golden.gen import make_input

SENT16 = 0x7FA5                 # as bf16 / IEEE half a NaN with a payload no conversion produces; two of them: the fp32 NaN 0x7FA57FA5
K_CAP = 4
U_P = {3: 2.0 ** -17, 4: 2.0 ** -13, 2: 2.0 ** -11, 1: 2.0 ** -9}
# Worst K of `emulate` over every input of the table, as test_gemm_dest_ref64_cpu.py::test_k_emu prints it (in brackets), pinned at
# the next half above it; -> the kernels' K (k_gpu)
K_EMU = {
    3: 1.0,        # [0.63]  -> 4   (q | k | v, K = 64)
    4: 0.5,        # [0.21]  -> 2
    2: 0.5,        # [0.40]  -> 2
    1: 1.0,        # [0.82]  -> 4
}

ROUTES = ("SplitK", "Tile128", "Tile256", "FfConv3", "Linear3", "Wavenet3")          # the order of csrc/gemm_route.h GemmRoute
# hook -> (ns2_debug_force_gemm mode, the route the canonical call takes, K of the product (per tap), needs lent split-K scratch)
HOOKS = {
    "gemm128": (1, "Tile128", 64, False),
    "gemm256": (2, "Tile256", 64, False),
    "splitk": (0, "SplitK", 512, True),
    "linear3": (5, "Linear3", 96, False),          # tile_linear() at precision 4
    "ffconv3": (5, "FfConv3", 64, False),          # tile_conv3() at precision 2, taps 3, dilation 1
    "wavenet3": (5, "Wavenet3", 0, False),         # tile_wavenet() at precision 5 (K = C)
}
ROW_SHAPES = ((2, 256), (2, 200), (1, 255))
N_F32 = (256, 203, 32, 48)
N_PLANES = (256, 200, 85)
QKV_A, QKV_SPLIT = 128, 256
GEGLU_F = (128, 85)
WAVENET_C = (256, 128)
WAVENET_DIL = 2
F32_VARIANTS = ("D0", "D1", "D2", "D3", "D4", "D5", "D5u")
ELEMENT_BOUND = {"f32": ("D0", "D1", "D2", "D3", "D4"), "split": ("P0", "P0d", "P1", "P2", "P3"), "qkv": ("Q0", "Q0d", "Q1", "Q2")}

Case = namedtuple("Case", "epi prec hook rows N K variant why")


def k_gpu(precision):
    """the K of (*) for a kernel at `precision`: 4 * K_EMU rounded up to a power of two, never above 4"""
    k, p = 4.0 * K_EMU[precision], 1
    while p < k:
        p *= 2
    return min(p, K_CAP)


# ================================================================================================ formats
# "f32"; "bf16" / "h8": interleaved 128-byte lines of 32 logical columns ([hi 32 | lo 32] / [half 32 | e5m2 x 32 | e5m2 rem 32]);
# "f16" / "bf16d": one dense 16-bit plane
def is_lines(fmt):
    return fmt in ("bf16", "h8")


def out_format(epi, prec, dense):
    """the format a call of `epi` at `prec` writes; dense: out_lo (and vt_lo) == NULL where the precision's own format has lines"""
    if epi == "f32":
        return "f32"
    if prec == 2 or (epi == "qkv" and prec == 4):
        return "f16"
    if prec == 3:
        assert not dense
        return "bf16"
    if prec == 1:
        return "bf16d" if dense else "bf16"
    if dense:                       # precision 4 planes, dense IEEE half through out_precision = 2: the plain product only
        assert epi == "split"
        return "f16"
    return "h8"


def has_dense_twin(epi, prec):
    """the precision's own format is interleaved lines AND the call can also write a dense plane"""
    return prec == 1 or (prec == 4 and epi == "split")


def half_ulp(ref, fmt):
    """the largest rounding error of a stored element near `ref` (float64), by output format"""
    a = ref.abs()
    if fmt == "f32":
        return a * 2.0 ** -24
    if fmt == "bf16":
        return fmt_half_ulp(ref, 3)
    if fmt == "h8":
        return fmt_half_ulp(ref, 4)
    if fmt == "f16":
        return (a * 2.0 ** -11).clamp(min=2.0 ** -25)
    return a * 2.0 ** -8                                             # dense bf16: 8 significant bits


# ================================================================================================ the sentinel arena
class Dest:
    """One matrix inside the arena: element (r, c) of format `fmt` with row stride `ld` (logical columns) from byte offset `base`.
    rows: its logical rows (tokens); own_cols: the columns a kernel may write; vt = (seq_len, vt_rows): transposed planes
    [b][feature][key] with row stride ld, seen BY TOKEN: logical row b * seq_len + n, logical column = feature."""

    def __init__(self, name, fmt, ld, rows, own_cols, shift=0, vt=None, written=True):
        self.name, self.fmt, self.ld, self.rows, self.own_cols, self.shift, self.vt, self.written = name, fmt, ld, rows, own_cols, shift, vt, written
        self.base = -1                                               # set by Arena
        self.nb = 2 if fmt in ("f16", "bf16d") else 4                # bytes of one logical element

    @property
    def phys_rows(self):
        return self.rows if self.vt is None else self.rows // self.vt[0] * self.vt[1]

    @property
    def row_bytes(self):
        return self.ld * self.nb

    def offsets(self, c0, c1):
        """byte offsets [rows, c1 - c0, nb] of the logical columns [c0, c1) of every logical row"""
        return _offsets(self.fmt, self.base, self.ld, self.rows, c0, c1, self.vt)


@functools.lru_cache(maxsize=16)
def _offsets(fmt, base, ld, rows, c0, c1, vt):
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(c0, c1, dtype=torch.int64)[None, :]
    if vt is not None:                                               # token m, feature f -> row b * vt_rows + f, column n
        seq, vt_rows = vt
        r, c = (r // seq) * vt_rows + c, (r % seq).expand(rows, c1 - c0)
    if fmt == "f32":
        o = base + (r * ld + c) * 4
        return o[..., None] + torch.arange(4)
    if not is_lines(fmt):
        o = base + (r * ld + c) * 2
        return o[..., None] + torch.arange(2)
    line, j = base + r * ld * 4 + (c // 32) * 128, c % 32
    if fmt == "bf16":
        return torch.stack((line + 2 * j, line + 2 * j + 1, line + 64 + 2 * j, line + 64 + 2 * j + 1), -1)
    return torch.stack((line + 2 * j, line + 2 * j + 1, line + 64 + j, line + 96 + j), -1)


class Arena:
    """A buffer of 16-bit words, all SENT16, with one region per Dest: 4 KiB in front of the first, each base 256-byte aligned
    + its `shift`, and one row + 256 bytes of guard behind each.  `address(d)`: the raw address a call is given."""
    FRONT = 4096

    def __init__(self, dests, device="cpu"):
        cur = self.FRONT
        for d in dests:
            d.base = rup(cur, 256) + d.shift
            cur = d.base + d.phys_rows * d.row_bytes + d.row_bytes + 256
        self.dests, self.nbytes = list(dests), rup(cur, 256)
        self.buf = torch.full((self.nbytes // 2,), SENT16, dtype=torch.int16, device=device)

    def address(self, d):
        return self.buf.data_ptr() + d.base

    def bytes(self):
        """the arena's bytes on the host (a copy)"""
        return self.buf.to("cpu", copy=True).view(torch.uint8)

    def put_f32(self, d, values):
        """fill the owned rectangle of an fp32 region (the residual) with values [rows, own_cols]"""
        v = values.contiguous().cpu().view(torch.uint8).reshape(d.rows, d.own_cols, 4)
        host = self.bytes()
        host[d.offsets(0, d.own_cols).reshape(-1)] = v.reshape(-1)
        self.buf.copy_(host.view(torch.int16))

    def owned_mask(self):
        m = torch.zeros(self.nbytes, dtype=torch.bool)
        for d in self.dests:
            if d.written and d.own_cols > 0:
                m[d.offsets(0, d.own_cols).reshape(-1)] = True
        return m


def check_untouched(before, after, owned):
    """every byte outside the owned regions is what it was before the launch (the sentinel, or the residual's values): -> the number
    of changed bytes and the offset of the first.  Bytes are compared as integers: a stored NaN is a store."""
    bad = (before != after) & ~owned
    n = int(bad.sum())
    return n, (int(bad.nonzero()[0]) if n else -1)


def owned_region(host, d, c0=0, c1=None):
    """the bytes [rows, columns, nb] of the logical columns [c0, c1) (default: all the kernel owns) of Dest d, the same logical
    layout for every variant: interleaved lines and V^T (by token) included"""
    c1 = d.own_cols if c1 is None else c1
    return host[d.offsets(c0, c1).reshape(-1)].reshape(d.rows, c1 - c0, d.nb)


def unstored(region, fmt):
    """elements of a region whose leading word still is the sentinel: a store that did not happen"""
    if fmt == "f32":
        w = region.reshape(-1, 4).contiguous().view(torch.int32).reshape(-1)
        return int((w == (SENT16 << 16 | SENT16)).sum())
    w = region[..., :2].reshape(-1, 2).contiguous().view(torch.int16).reshape(-1)
    return int((w == SENT16).sum())


def decode(region, fmt):
    """stored bytes [rows, cols, nb] -> the values they hold, float64"""
    flat = region.reshape(-1, region.shape[-1]).contiguous()
    shape = region.shape[:-1]
    if fmt == "f32":
        return flat.view(torch.float32).reshape(shape).double()
    first = flat[:, :2].contiguous()
    if fmt in ("f16", "h8"):
        v = first.view(torch.float16).reshape(shape).double()
        if fmt == "h8":                                              # + e5m2 of the 2^12-scaled remainder (e5m2 = the top byte of a half)
            rem = torch.stack((torch.zeros_like(flat[:, 3]), flat[:, 3]), -1).contiguous().view(torch.float16).reshape(shape).double()
            v = v + rem / 4096
        return v
    v = first.view(torch.bfloat16).reshape(shape).double()
    if fmt == "bf16":
        v = v + flat[:, 2:].contiguous().view(torch.bfloat16).reshape(shape).double()
    return v


# ================================================================================================ geometry of a case
def f32_geometry(variant, N):
    """-> dict(ldo_f, ldr, out_shift, resid_shift (bytes), bias, resid, act)"""
    ld0 = rup(N, 4)
    g = dict(ldo_f=ld0, ldr=ld0, out_shift=0, resid_shift=0, bias=True, resid=True, act=0)
    if variant == "D1":
        g.update(ldo_f=ld0 + 12, ldr=ld0 + 4)
    elif variant == "D2":
        g.update(ldo_f=ld0 + 1)
    elif variant == "D3":
        g.update(out_shift=4)
    elif variant == "D4":
        g.update(resid_shift=4, ldr=ld0 + 1)
    elif variant in ("D5", "D5u"):
        g.update(bias=False, resid=False, act=1, ldo_f=ld0 + (1 if variant == "D5u" else 0))
    else:
        assert variant == "D0", variant
    return g


def plane_geometry(variant, N):
    """-> dict(ldo, shift (bytes), dense)"""
    if variant in ("P0", "P0d"):
        return dict(ldo=rup(N, 32), shift=0, dense=variant == "P0d")
    if variant == "P1":
        return dict(ldo=min(rup(N, 32) + 32, rup(N, 128)), shift=0, dense=False)
    if variant == "P2":
        return dict(ldo=rup(N, 2), shift=0, dense=True)
    if variant == "P3":
        return dict(ldo=rup(N, 32), shift=8, dense=True)
    assert variant == "P4", variant
    return dict(ldo=rup(N, 128) + 32, shift=0, dense=False)


def qkv_geometry(variant, seq_len, lines):
    """-> dict(ldo, vt_ld, vt_shift (bytes), dense); lines: V^T is written as interleaved hi / lo lines (blocks of 32 keys)"""
    g = dict(ldo=QKV_SPLIT, vt_ld=rup(seq_len, 32), vt_shift=0, dense=variant in ("Q0d", "Q2"))
    if variant == "Q1":
        g.update(ldo=QKV_SPLIT + 32, vt_ld=rup(seq_len, 32) + 32 if lines else rup(seq_len, 8) + 8)
    elif variant == "Q2":
        g.update(vt_shift=8)
    else:
        assert variant in ("Q0", "Q0d"), variant
    return g


def baseline_of(variant, variants):
    """the canonical run of the same format a variant's owned region is compared with bit for bit (`variants`: those of its group;
    where the precision's own format is dense there is no P0d / Q0d and P0 / Q0 is that run)"""
    if variant in ("D0", "D5", "P0", "P0d", "Q0", "Q0d"):
        return variant
    b = {"D5u": "D5", "P2": "P0d", "P3": "P0d", "Q2": "Q0d"}.get(variant, variant[0] + "0")
    return b if b in variants else b[:2]


def destinations(case):
    """The Dests of a case, in arena order: {"out": ..., "resid": ..., "vt": ...} (what the epilogue has).  A dense variant at a
    precision whose only format is dense (precision 2; q | k | v at 4) uses that format's canonical run as its baseline."""
    B, n = case.rows
    M = B * n
    if case.epi == "f32":
        g = f32_geometry(case.variant, case.N)
        d = {}
        if g["resid"]:                  # in front of the output: a residual read with the output's (larger) stride stays inside the arena
            d["resid"] = Dest("resid", "f32", g["ldr"], M, case.N, g["resid_shift"], written=False)
        d["out"] = Dest("out", "f32", g["ldo_f"], M, case.N, g["out_shift"])
        return d
    if case.epi == "qkv":
        lines = is_lines(out_format("qkv", case.prec, case.variant in ("Q0d", "Q2")))
        g = qkv_geometry(case.variant, n, lines)
        fmt = out_format("qkv", case.prec, g["dense"])
        return {"out": Dest("out", fmt, g["ldo"], M, QKV_SPLIT),
                "vt": Dest("vt", fmt, g["vt_ld"], M, QKV_A, g["vt_shift"], vt=(n, QKV_A))}
    g = plane_geometry(case.variant, case.N)
    fmt = out_format(case.epi, 4 if case.prec == 5 else case.prec, g["dense"])
    return {"out": Dest("out", fmt, g["ldo"], M, 0 if case.variant == "P4" else g["ldo"], g["shift"])}


def conditions(case):
    """the dispatcher's conditions as this entry's geometry makes them (None: the epilogue has no such operand).  Bases are taken
    modulo 256 bytes: an arena base is 256-byte aligned + the variant's shift."""
    d = destinations(case)
    for x in d.values():
        x.base = x.shift
    B, n = case.rows
    M = B * n
    c = dict.fromkeys(("out_f & 15", "ldo_f & 3", "resid & 15", "ldr & 3", "out_hi & 15", "ldo_s & 31", "vt_hi & 15", "vt_ld & 7"))
    c["interior"] = M % 128 == 0 and (case.N if case.epi != "geglu" else 2 * rup(case.N, 32)) % 64 == 0
    c["route " + HOOKS[case.hook][1]] = True
    c["format " + d["out"].fmt] = True
    if case.epi == "f32":
        c["out_f & 15"], c["ldo_f & 3"] = d["out"].base % 16 == 0, d["out"].ld % 4 == 0
        if "resid" in d:
            c["resid & 15"], c["ldr & 3"] = d["resid"].base % 16 == 0, d["resid"].ld % 4 == 0
    else:
        c["out_hi & 15"], c["ldo_s & 31"] = d["out"].base % 16 == 0, d["out"].ld % 32 == 0
        if "vt" in d:
            c["vt_hi & 15"], c["vt_ld & 7"] = d["vt"].base % 16 == 0, d["vt"].ld % 8 == 0
    return c


# ================================================================================================ the case table
_WHY = {
    "D0": "aligned, contiguous: interior tiles take the staged fp32 epilogue (al true)",
    "D1": "ldo_f != ldr, both & 3 == 0: al stays true, a kernel that confuses the two strides shows",
    "D2": "ldo_f & 3 == 1: al false through the out stride",
    "D3": "out_f & 15 == 4: al false through the out base",
    "D4": "resid & 15 == 4 and ldr & 3 == 1: al false through the residual alone",
    "D5": "act = 1: al false through the activation, no bias, no residual (the baseline of D5u)",
    "D5u": "act = 1 and ldo_f & 3 == 1: the same call as D5 on the per-value stores",
    "P0": "aligned, ldo = round_up(N, 32): planes() true",
    "P0d": "the dense format at the canonical layout: planes() true for PF_F16 / PF_BF16 (the baseline of P2 / P3)",
    "P1": "ldo > round_up(N, 32): zero bits in [N, ldo), some of them in wave tiles of their own",
    "P2": "ldo_s & 31 != 0: planes() false through the stride",
    "P3": "out_hi & 15 == 8: planes() false through the base",
    "P4": "ldo > round_up(N, 128): beyond every route's column tiles -- the call is refused",
    "Q0": "aligned: q | k through planes(), V^T through the LDS transpose where seq_len allows",
    "Q0d": "dense bf16 q | k and V^T (vt_lo == NULL) at the canonical layout (the baseline of Q2)",
    "Q1": "ldo > split_col and vt_ld > round_up(seq_len, 8): sentinels behind split_col and behind seq_len survive",
    "Q2": "vt_hi & 15 == 8: V^T leaves the LDS transpose through the base",
}
_ROWS_WHY = {(2, 256): "interior rows", (2, 200): "row edge, utterance boundary in a wave tile, seq_len % 4 == 0", (1, 255): "row edge, seq_len & 3 != 0"}


def _variants(epi, prec, N):
    if epi == "f32":
        return F32_VARIANTS
    p = 4 if prec == 5 else prec
    twin = has_dense_twin(epi, p)
    dense = twin or out_format(epi, p, False) in ("f16", "bf16d")      # a dense plane can be asked for
    if epi == "qkv":
        return ("Q0", "Q1") + (("Q0d",) if twin else ()) + (("Q2",) if dense else ())
    v = ["P0"]
    if epi == "split" and plane_geometry("P1", N)["ldo"] != rup(N, 32):
        v.append("P1")
    if twin:
        v.append("P0d")
    if dense:
        v += (["P2"] if epi == "split" and rup(N, 2) % 32 else []) + ["P3"]
    if epi == "wavenet":
        v.append("P4")
    if epi == "split":
        v.append("P4")
    return tuple(v)


def _build():
    cases = []
    for epi, widths in (("f32", N_F32), ("split", N_PLANES), ("qkv", (QKV_SPLIT + QKV_A,)), ("geglu", GEGLU_F), ("wavenet", WAVENET_C)):
        for prec in (3, 4, 2, 1, 5):
            for hook, (_, route, K, _) in HOOKS.items():
                if (prec == 5) != (hook == "wavenet3") or (hook == "wavenet3") != (epi == "wavenet" and prec == 5):
                    continue
                if hook == "linear3" and (prec != 4 or epi == "wavenet"):
                    continue
                if hook == "ffconv3" and (prec != 2 or epi not in ("f32", "split")):
                    continue
                if hook == "splitk" and epi == "wavenet":            # the Wavenet block is never split
                    continue
                for rows in ROW_SHAPES:
                    if hook in ("linear3", "ffconv3", "wavenet3") and rows != (2, 256):      # the dedicated kernels: whole 256-row tiles
                        continue
                    for N in widths:
                        if hook == "wavenet3" and N % 256:
                            continue
                        for v in _variants(epi, prec, N):
                            cases.append(Case(epi, prec, hook, rows, N, N if epi == "wavenet" else K, v,
                                              f"{_WHY[v]}; {_ROWS_WHY[rows]}; N = {N}; {route}"))
    return tuple(cases)


CASES = _build()


def groups():
    """the (epilogue, precision, hook) triples of the table, in order: one GPU test each"""
    seen = {}
    for c in CASES:
        seen.setdefault((c.epi, c.prec, c.hook), []).append(c)
    return seen


def canonical_route(case):
    """the route the table names for a canonical run: the hook's, except that an activated call (D5) is not eligible for the FF conv
    kernel (ffconv3_eligible: act == 0) and falls back by shape -- 512 rows are at most 64 blocks of 256 x 256: the 128 x 128 kernel"""
    return "Tile128" if case.hook == "ffconv3" and case.variant == "D5" else HOOKS[case.hook][1]


def taps_of(case):
    return 3 if case.hook == "ffconv3" else 1


def splits_k(case):
    """does the table mark this case split-K?"""
    return case.hook == "splitk"


# ================================================================================================ inputs, reference, bound
def rnd(name, shape, scale=1.0):
    return make_input("gemm_dest:" + name, tuple(shape), seed=31) * scale


def inputs(case):
    """x [M, K], w [N, K] (k = 3: [N, K, 3]; GEGLU: 2 f rows, [x | gate]) ~ N(0, 1 / K_total), bias [rows of w], resid [M, N] ~ N(0, 1);
    the same for every variant and precision of a shape, so one reference serves all variants of a group's shape"""
    B, n = case.rows
    M, taps = B * n, taps_of(case)
    rows_w = 2 * case.N if case.epi == "geglu" else case.N
    t = f"{M}_{rows_w}_{case.K}_{taps}"
    w = rnd("w_" + t, (rows_w, case.K, taps) if taps > 1 else (rows_w, case.K), (case.K * taps) ** -0.5)
    return rnd("x_" + t, (M, case.K)), w, rnd("b_" + t, (rows_w,)), rnd("r_" + t, (M, case.N))


def wavenet_inputs(case):
    """x [M, C], the dilated conv [C, C, 3] and res_conv [C, C, 1] weights, their biases [C], film [B, 2 C] = [1 + 0.3 N | 0.3 N]"""
    B, n = case.rows
    C, t = case.N, f"wn_{case.rows[0]}_{case.rows[1]}_{case.N}"
    film = torch.cat((1 + 0.3 * rnd("fg_" + t, (B, C)), 0.3 * rnd("fb_" + t, (B, C))), -1)
    return (rnd("x_" + t, (B * n, C)), rnd("wc_" + t, (C, C, 3), (3 * C) ** -0.5), rnd("wr_" + t, (C, C, 1), C ** -0.5),
            rnd("bc_" + t, (C,)), rnd("br_" + t, (C,)), film)


def unfold_causal(a, B, n, taps, dil=1):
    """[B n, C] -> [B n, taps C]: block t holds row m - (taps - 1 - t) dil of the same utterance, zeros in front of it
    (CausalConv1d); with w.permute(0, 2, 1).reshape(N, taps C) the conv is one product"""
    C = a.shape[1]
    x = a.reshape(B, n, C)
    out = torch.zeros(B, n, taps, C, dtype=a.dtype)
    for t in range(taps):
        s = (taps - 1 - t) * dil
        if s < n:
            out[:, s:, t] = x[:, :n - s]
    return out.reshape(B * n, taps * C)


def flat_weight(w):
    return w.permute(0, 2, 1).reshape(w.shape[0], -1) if w.ndim == 3 else w


def product(a_seen, w, bias=None, resid=None):
    """-> (ref, A), float64: ref = a w^T (+ bias) (+ resid), A = |a| |w|^T (+ |bias|) (+ |resid|)"""
    a, w = a_seen.double(), w.double()
    ref, A = a @ w.t(), a.abs() @ w.abs().t()
    if bias is not None:
        ref, A = ref + bias.double(), A + bias.double().abs()
    if resid is not None:
        ref, A = ref + resid.double(), A + resid.double().abs()
    return ref, A


def k_of(got, ref, A, precision, fmt):
    """the smallest K with which every element of `got` meets (*), and the flat index of the element that needs it; a non-finite
    element or an error where A = 0 gives inf"""
    got, ref, A = got.double().reshape(-1), ref.reshape(-1), A.reshape(-1)
    e = (got - ref).abs()
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    e = (e - half_ulp(ref, fmt) - FLOOR).clamp(min=0)
    k = torch.where(e > 0, e / (U_P[precision] * A), torch.zeros_like(e))
    i = int(k.argmax())
    return float(k[i]), i


# ---- the four arithmetics in plain fp32 torch (include/ns2hip.h "Conventions", csrc/ns2_common.h split2 / cvt2h / cvt2_h8)
def _e5m2(x):
    return x.clamp(-57344.0, 57344.0).to(torch.float8_e5m2).float()


def operand_parts(x, precision):
    """fp32 -> the parts an operand of `precision` is stored as, and the value they stand for (what ns2_join_f32 returns)"""
    x = x.float()
    if precision in (1, 3):
        hi = x.to(torch.bfloat16).float()
        if precision == 1:
            return dict(hi=hi, seen=hi)
        lo = (x - hi).to(torch.bfloat16).float()
        return dict(hi=hi, lo=lo, seen=hi + lo)
    if precision == 2:
        h = x.clamp(-65504.0, 65504.0).to(torch.float16).float()
        return dict(hi=h, seen=h)
    xc = x.clamp(-57344.0, 57344.0)
    h = xc.to(torch.float16).float()
    l8 = _e5m2((xc - h) * 4096.0)
    return dict(hi=h, h8=_e5m2(xc), l8=l8, seen=h + l8 / 4096.0)


def emulate(a, w, precision, bias=None, resid=None):
    """the product as the kernels of `precision` form it, in fp32: a, w = operand_parts(...); every partial product is an fp32
    matmul (the MFMA accumulates in fp32), then + bias, + resid.  3: hi.hi + lo.hi + hi.lo (lo.lo dropped); 4: the IEEE-half
    product + (e5m2(a) . e5m2(w_rem 2^12) + e5m2(a_rem 2^12) . e5m2(w)) 2^-12; 2: one IEEE-half product; 1: bf16 hi only"""
    y = a["hi"] @ w["hi"].t()
    if precision == 3:
        y = y + a["lo"] @ w["hi"].t() + a["hi"] @ w["lo"].t()
    elif precision == 4:
        y = y + (a["h8"] @ w["l8"].t() + a["l8"] @ w["h8"].t()) / 4096.0
    if bias is not None:
        y = y + bias
    if resid is not None:
        y = y + resid
    return y
