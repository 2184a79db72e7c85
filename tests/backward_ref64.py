"""TEST INFRASTRUCTURE: float64 references of the pointwise and fixed-order reduction kernels of csrc/backward.hip, each with the
MAGNITUDE of the terms its formula adds, plus the inputs, shapes and bounds that tests/test_backward_ref64_cpu.py (here, no GPU) and
tests/test_backward_pointwise_gpu.py (on the MI355X) share.  Written from include/ns2hip.h and the kernels' comments; nothing here
comes from tests/emu_backend.py.

Every reference returns (ref, A), float64, element by element:
  ref   the formula as the header / the kernel comment states it;
  A     >= |ref|: the sum of the absolute values of the terms the formula adds.  A column sum over n has A = sum_n |term_n|;
        `1 - th * th` counts as `1 + th * th`, `1 - sg` as `1 + sg`, `Phi = 0.5 (1 + erf)` as `0.5 (1 + |erf|)`, and
        `dn - nh * dot` as `|dn| + |nh| * sum |nh dn| / d`.
With it the element-wise bound

    |got - ref| <= K * 2^-24 * A + 2^-120                                                                         (*)

means something where the result cancels (the `1 - tanh^2` tail, the zero of gelu', a column sum near zero): an fp32 evaluation
loses 2^-24 of every TERM, not of the result.  The floor 2^-120 covers results that underflow fp32.

One extension, for the FiLM gate's FORWARD: g = tanh(z) sigmoid(z) is a function of the sum z = h gamma + beta, whose rounding
(2^-24 of |h gamma| + |beta|) reaches g through g'(z); at z = 0 the result is 0 and the error is not.  Its A is therefore
|g| + |g'(z)| (|h gamma| + |beta|) -- first-order propagation of the terms of z.  The backward's A is the plain term count above.

K:  K_EMU[output] is what a plain fp32 torch evaluation of the same formula makes of K at the GPU test's own inputs (measured by
test_backward_ref64_cpu.py, which also asserts that the fp32 evaluation stays at or under the pinned value).  The kernels get
K = 4 * K_EMU rounded up to a power of two and never above 64 (`k_gpu`): the factor 4 pays for what they do and torch does not
(v_exp / v_rcp in the gate, erfc_fast's 1.2e-7, __expf, another but fixed summation order); the cap is a condition, not a measurement:
with the longest sum here (600 rows) one dropped term moves a column sum by about A / 600 = 1.7e-3 A, K = 64 allows 3.8e-6 A.
"""
import math

import torch

from tests.golden.gen import make_input

EPS = 2.0 ** -24
FLOOR = 2.0 ** -120
K_CAP = 64
NAN = float("nan")

# Worst K of the fp32 torch restatement over every case below, as test_backward_ref64_cpu.py::test_k_emu_* prints it (in brackets),
# pinned at the next half above it with some room for another CPU's vector math library; -> the kernels' K (k_gpu)
K_EMU = {
    "reduce_slices": 2.5,        # [2.41]  -> 16   (explicit IEEE adds: the same everywhere)
    "embedding_bwd": 4.0,        # [3.62]  -> 16
    "silu_fwd": 3.0,             # [2.42]  -> 16
    "silu_bwd": 4.0,             # [3.35]  -> 16
    "film_gate_fwd": 3.0,        # [2.55]  -> 16
    "film_gate_dh": 11.0,        # [10.39] -> 64
    "film_gate_dfilm": 7.5,      # [7.04]  -> 32   (N = 1: the column sum is one term of dh's kind)
    "geglu_fwd": 10.0,           # [9.08]  -> 64   (torch's fp32 gelu is 9 ulp off near gate = 0.05)
    "geglu_bwd": 4.0,            # [3.38]  -> 16
    "rmsnorm_dx": 6.5,           # [5.77]  -> 32
    "rmsnorm_dcond": 3.5,        # [3.23]  -> 16
    "rmsnorm_dgamma": 3.5,       # [3.03]  -> 16
    "attention_delta": 2.0,      # [1.54]  -> 8
}


def k_gpu(output):
    """the K of (*) for a kernel output: 4 * K_EMU rounded up to a power of two, never above 64"""
    k, p = 4.0 * K_EMU[output], 1
    while p < k:
        p *= 2
    return min(p, K_CAP)


def k_of(got, ref, A, extra=None):
    """the smallest K with which every element of `got` meets (*) (`extra`: a further absolute allowance per element, e.g. a format's
    half-ulp), and the flat index of the element that needs it; a non-finite element or an error where A = 0 gives inf"""
    got, ref, A = got.double().reshape(-1), ref.reshape(-1), A.reshape(-1)
    if got.numel() == 0:
        return 0.0, -1
    e = (got - ref).abs()
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    if extra is not None:
        e = e - extra.reshape(-1)
    e = (e - FLOOR).clamp(min=0)
    k = torch.where(e > 0, e / (EPS * A), torch.zeros_like(e))
    i = int(k.argmax())
    return float(k[i]), i


def rup(x, m):
    return (x + m - 1) // m * m


def pad_cols(t, ld, fill=NAN):
    """[M, C] -> [M, ld] with `fill` in the columns >= C: a row stride larger than the width, and nothing a kernel may read beyond it"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def rnd(name, shape, scale=1.0):
    return make_input("bwd_pointwise:" + name, tuple(shape), seed=29) * scale


# ================================================================================================ slot reduction
# out[o, j] (+)= sum_s partial[o, s, j]
def reduce_slices(partial, prev=None):
    p = partial.double()
    ref, A = p.sum(1), p.abs().sum(1)
    if prev is not None:
        ref, A = ref + prev.double(), A + prev.double().abs()
    return ref, A


def reduce_slices_f32(partial, prev=None):
    """the documented order in fp32, add by add (IEEE, no contraction possible: there is no product): eight partial sums over
    s = g, g + 8, ... in ascending s, then ((((((g0 + g1) + g2) + g3) + g4) + g5) + g6) + g7, then (accumulate) prev + that"""
    assert partial.dtype == torch.float32
    outer, S, inner = partial.shape
    grp = []
    for g in range(8):
        v = torch.zeros(outer, inner, dtype=torch.float32)
        for s in range(g, S, 8):
            v = v + partial[:, s]
        grp.append(v)
    t = grp[0]
    for g in range(1, 8):
        t = t + grp[g]
    return prev + t if prev is not None else t


REDUCE_S = (1, 7, 8, 9, 64, 513)
REDUCE_INNER = (1, 31, 32, 33, 1000)
REDUCE_OUTER = (1, 3)


def reduce_inputs(outer, S, inner):
    return rnd(f"rs_p_{outer}_{S}_{inner}", (outer, S, inner)), rnd(f"rs_o_{outer}_{S}_{inner}", (outer, inner))


# ================================================================================================ embedding gradient
def _ids(ids, pad_id):
    ids = ids.reshape(-1).long()
    return torch.where(ids < 0, torch.full_like(ids, pad_id), ids)


def embedding_fwd(ids, table, pad_id):
    return table.double()[_ids(ids, pad_id)]


def embedding_bwd(ids, dy, rows, d, pad_id):
    """dW[v, c] = sum over the tokens m with ids[m] == v (negative ids count as pad_id) of dy[m, c]"""
    g = dy[:, :d].double()
    i = _ids(ids, pad_id)
    ref = torch.zeros(rows, d, dtype=torch.float64).index_add_(0, i, g)
    A = torch.zeros(rows, d, dtype=torch.float64).index_add_(0, i, g.abs())
    return ref, A


def embedding_bwd_f32(ids, dy, rows, d, pad_id):
    """the ascending-m sequential fp32 sum, one explicit add per token"""
    assert dy.dtype == torch.float32
    i = _ids(ids, pad_id).tolist()
    dw = torch.zeros(rows, d, dtype=torch.float32)
    for m, v in enumerate(i):
        dw[v] = dw[v] + dy[m, :d]
    return dw


EMBED_ROWS = (1, 7, 300)
EMBED_D = (1, 255, 256, 257, 512)
EMBED_M = (1, 1000)
EMBED_IDS = ("negatives", "sparse", "equal")


def embedding_inputs(rows, d, M, kind):
    """-> (ids int64 [M], pad_id, dy [M, d]).  negatives: every id in [-3, rows); sparse: only ids = 0 mod 3 (the other table rows stay
    untouched); equal: one id, an M-term serial sum"""
    g = torch.Generator().manual_seed(1000 * rows + 10 * d + M)
    pad_id = rows // 2
    if kind == "negatives":
        ids = torch.randint(-3, rows, (M,), generator=g)
        if M >= 2:
            ids[0], ids[-1] = -1, -3
        else:
            ids[0] = -2
    elif kind == "sparse":
        ids = torch.randint(0, (rows + 2) // 3, (M,), generator=g) * 3
    else:
        ids = torch.full((M,), rows - 1, dtype=torch.int64)
    return ids.long(), pad_id, rnd(f"emb_dy_{rows}_{d}_{M}_{kind}", (M, d))


# ================================================================================================ SiLU
def silu_fwd(x):
    x = x.double()
    ref = x / (1 + torch.exp(-x))
    return ref, ref.abs()


def silu_bwd(dy, x):
    """dx = dy s (1 + x (1 - s)), s = 1 / (1 + exp(-x))"""
    dy, x = dy.double(), x.double()
    s = 1 / (1 + torch.exp(-x))
    return dy * s * (1 + x * (1 - s)), dy.abs() * s * (1 + x.abs() * (1 + s))


def silu_fwd_f32(x):
    return x / (1 + torch.exp(-x))


def silu_bwd_f32(dy, x):
    s = 1 / (1 + torch.exp(-x))
    return dy * s * (1 + x * (1 - s))


SILU_C = (1, 3, 4, 5, 30, 33, 512)
SILU_M = (1, 257)
SILU_EDGES = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e-40)


def silu_inputs(M, C):
    """x ~ N(0, 4^2) with the edge values down the first and the last column (the float4 path and the scalar tail), dy ~ N(0, 1)"""
    x, dy = rnd(f"silu_x_{M}_{C}", (M, C), 4.0), rnd(f"silu_dy_{M}_{C}", (M, C))
    e = torch.tensor(SILU_EDGES, dtype=torch.float32)
    if M >= len(SILU_EDGES):
        x[:len(e), 0] = e
        x[M - len(e):, C - 1] = e
    else:                                     # one row: one edge value per end, chosen by the width
        x[0, 0] = e[(2 + C) % len(e)]
        x[0, C - 1] = e[(5 + 3 * C) % len(e)]
    return x, dy


# ================================================================================================ FiLM + gate
def _gate_grad(z):
    """d/dz tanh(z) sigmoid(z) = (1 - th^2) sg + th sg (1 - sg), and its term magnitude"""
    th, sg = torch.tanh(z), torch.sigmoid(z)
    return (1 - th * th) * sg + th * sg * (1 - sg), (1 + th * th) * sg + th.abs() * sg * (1 + sg)


def _film(h, film, B, N, d):
    hh = h[:, :d].double().reshape(B, N, d)
    gam, bet = film[:, None, :d].double(), film[:, None, d:2 * d].double()
    return hh, gam, bet, hh * gam + bet


def film_gate_fwd(h, film, B, N, d):
    """out = tanh(z) sigmoid(z), z = h gamma_b + beta_b, film[b] = [gamma (d) | beta (d)]"""
    hh, gam, bet, z = _film(h, film, B, N, d)
    ref = torch.tanh(z) * torch.sigmoid(z)
    A = ref.abs() + _gate_grad(z)[0].abs() * ((hh * gam).abs() + bet.abs())
    return ref.reshape(-1, d), A.reshape(-1, d)


def film_gate_bwd(dg, h, film, B, N, d):
    """-> (dh, A), (dfilm [B, 2 d] = [dgamma | dbeta], A):  dh = dg g'(z) gamma ; dgamma[b] = sum_n dg g'(z) h ; dbeta[b] = sum_n dg g'(z)"""
    hh, gam, bet, z = _film(h, film, B, N, d)
    g1, a1 = _gate_grad(z)
    dgg = dg[:, :d].double().reshape(B, N, d)
    dz, adz = dgg * g1, dgg.abs() * a1
    dh, adh = dz * gam, adz * gam.abs()
    dfilm = torch.cat(((dz * hh).sum(1), dz.sum(1)), -1)
    adfilm = torch.cat(((adz * hh.abs()).sum(1), adz.sum(1)), -1)
    return (dh.reshape(-1, d), adh.reshape(-1, d)), (dfilm, adfilm)


# (B, N, d): FG_ROWS = 256 rows per chunk -> N = 255 / 256 / 257 / 600 = one partial chunk, one full, full + 1 row, two full + a partial one;
# 64 columns per workgroup -> d = 64 (one), 70 / 72 (a partial second; 70 for the backward only: the forward wants d % 4 == 0), 128, 512
FILM_CASES = tuple((B, N, d) for d in (64, 70, 72, 128, 512) for N in (1, 255, 256, 257, 600) for B in (1, 3))


def film_inputs(B, N, d):
    """h ~ 3 N(0, 1) with +-12 planted (gamma ~ 1: |z| reaches 12, where 1 - tanh^2 is all rounding), dg ~ N(0, 1), film = [1 + 0.3 N | 0.3 N]"""
    M = B * N
    t = f"{B}_{N}_{d}"
    h, dg = rnd("fg_h_" + t, (M, d), 3.0), rnd("fg_dg_" + t, (M, d))
    h[0, 0], h[M - 1, d - 1], h[M // 2, d // 2] = 12.0, -12.0, 9.0
    film = torch.cat((1 + 0.3 * rnd("fg_g_" + t, (B, d)), 0.3 * rnd("fg_b_" + t, (B, d))), -1)
    return h, dg, film


# ================================================================================================ GEGLU
def _geglu(pre, f):
    x, g = pre[:, :f].double(), pre[:, f:2 * f].double()
    erf = torch.erf(g / math.sqrt(2.0))
    return x, g, 0.5 * (1 + erf), 0.5 * (1 + erf.abs())


def geglu_fwd(pre, f):
    """h = gelu(gate) x, pre = [x (f) | gate (f)], gelu(g) = g Phi(g)"""
    x, g, Phi, aPhi = _geglu(pre, f)
    return g * Phi * x, g.abs() * aPhi * x.abs()


def geglu_bwd(dh, pre, f):
    """dpre[:, c] = dh gelu(gate) ; dpre[:, f + c] = dh x (Phi(gate) + gate phi(gate))"""
    x, g, Phi, aPhi = _geglu(pre, f)
    dy = dh[:, :f].double()
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    ref = torch.cat((dy * g * Phi, dy * x * (Phi + g * phi)), -1)
    A = torch.cat((dy.abs() * g.abs() * aPhi, dy.abs() * x.abs() * (aPhi + g.abs() * phi)), -1)
    return ref, A


def fmt_half_ulp(ref, precision):
    """the largest rounding error of an operand-plane element near `ref` (float64): precision 3 = bf16 hi + bf16 lo: the remainder of an
    8-bit hi is at most 2^(e - 8) and loses at most 2^-8 of that to its own 8 bits: 2^(e - 16) <= 2^-16 |ref|; precision 4 = IEEE half +
    e5m2 of the 2^12-scaled remainder: 2^(e - 11) of which 3 bits are kept: 2^(e - 14) <= 2^-14 |ref|, and below the half's normal range
    (ulp 2^-24) the remainder <= 2^-25 keeps 2^-28.  (The CPU test checks this against the rounding helpers of tests/emu_backend.py.)"""
    if precision == 3:
        return ref.abs() * 2.0 ** -16
    return (ref.abs() * 2.0 ** -14).clamp(min=2.0 ** -28)


def stored_half_ulp(got, precision):
    """the format's half-ulp AT a stored plane element `got` (fp32, = hi + lo exactly): whatever fp32 value was rounded to it lay within
    this distance.  precision 3: lo = got - bf16(got) is a bf16 with 8 significant bits: 2^(e_lo - 8); precision 4: the remainder
    (got - half(got)) 2^12 is an e5m2 with 3: 2^(e_l - 3) / 2^12, the spacing staying that of the smallest normal below it.  At a power of
    two this takes the wider side."""
    got = got.float()
    if precision == 3:
        lo = (got - got.to(torch.bfloat16).float()).double()
        return torch.exp2(torch.floor(torch.log2(lo.abs().clamp(min=2.0 ** -126))) - 8)
    l = (got - got.to(torch.float16).float()).double() * 4096
    return torch.exp2(torch.floor(torch.log2(l.abs().clamp(min=2.0 ** -14))) - 3) / 4096


GEGLU_F = (1, 31, 32, 33, 341, 1365)
GEGLU_M = (1, 300)
GEGLU_EDGES = (0.7518, -0.7518, 6.0, -6.0, 40.0, -40.0)


def geglu_inputs(M, f):
    """pre = [x | gate] ~ 3 N(0, 1) with the gate's edge values (+-0.7518: the zero of gelu'; +-6; +-40) down its first and last column; dh ~ N(0, 1)"""
    pre, dh = rnd(f"gg_pre_{M}_{f}", (M, 2 * f), 3.0), rnd(f"gg_dh_{M}_{f}", (M, f))
    e = torch.tensor(GEGLU_EDGES, dtype=torch.float32)
    if M >= len(e):
        pre[:len(e), f] = e
        pre[M - len(e):, 2 * f - 1] = e
    else:
        pre[0, f] = e[f % len(e)]
        pre[0, 2 * f - 1] = e[(f + 3) % len(e)]
    return pre, dh


# ================================================================================================ RMSNorm
def rmsnorm_fwd(x, B, N, d, gamma=None, cond=None):
    """y = nh gp gc + bc, nh = x r, r = sqrt(d) / max(|x|, 1e-12); cond[b] = [gc (d) | bc (d)]"""
    x = x[:, :d].double()
    r = math.sqrt(d) / x.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    y = x * r
    if gamma is not None:
        y = y * gamma.double()
    if cond is not None:
        c = cond.double()
        y = (y.reshape(B, N, d) * c[:, None, :d] + c[:, None, d:2 * d]).reshape(-1, d)
    return y


def rmsnorm_bwd(x, dy, B, N, d, gamma=None, cond=None, dx_add=None):
    """-> (dx, A), (dcond [B, 2 d], A) or None, (dgamma [d], A) or None:
    dx = (dx_add) + r (dn - nh (nh . dn) / d), dn = dy gc gp ; dgc[b] = sum_n dy nh gp ; dbc[b] = sum_n dy ; dgp = sum_m dy gc nh"""
    x, dy = x[:, :d].double(), dy[:, :d].double()
    r = math.sqrt(d) / x.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    nh = x * r
    gp = gamma.double() if gamma is not None else torch.ones(d, dtype=torch.float64)
    gc = cond[:, :d].double().repeat_interleave(N, 0) if cond is not None else torch.ones(1, d, dtype=torch.float64)
    dn = dy * gc * gp
    dot = (nh * dn).sum(-1, keepdim=True) / d
    adot = (nh * dn).abs().sum(-1, keepdim=True) / d
    dx, adx = r * (dn - nh * dot), r * (dn.abs() + nh.abs() * adot)
    if dx_add is not None:
        dx, adx = dx + dx_add[:, :d].double(), adx + dx_add[:, :d].double().abs()
    dcond = dgamma = None
    if cond is not None:
        t = (dy * nh * gp).reshape(B, N, d)
        dcond = (torch.cat((t.sum(1), dy.reshape(B, N, d).sum(1)), -1), torch.cat((t.abs().sum(1), dy.abs().reshape(B, N, d).sum(1)), -1))
    if gamma is not None:
        t = dy * gc * nh
        dgamma = (t.sum(0), t.abs().sum(0))
    return (dx, adx), dcond, dgamma


# (B, N, d): NB_ROWS = 64 rows per workgroup -> N = 63 / 64 / 65 / 200; a lane owns 4 columns of every 256 -> d <= 256 is <1>, <= 512 <2>,
# <= 1024 <4>, <= 2048 <8> (12 d floats of dynamic LDS: 96 KiB at 2048).  Every d meets N = 1 and N = 65.
RMSNORM_D = (64, 200, 256, 260, 512, 768, 1024, 1028, 2048)
RMSNORM_CASES = tuple((1, 1, d) for d in RMSNORM_D) + tuple((3, 65, d) for d in RMSNORM_D) + (
    (3, 63, 64), (1, 64, 200), (3, 200, 256), (1, 200, 260), (3, 64, 512), (3, 64, 768), (1, 63, 1024), (1, 63, 1028), (1, 200, 2048))
RMSNORM_COMBOS = ((False, False), (True, False), (False, True), (True, True))        # (gamma given, cond given)


def rmsnorm_inputs(B, N, d):
    """x, dy, add ~ N(0, 1); gamma = 1 + 0.2 N; cond = [1 + 0.3 N | 0.3 N].  From 4 rows on: row 1 of x is zero (the reference's
    max(|x|, 1e-12): r = sqrt(d) 1e12, a finite result), row 2 has norm 1e-20, row 3 is scaled by 1e4"""
    M = B * N
    t = f"{B}_{N}_{d}"
    x, dy, add = rnd("rn_x_" + t, (M, d)), rnd("rn_dy_" + t, (M, d)), rnd("rn_add_" + t, (M, d))
    if M >= 4:
        x[1] = 0.0
        x[2] = (x[2].double() / x[2].double().norm() * 1e-20).float()
        x[3] = x[3] * 1e4
    gamma = 1 + 0.2 * rnd("rn_g_" + t, (d,))
    cond = torch.cat((1 + 0.3 * rnd("rn_cg_" + t, (B, d)), 0.3 * rnd("rn_cb_" + t, (B, d))), -1)
    return x, dy, add, gamma, cond


# ================================================================================================ attention delta
def attention_delta(do, o, B, H, Nq):
    """delta[b, h, q] = sum_d dO[q, 64 h + d] O[q, 64 h + d], O = the values its operand planes hold"""
    p = (do[:, :64 * H].double() * o[:, :64 * H].double()).reshape(B, Nq, H, 64)
    return p.sum(-1).transpose(1, 2).contiguous(), p.abs().sum(-1).transpose(1, 2).contiguous()


# a lane owns 8 features, a wave 512 per pass: H <= 8 is one pass, 9 / 12 a second one for 8 / 32 lanes only, 16 two full, 20 a third for 32
DELTA_H = (1, 8, 9, 12, 16, 20)
DELTA_NQ = (1, 3, 130)
DELTA_B = (1, 2)


def delta_inputs(B, H, Nq):
    """dO [B Nq, 64 H] ~ N(0, 1); o [B Nq, 64 H + 32] ~ N(0, 1): the last 32 columns are a block of finite values the kernel must not read"""
    t = f"{B}_{H}_{Nq}"
    return rnd("ad_do_" + t, (B * Nq, 64 * H)), rnd("ad_o_" + t, (B * Nq, 64 * H + 32))
