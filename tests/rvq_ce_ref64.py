"""TEST INFRASTRUCTURE: float64 reference of the RVQ cross-entropy term of the training loss (NS2:1668-1684; codec.py
`ResidualVQCrossEntropy`, csrc/rvq_ce.hip), with the MAGNITUDES its bound needs, and the cases that tests/test_rvq_ce_cpu.py (here, no
GPU) and tests/test_rvq_ce_gpu.py (on the MI355X) share.  Convention of tests/backward_ref64.py: every output comes with an A >= |ref|,
the sum of the absolute values of the terms its formula adds, and is held to

    |got - ref| <= K * 2^-24 * A + 2^-120                                                                         (*)

The reference, per quantizer q on the running residual r (direct form, float64):

    dist_c = sqrt(sum_k (r_k - e_ck)^2)      lse = log sum_c exp(-dist_c)      row_loss[m, q] = lse + dist_target
    p = softmax(-dist)    w_c = (p_c - [c = target]) / dist_c  (0 where dist_c = 0)    dL/dr = -sum_c w_c (r - e_c)
    r <- fp32(r - e_nearest)        the SAME fp32 subtraction the composite and the kernel perform, element by element (no summation
                                    order in it): the reference follows the fp32 residual instead of charging its rounding to the bound
    loss = sum_q mean_m row_loss      G = (1 / M) sum_q dL/dr_q      quantized_out = 0 + e_nearest_0 + e_nearest_1 + ... (fp32 adds, stage order)

Magnitudes:
    G          A = (1 / M) sum_q sum_c |w_c| (|r| + |e_c|), element-wise
    row_loss   A = |lse| + dist_target + first-order propagation of the rounding of the EXPANDED distance |r|^2 - 2 r.e + |e|^2 (what the
               fp32 composite, and the kernel's sweeps, evaluate): T_c / (2 dist_c) with T_c = |r|^2 + 2 sum_k |r_k e_ck| + |e_c|^2, through
               the log-sum-exp with its weights p_c, and once more for the target.  dist = 0 makes that inf: the expansion has no first order there.
    loss       A = (1 / M) sum of the row A's

Near-ties.  The nearest code is decided in fp32 by the code under test and in fp64 here; where the two best codes of a (row, stage) are
closer than fp32 resolves, either is a valid result, and everything after it in that row differs legitimately.  tie[m, q] = the fp64
top-2 margin in d^2, relative to the row's mean d^2 over the codes, is below TIE_MARGIN.  A row is compared up to its first tie stage:
`compared[m, q]` = no tie at any stage <= q (the tie stage itself is left out too: conservative).  G of a row needs every stage before
the last to be tie-free, quantized_out every stage.  At most MAX_LEFT_OUT of the (row, stage) pairs of a case may be left out -- asserted by
test_rvq_ce_cpu.py on the reference alone.  The scalar loss is compared against the reference's mean with the left-out pairs taken from the
tested row losses themselves.

K.  K_EMU[output] is what the existing fp32 composite, run on the CPU at these cases, makes of K (test_rvq_ce_cpu.py prints it and asserts
it stays under the pinned value).  The kernel gets 4 * K_EMU rounded up to a power of two and never above 64 (`k_gpu`): the factor pays
for another (fixed) summation order and for the MFMA's own accumulation order; the cap is a condition, not a measurement -- one dropped
code of C = 64 moves a row's softmax by about 1 / 64 of its terms, K = 64 allows 3.8e-6 of them.
"""
import torch

from tests.golden.gen import make_input

EPS = 2.0 ** -24
FLOOR = 2.0 ** -120
K_CAP = 64
TIE_MARGIN = 1e-5
MAX_LEFT_OUT = 0.01
D = 128

# name -> (b, n, Q, C, noise, targets)
CASES = {
    "a": (2, 37, 3, 128, 0.5, "nearest"),      # one partial workgroup, waves that have no rows
    "b": (3, 70, 8, 64, 0.1, "nearest"),       # one tile per stage; the second workgroup is partial
    "c": (1, 130, 2, 192, 1.0, "nearest"),     # an odd tile count: the ring's parity
    "d": (1, 16, 1, 1024, 0.5, "nearest"),     # the real codebook size
    "e": (1, 64, 2, 128, 0.5, "uniform"),      # the target is not the nearest code: y and the arg-max differ
}
SEED = 41

# Worst K of the fp32 composite over the cases, as test_rvq_ce_cpu.py::test_composite_within_k_emu prints it (in brackets), pinned at the
# next half above; -> the kernel's K (k_gpu)
K_EMU = {
    "row_loss": 1.0,     # [0.55]  -> 4
    "loss": 0.5,         # [0.21]  -> 2
    "G": 11.5,           # [11.43] -> 64 (46 rounded up; case d, C = 1024: the composite's autograd divides by the expanded distance;
                         #            11.43 or 11.21 with the number of threads the CPU matmul uses: 1 to 32 tried)
}


def k_gpu(output):
    k, p = 4.0 * K_EMU[output], 1
    while p < k:
        p *= 2
    return min(p, K_CAP)


def k_of(got, ref, A, keep=None):
    """the smallest K with which every kept element of `got` meets (*); a non-finite element, or an error where A = 0, gives inf"""
    got, ref, A = got.double().reshape(-1), ref.double().reshape(-1), A.double().reshape(-1)
    e = (got - ref).abs()
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    e = (e - FLOOR).clamp(min=0)
    k = torch.where(e > 0, e / (EPS * A), torch.zeros_like(e))
    if keep is not None:
        k = torch.where(keep.reshape(-1), k, torch.zeros_like(k))
    return float(k.max()) if k.numel() else 0.0


def nearest64(r, e):
    """fp64 squared distances [M, C] of rows r to codes e (direct form) -> (d2, nearest index, tie flag per row)"""
    d2 = ((r[:, None, :].double() - e[None].double()) ** 2).sum(-1)
    two = d2.topk(2, dim=-1, largest=False).values
    tie = (two[:, 1] - two[:, 0]) / d2.mean(-1) < TIE_MARGIN
    return d2, d2.argmin(-1), tie


def reference(x, codebooks, indices):
    """x [M, 128] fp32, codebooks [Q, C, 128] fp32, indices [M, Q] int64 (all inside [0, C)) -> dict of float64 tensors (module docstring):
    row_loss, A_row [M, Q]; loss, A_loss; G, A_G [M, 128]; quantized [M, 128] fp32; nearest [M, Q]; tie [M, Q] bool"""
    M, Q = indices.shape
    r32 = x.float().clone()
    quant = torch.zeros_like(r32)
    G, A_G = torch.zeros(M, D, dtype=torch.float64), torch.zeros(M, D, dtype=torch.float64)
    row_loss, A_row = torch.zeros(M, Q, dtype=torch.float64), torch.zeros(M, Q, dtype=torch.float64)
    nearest, tie = torch.zeros(M, Q, dtype=torch.int64), torch.zeros(M, Q, dtype=torch.bool)
    for q in range(Q):
        e32 = codebooks[q].float()
        r, e = r32.double(), e32.double()
        diff = r[:, None, :] - e[None]                                        # [M, C, 128]
        d2, nearest[:, q], tie[:, q] = nearest64(r32, e32)
        dist = d2.sqrt()
        lse = torch.logsumexp(-dist, dim=-1)
        t = indices[:, q]
        dist_t = dist.gather(1, t[:, None])[:, 0]
        row_loss[:, q] = lse + dist_t
        p = (-dist - lse[:, None]).exp()
        y = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
        w = torch.where(dist > 0, (p - y) / dist, torch.zeros_like(p))
        G -= (w[:, :, None] * diff).sum(1) / M
        A_G += (w.abs()[:, :, None] * (r.abs()[:, None, :] + e.abs()[None])).sum(1) / M
        T = (r * r).sum(-1)[:, None] + 2 * (r.abs() @ e.abs().t()) + (e * e).sum(-1)[None]
        prop = torch.where(dist > 0, T / (2 * dist), torch.full_like(T, float("inf")))
        A_row[:, q] = lse.abs() + dist_t + (p * prop).sum(-1) + prop.gather(1, t[:, None])[:, 0]
        sel = e32[nearest[:, q]]
        r32 = r32 - sel
        quant = quant + sel
    return dict(row_loss=row_loss, A_row=A_row, loss=row_loss.mean(0).sum(), A_loss=A_row.sum() / M, G=G, A_G=A_G, quantized=quant,
                nearest=nearest, tie=tie)


def compared(ref):
    """-> (pairs [M, Q]: (row, stage) pairs whose row loss is compared; rows_G [M]; rows_quant [M])"""
    seen = ref["tie"].long().cumsum(1) > 0                                    # a tie at some stage <= q
    pairs = ~seen
    Q = seen.shape[1]
    rows_G = pairs[:, Q - 2] if Q > 1 else torch.ones(seen.shape[0], dtype=torch.bool)
    return pairs, rows_G, pairs[:, Q - 1]


def mixed_loss(ref, got_row_loss):
    """the reference's scalar loss with the left-out pairs taken from the tested row losses"""
    pairs, _, _ = compared(ref)
    return torch.where(pairs, ref["row_loss"], got_row_loss.double()).mean(0).sum()


_CACHE = {}


def case(name):
    """-> (x [b, n, 128] fp32, codebooks [Q, C, 128] fp32, indices [b, n, Q] int64, reference dict): computed once, shared, never modified"""
    if name not in _CACHE:
        b, n, Q, C, noise, targets = CASES[name]
        M = b * n
        cb = make_input(f"rvq_ce:{name}:codebooks", (Q, C, D), seed=SEED) * (0.5 ** torch.arange(Q, dtype=torch.float32))[:, None, None]
        lat = make_input(f"rvq_ce:{name}:latents", (M, D), seed=SEED)
        x = lat + noise * make_input(f"rvq_ce:{name}:noise", (M, D), seed=SEED)
        if targets == "nearest":                                              # the fp64 nearest codes of the clean latents
            idx, r = torch.zeros(M, Q, dtype=torch.int64), lat.clone()
            for q in range(Q):
                _, idx[:, q], _ = nearest64(r, cb[q])
                r = r - cb[q][idx[:, q]]
        else:
            idx = (make_input(f"rvq_ce:{name}:targets", (M, Q), seed=SEED, uniform=True) * C).long().clamp(max=C - 1)
        ref = reference(x, cb, idx)
        _CACHE[name] = (x.reshape(b, n, D), cb, idx.reshape(b, n, Q), ref)
    return _CACHE[name]
