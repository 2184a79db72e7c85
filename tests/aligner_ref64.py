"""TEST INFRASTRUCTURE: float64 references of the Aligner's training kernels (csrc/aligner.hip: ns2_align_attn_bwd, ns2_align_losses_fwd /
_bwd), the inputs, shapes and bounds that tests/test_aligner_training_cpu.py (here, no GPU) and tests/test_aligner_training_gpu.py (on the
MI355X) share, and the CPU emulation of the new backend methods (`AlignerEmuBackend`).  Written from include/ns2hip.h; the pattern is
tests/backward_ref64.py's: a reference returns (ref, A) with A = the sum of the absolute values of the terms its formula adds, and

    |got - ref| <= K * 2^-24 * A + 2^-120                                                                         (*)

K_EMU[output] is what a plain fp32 torch evaluation of the same formula makes of K on these very inputs (measured and asserted by
test_aligner_training_cpu.py); the kernels get 4 * K_EMU rounded up to a power of two and never above 64 (`k_gpu`).

Distance backward: dq_t = sum_i w (q_t - k_i), dk_i = sum_t w (k_i - q_t) -- A = sum |w (q - k)| per output element, w in fp64 from the
SAME saved aln_log / aln_soft the kernel reads (they are inputs of the backward).

CTC has no term list (the recursion cancels in log space), so its measure is relative: the error of the loss over |loss|, the error of the
gradient over the largest |gradient| of the utterance, both in units of 2^-24.  The reference is F.ctc_loss in float64 on the CPU under
autograd, fed the fp64 log-softmax of the padded and masked rows; the pin is the same quantity for torch's own fp32 CPU ctc_loss on the
same inputs.  Where the reference is exactly 0 (an infeasible utterance under zero_infinity) the result must be exactly 0.

Bin loss: sum hard lp / B with lp = x - lse: A = sum hard (|x| + |lse|) / B.  Its gradient (hard - sm hs) / B with sm = exp(x - lse): the
rounding of x - lse reaches sm through exp, first order: A = (hard + sm hs (1 + |x| + |lse|)) / B.
"""
import torch
import torch.nn.functional as F

from tests.backward_ref64 import EPS, K_CAP, k_of  # noqa: F401  (k_of: re-exported for the tests)
from tests.emu_backend import EmuBackend, rup
from tests.golden.gen import make_input

FLT_MAX = torch.finfo(torch.float32).max

# worst K of the fp32 torch restatement over the cases below, as test_aligner_training_cpu.py prints it (in brackets), pinned above it
# with some room for another CPU's vector math library; -> the kernels' K (k_gpu)
K_EMU = {
    "attn_dq": 5.5,              # [4.61]    -> 32
    "attn_dk": 2.0,              # [1.73]    -> 8
    "ctc_loss": 1.5,             # [0.98]    -> 8
    "ctc_grad": 13000.0,         # [11725]   -> 64  (torch's fp32 ctc_loss: alpha ~ -1000 in fp32, and softmax - occupancy cancels; the cap binds)
    "bin_loss": 0.75,            # [0.42]    -> 4
    "bin_grad": 1.5,             # [1.12]    -> 8
}


def k_gpu(output):
    k, p = 4.0 * K_EMU[output], 1
    while p < k:
        p *= 2
    return min(p, K_CAP)


# ---------------------------------------------------------------------------------------------- distance backward
ATTN_CASES = {      # name -> (B, T, n, C, text_lens, seed)
    "base": (3, 150, 37, 80, [37, 20, 0], 11),          # the forward test's shape: full, ragged, fully masked
    "zero": (2, 70, 65, 48, [65, 40], 12),              # C = 48 (three 16-column groups), n = 65 (two key tiles); one distance exactly 0
    "long": (2, 2100, 8, 32, [8, 5], 13),               # 9 slices of 256 frames in the dk reduction
}
G_MODES = ("log", "soft", "both")


def attn_modes(name):
    """the gradients a case runs with: each output's alone and both; the long-sum case is there for the sliced dk reduction (both)"""
    return ("both",) if name == "long" else G_MODES


def attn_grads(c, mode):
    return (c["g_log"] if mode != "soft" else None), (c["g_soft"] if mode != "log" else None)


def attn_inputs(name):
    B, T, n, C, tl, seed = ATTN_CASES[name]
    q, k = make_input("al_q", (B * T, C), seed=seed), make_input("al_k", (B * n, C), seed=seed)
    if name == "zero":
        k[3] = q[5]                                      # utterance 0: frame 5 sits exactly on phoneme 3
    g_log = make_input("al_glog", (B, 1, T, n), seed=seed)
    g_soft = make_input("al_gsoft", (B, n, T), seed=seed)
    return dict(B=B, T=T, n=n, C=C, q=q, k=k, text_lens=torch.tensor(tl, dtype=torch.int32), g_log=g_log, g_soft=g_soft)


def attn_forward_torch(q, k, text_lens, B):
    """(aln_log [B, 1, T, n], aln_soft [B, n, T]) in the dtype of q: cdist, -FLT_MAX at masked phonemes, softmax over phonemes"""
    C = q.shape[1]
    qq, kk = q.reshape(B, -1, C), k.reshape(B, -1, C)
    n = kk.shape[1]
    d = (qq[:, :, None] - kk[:, None]).pow(2).sum(-1).sqrt()
    live = torch.arange(n)[None] < text_lens[:, None]
    log = d.masked_fill(~live[:, None], -FLT_MAX)
    return log[:, None], log.softmax(-1).transpose(1, 2)


def attn_weights(log, soft, g_log, g_soft, text_lens):
    """w [B, T, n] of ns2_align_attn_bwd in the dtype of `log`"""
    B, _, T, n = log.shape
    live = (torch.arange(n)[None] < text_lens[:, None])[:, None].expand(B, T, n)
    d = log[:, 0]
    G = torch.zeros_like(d) if g_log is None else g_log[:, 0].clone()
    if g_soft is not None:
        s, gs = soft.transpose(1, 2), g_soft.transpose(1, 2)
        dot = (torch.where(live, s * gs, torch.zeros_like(s))).sum(-1, keepdim=True)
        G = G + s * (gs - dot)
    ok = live & (d > 0)
    return torch.where(ok, G / torch.where(ok, d, torch.ones_like(d)), torch.zeros_like(d))


def attn_bwd(q, k, log, soft, g_log, g_soft, text_lens, dtype=torch.float64):
    """-> (dq, A_dq, dk, A_dk): the direct form, evaluated in `dtype`"""
    c = lambda t: None if t is None else t.to(dtype)     # noqa: E731
    B, _, T, n = log.shape
    w = attn_weights(c(log), c(soft), c(g_log), c(g_soft), text_lens)
    qq, kk = c(q).reshape(B, T, -1), c(k).reshape(B, n, -1)
    dq, aq, dk, ak = (torch.zeros_like(t) for t in (qq, qq, kk, kk))
    for b in range(B):                                   # per utterance: the [T, n, C] block of terms stays small
        term = w[b, :, :, None] * (qq[b, :, None] - kk[b, None])
        dq[b], aq[b] = term.sum(1), term.abs().sum(1)
        dk[b], ak[b] = -term.sum(0), term.abs().sum(0)
    r = lambda t: t.reshape(-1, t.shape[-1])             # noqa: E731
    return r(dq), r(aq), r(dk), r(ak)


# ---------------------------------------------------------------------------------------------- the two losses
LOSS_CASES = {      # name -> (B, T, n, text_lens, mel_lens, seed)
    # S = 141, 63, 65, 67, 3, 1: both sides of a wave boundary, several states per lane, one label, the empty target; utterance 2 is
    # infeasible (20 frames for 32 labels), utterance 4 has one frame
    "small": (6, 96, 70, [70, 31, 32, 33, 1, 0], [96, 70, 20, 96, 1, 5], 21),
    "wide": (2, 310, 300, [300, 170], [310, 240], 22),   # S = 601: three states per lane
}
BLANK = -1.0


def loss_inputs(name):
    """aln_log as the aligner writes it: distances of unit-scale rows (positive), -FLT_MAX at the masked phonemes; the hard path is
    maximum_path_composite's on the softmax"""
    from naturalspeech2_pytorch_amd.autograd_path import maximum_path_composite
    B, T, n, tl, ml, seed = LOSS_CASES[name]
    tl, ml = torch.tensor(tl, dtype=torch.int32), torch.tensor(ml, dtype=torch.int32)
    d = (make_input("al_dist", (B, 1, T, n), seed=seed) * 1.5 + 9.0).abs()
    live = torch.arange(n)[None] < tl[:, None]
    log = d.masked_fill(~live[:, None, None], -FLT_MAX)
    mask = (live[:, :, None] & (torch.arange(T)[None] < ml[:, None])[:, None, :]).float()
    hard = maximum_path_composite(log[:, 0].softmax(-1).transpose(1, 2), mask)
    return dict(B=B, T=T, n=n, log=log, text_lens=tl, mel_lens=ml, hard=hard.contiguous())


def ctc_torch(log, text_lens, mel_lens, blank=BLANK, dtype=torch.float64):
    """(loss, d loss / d aln_log, per-utterance largest |gradient|) by torch's CPU ctc_loss under autograd in `dtype`"""
    x = log.detach().to(dtype).requires_grad_(True)
    B, _, T, n = x.shape
    lp = F.pad(x[:, 0].permute(1, 0, 2), (1, 0), value=blank)
    cols = torch.arange(n + 1)
    lp = lp.masked_fill(cols[None, None] > text_lens.long()[None, :, None], -torch.finfo(dtype).max).log_softmax(-1)
    targets = torch.arange(1, n + 1)[None].expand(B, n)
    loss = F.ctc_loss(lp, targets, mel_lens.long(), text_lens.long(), blank=0, zero_infinity=True)
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g, g.abs().amax(dim=(1, 2, 3))


def ctc_k(got_loss, got_grad, ref_loss, ref_grad, ref_gmax):
    """(K of the loss, K of the gradient): relative errors in units of 2^-24; inf where an exact zero of the reference is not met"""
    gl, gg = got_loss.double().cpu(), got_grad.double().cpu()
    kl = float((gl - ref_loss).abs() / ref_loss.abs() / EPS) if float(ref_loss) != 0 else (0.0 if float(gl) == 0 else float("inf"))
    kg = 0.0
    for b in range(ref_grad.shape[0]):
        e = float((gg[b] - ref_grad[b]).abs().max())
        zero_ok = bool((gg[b][ref_grad[b] == 0] == 0).all())
        if not zero_ok or not bool(torch.isfinite(gg[b]).all()):
            return kl, float("inf")
        if float(ref_gmax[b]) > 0:
            kg = max(kg, e / float(ref_gmax[b]) / EPS)
    return kl, kg


def bin_ref(log, hard, text_lens, dtype=torch.float64):
    """-> (loss, A_loss, grad [B, 1, T, n], A_grad) of BinLoss, evaluated in `dtype`"""
    x, h = log.to(dtype)[:, 0], hard.to(dtype).transpose(1, 2)                    # [B, T, n]
    B, T, n = x.shape
    keep = (torch.arange(n)[None] <= text_lens.long()[:, None])[:, None].expand(B, T, n)
    xm = x.masked_fill(~keep, -torch.finfo(dtype).max)
    lse = torch.logsumexp(xm, dim=-1, keepdim=True)
    lp = xm - lse
    hk = torch.where(keep, h, torch.zeros_like(h))
    loss = (hk * lp).sum() / B
    a_loss = (hk * (xm.abs() + lse.abs())).sum() / B
    sm, hs = torch.exp(lp), hk.sum(-1, keepdim=True)
    grad = torch.where(keep, (hk - sm * hs) / B, torch.zeros_like(x))
    a_grad = torch.where(keep, (hk + sm * hs * (1 + torch.where(keep, x.abs(), torch.zeros_like(x)) + lse.abs())) / B, torch.zeros_like(x))
    return loss, a_loss, grad[:, None], a_grad[:, None]


# ---------------------------------------------------------------------------------------------- the CPU emulation of the new backend methods
class AlignerEmuBackend(EmuBackend):
    """EmuBackend + the methods `training.aligner_forward_train` adds to the backend, restated with plain fp32 torch ops from the header's
    contracts (padded leading dimensions, NaN in the columns a kernel does not write)"""
    name = "emu-aligner"

    def _padded(self, y, C):
        out = torch.full((y.shape[0], rup(C, 32)), float("nan"))
        out[:, :C] = y[:, :C]
        return out

    def relu_fwd(self, pre, C):
        self.calls.append("relu_fwd")
        return self._padded(pre[:, :C].clamp(min=0), C)

    def relu_bwd(self, dy, pre, C):
        self.calls.append("relu_bwd")
        assert not torch.isnan(dy[:, :C]).any()
        return self._padded(torch.where(pre[:, :C] > 0, dy[:, :C], torch.zeros_like(dy[:, :C])), C)

    def align_attn(self, q, k, text_lens, B):
        self.calls.append("align_attn")
        log, soft = attn_forward_torch(q, k, text_lens, B)
        return log.contiguous(), soft.contiguous()

    def align_attn_bwd(self, q, k, log, soft, g_log, g_soft, text_lens):
        self.calls.append("align_attn_bwd")
        dq, _, dk, _ = attn_bwd(q, k, log, soft, g_log, g_soft, text_lens, dtype=torch.float32)
        return dq, dk
