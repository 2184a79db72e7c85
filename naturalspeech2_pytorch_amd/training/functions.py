"""The autograd Functions of the training path (how the graph is cut: the package docstring) and the helpers they share.  Everything a
Function launches is a call of the backend it took from `passes.backend()` at the top of its forward."""
import torch

from ..ops import round_up
from .passes import _un, backend, current


# =============================================================================================== weight sources of the two packs
def _taps(w):
    return w.shape[2] if w.ndim == 3 else 0


def _fwd_pack(bk, w):
    return bk.pack(("f", id(w)), (w,), lambda: w, parts=[(0, "n", 0, 0)])


def _bwd_pack(bk, w):
    """the dgrad weight: dX = dY W  ->  rows = input channels, columns = output channels, taps flipped (the gradient of a causal
    conv reads dY[n + (k - 1 - t) dil], i.e. a conv with pad_left = 0 whose tap t' is the forward's tap k - 1 - t')"""
    if w.ndim == 3:
        return bk.pack(("b", id(w)), (w,), lambda: w.detach().permute(1, 0, 2).flip(-1), parts=[(0, "tf", 0, 0)])
    return bk.pack(("b", id(w)), (w,), lambda: w.detach().t(), parts=[(0, "t", 0, 0)])


def _shifts(taps, dil):
    return tuple((taps - 1 - t) * dil for t in range(taps)) if taps else (0,)


def _rl(lens, seq_len):
    """the `row_lens=` keyword of the backend's products over the b * n frame rows of a pass that skips (`ragged_skip_training`;
    include/ns2hip_train.h): lens = int32 [b] on the device, or None -- then no keyword at all: the same calls as ever"""
    return {} if lens is None else {"row_lens": (lens, seq_len)}


def _grads(bk, dy, C, xp, K, taps=0, dil=1, seq_len=0, need_row=True, need_w=True, need_b=False, pad_left=-1, rl={}):
    """what the backward of y = conv_or_linear(x) (+ b) needs from dy fp32 [M, >= C]: its row planes (the dgrad GEMM's operand), the
    weight gradient dW against xp = the operand planes the forward GEMM read, the bias gradient.  The weight gradient comes
    from the row planes themselves where the kernel can (ns2_wgrad_rows: LDS transpose reads), else through transposed copies
    (narrow gradients: the dim = 128 model).  `pad_left` >= 0 and != taps - 1: a NON-causal conv (SpeechPromptEncoder's Conv1d(k = 9, padding = 4),
    NS2:306-311): tap t read x[n - (pad_left - t) dil], rows shifted in BOTH directions -- the transposed copies take any signed shift
    (tplanes_kernel zero-fills outside the utterance), the row-plane kernel's tap offsets are the causal ones, so this case always goes
    through the copies.  `rl`: `_rl(...)` of a skipping pass, handed to the row-plane weight gradient (the transposed route takes no lengths:
    it adds the exact zeros of dy's hidden rows).  -> (dy_row or None, dW or None, db or None); dW in the parameter's own shape: [C, K, taps],
    a Linear's (taps = 0) [C, K]"""
    T = max(taps, 1)
    causal = pad_left < 0 or pad_left == taps - 1
    dw = None
    if causal and need_w and bk.wgrad_rows_ok(C, T, K, seq_len, dy.shape[0]):
        row, _, db = bk.grad_prep(dy, C, want_row=True, want_colsum=need_b)
        dw = bk.wgrad_rows(row, xp, C, T, K, dil, seq_len, **rl)
    else:
        row, dy_t, db = bk.grad_prep(dy, C, want_row=need_row, want_t=need_w, want_colsum=need_b)
        if need_w:
            shifts = _shifts(taps, dil) if causal else tuple((pad_left - t) * dil for t in range(taps))
            xt = bk.transpose(xp, 0, round_up(K, 32), seq_len if taps else 0, shifts)
            dw = bk.wgrad(dy_t, xt, C, T, K)
    return row, (dw if taps or dw is None else dw[:, :, 0]), db


# =============================================================================================== what the Functions share
def _begin(ctx):
    """top of every forward: the Function keeps the backend and the loss scale of the pass being built for its backward"""
    ctx.bk, ctx.sc = backend(), current().scale
    return ctx.bk


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _rowmajor(dy):
    """an incoming gradient [M, C] with unit column stride (the kernels take a row stride only)"""
    return dy if dy.stride(1) == 1 else dy.contiguous()


def _norm_in_front(bk, h, seq_len, film, gamma):
    """the operand planes a block's first GEMM reads: RMSNorm(h) under the adaptive (gamma, beta) of `film`, under the learned `gamma`,
    or h itself"""
    assert film is None or gamma is None
    if film is not None:
        return bk.rmsnorm(h, seq_len, cond=film)
    return bk.rmsnorm(h, seq_len, gamma=gamma) if gamma is not None else bk.split(h)


def _norm_in_front_bwd(bk, h, dxn, dy, B, seq_len, film, gamma):
    """backward of `_norm_in_front` and of the residual around the block: dxn = the gradient of the norm's output, dy = the block's
    incoming gradient -> (dh = dy + dL/dh through the norm, dfilm or None, dgamma or None)"""
    d = h.shape[1]
    if film is not None:
        dh, dfilm, _ = bk.rmsnorm_bwd(h, dxn, B, seq_len, d, cond=film, dx_add=dy)
        return dh, dfilm, None
    if gamma is not None:
        dh, _, dgamma = bk.rmsnorm_bwd(h, dxn, B, seq_len, d, gamma=gamma, dx_add=dy)
        return dh, None, dgamma
    return dy[:, :d] + dxn[:, :d], None, None


# =============================================================================================== Functions
class GemmFn(torch.autograd.Function):
    """y = conv_or_linear(x) + b (+ resid);  x [M, Cin] fp32, w [Cout, Cin(, k)], causal with dilation `dil` inside utterances of
    `seq_len` tokens (NS2:583-595).  `pad_left` >= 0: a conv with that many zero rows in front instead of the causal k - 1 (nn.Conv1d(k,
    padding = pad_left), NS2:306-311): its dgrad is the forward kernel on the tap-flipped weight with pad_left' = k - 1 - pad_left"""

    @staticmethod
    def forward(ctx, x, w, b, resid, seq_len, dil, pad_left=-1, lens=None):
        """lens: int32 [b] on the device when the rows are the b * seq_len frame rows of a pass that skips (`_rl`), else None"""
        bk = _begin(ctx)
        taps = _taps(w)
        if pad_left == taps - 1 or not taps:
            pad_left = -1
        assert lens is None or pad_left < 0, "a skipping product is causal or plain in the forward"
        xp = bk.split(x)
        kw = {} if pad_left < 0 else {"pad_left": pad_left}
        ctx.rl = _rl(lens, seq_len)
        y = bk.gemm_f32(_fwd_pack(bk, w), xp, bias=b, resid=resid, taps=taps, dil=dil, seq_len=seq_len if taps else 0, **kw, **ctx.rl)
        ctx.save_for_backward(w, b)
        ctx.xp, ctx.cfg, ctx.pad_left = xp, (taps, dil, seq_len, x.shape[1], resid is not None), pad_left
        return y[:, :w.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        bk = ctx.bk
        w, b = ctx.saved_tensors
        taps, dil, seq_len, cin, has_resid = ctx.cfg
        cout = w.shape[0]
        dy = _rowmajor(dy)
        # (frozen weights / a gradient wanted for the input only -- guidance: no wgrad GEMM, no transposes, no workspace: ADVICE r4)
        need_w, need_b = ctx.needs_input_grad[1], b is not None and ctx.needs_input_grad[2]
        pl = ctx.pad_left
        dy_row, dw, db = _grads(bk, dy, cout, ctx.xp, cin, taps, dil, seq_len, need_row=ctx.needs_input_grad[0], need_w=need_w, need_b=need_b,
                                pad_left=pl, rl=ctx.rl)
        dx = None
        if ctx.needs_input_grad[0]:
            pl_b = (0 if pl < 0 else taps - 1 - pl) if taps else -1
            dx = bk.gemm_f32(_bwd_pack(bk, w), dy_row, taps=taps, dil=dil, seq_len=seq_len if taps else 0, pad_left=pl_b, **ctx.rl)[:, :cin]
        return dx, *_un(ctx, dw, db), (dy if has_resid else None), None, None, None, None


class WavenetBlockFn(torch.autograd.Function):
    """WavenetResBlock (NS2:597-642) without its skip conv: out = tanh(z) sigmoid(z) + res_conv(u), z = conv_dil(u) gamma + beta"""

    @staticmethod
    def forward(ctx, u, film, wc, bc, wr, br, seq_len, dil, lens=None):
        bk = _begin(ctx)
        d = u.shape[1]
        up = bk.split(u)
        rl = ctx.rl = _rl(lens, seq_len)
        hc = bk.gemm_f32(_fwd_pack(bk, wc), up, bias=bc, taps=3, dil=dil, seq_len=seq_len, **rl)
        g = bk.film_gate_fwd(hc, film, seq_len, d)
        out = bk.gemm_f32(_fwd_pack(bk, wr), up, bias=br, resid=g, taps=1, dil=1, seq_len=seq_len, **rl)
        ctx.save_for_backward(film, wc, wr, hc)
        ctx.up, ctx.cfg = up, (seq_len, dil, d)
        return out[:, :d]

    @staticmethod
    def backward(ctx, dout):
        bk = ctx.bk
        film, wc, wr, hc = ctx.saved_tensors
        seq_len, dil, d = ctx.cfg
        B = dout.shape[0] // seq_len
        dout = _rowmajor(dout)
        ng = ctx.needs_input_grad                                           # (u, film, wc, bc, wr, br, -, -, -)
        rl = ctx.rl
        if bk.wgrad_rows_ok(d, 3, d, seq_len, dout.shape[0]) and bk.wgrad_rows_ok(d, 1, d, seq_len, dout.shape[0]):
            dout_row, dwr, dbr = _grads(bk, dout, d, ctx.up, d, 1, 1, seq_len, need_w=ng[4], need_b=ng[5], rl=rl)
            dhc, dfilm = bk.film_gate_bwd(dout, hc, film, B, seq_len, d)
            dhc_row, dwc, dbc = _grads(bk, dhc, d, ctx.up, d, 3, dil, seq_len, need_w=ng[2], need_b=ng[3], rl=rl)
        else:                                                               # narrow model: transposed copies, one set for both gradients
            dout_row, dout_t, dbr = bk.grad_prep(dout, d, want_row=True, want_t=ng[4], want_colsum=ng[5])
            dhc, dfilm = bk.film_gate_bwd(dout, hc, film, B, seq_len, d)
            dhc_row, dhc_t, dbc = bk.grad_prep(dhc, d, want_row=True, want_t=ng[2], want_colsum=ng[3])
            dwc = dwr = None
            if ng[2] or ng[4]:
                xt = bk.transpose(ctx.up, 0, d, seq_len, _shifts(3, dil))       # taps 0, 1, 2: shifts 2 dil, dil, 0
                if ng[2]:
                    dwc = bk.wgrad(dhc_t, xt, d, 3, d)
                if ng[4]:
                    dwr = bk.wgrad(dout_t, xt, d, 1, d, row_off=2 * round_up(d, 32))    # res_conv reads the unshifted block (tap 2)
        du = bk.gemm_f32(_bwd_pack(bk, wc), dhc_row, taps=3, dil=dil, seq_len=seq_len, pad_left=0, **rl)
        du = bk.gemm_f32(_bwd_pack(bk, wr), dout_row, resid=du, taps=1, dil=1, seq_len=seq_len, pad_left=0, **rl)
        return du[:, :d], *_un(ctx, dfilm, dwc, dbc, dwr, dbr), None, None, None


class AttnFn(torch.autograd.Function):
    """h + to_out(attention(q, k, v)) with q = to_q(norm(h)), k, v = to_kv(context or norm(h)); norm = RMSNorm with the adaptive
    (gamma, beta) of `film` (Model, NS2:727-746) -- heads of 64, non-causal, no mask (ATT:77-155).  `film = None`: no norm in front
    (the PerceiverResampler's attention, NS2:574: its context = cat(latents, prompt) is formed by the caller, so the part of the
    context gradient that belongs to the latents reaches them through torch's cat).
    The plain `Transformer` of the conditioning encoders (NS2:1073-1115) adds three things, all absent by default (same kernels, same
    bits as before): `gamma` -- the learned-gamma RMSNorm in front (with `film = None`); `kmask` -- key-padding mask, uint8 [B, Nk],
    1 = attend (ATT:92-94); `drop` = (p, seed tensor, call index) -- dropout on the softmax output (ATT:100-101; csrc/dropout_keep.h).
    The DurationPitchPredictor's attention (NS2:464, 1060-1061) reads an `h` that IS the norm's output (it is also part of the context, so
    the caller forms it) and adds the PRE-norm rows: `resid` [M, d] replaces `h` as the residual (with `film = gamma = None`); `h` then gets
    the q path's gradient only and `resid` the incoming one.  Absent by default, like the others.
    `lens` -- int32 [B] on the device, the utterances' lengths of a ragged batch (self-attention only, without kmask / drop;
    include/ns2hip_train.h): keys stop at the length, and the rows of o and of dq | dk | dv from the length on are exact zeros.
    The kernels alone read it.  Absent by default: same kernels, same bits.
    `masked_rows_zero` -- a promise of the ragged conditioning passes (include/ns2hip_train.h), with `kmask` and without `drop`:
    the rows of h / the context that the mask hides are ZEROS (so their k and v are zeros: no bias in to_q / to_kv, RMSNorm(0) = 0), the
    cotangent of every query row they stand for is 0, and the caller selects the returned gradient rows of the hidden rows to 0.  The
    backward then runs the PLAIN attention backward -- the instantiation the pass without lengths runs at dropout 0, i.e. what each
    utterance alone gets: a hidden key has P = exp2(-lse) there instead of 0, but k = v = 0 keeps it out of dq, a zero dO row keeps the
    hidden queries out of dk | dv, the hidden rows' own dk | dv meet zero operand rows in the weight gradient, and what they leave in the
    input gradient is selected away.  (The key-mask backward instantiation gives other last bits than the plain one on the same operands;
    with dropout both the ragged batch and the utterance alone run it.)  Absent by default.
    `head_dim` -- 32 or 128 instead of the heads of 64 (include/ns2hip_train.h; `head_dim_training`).  The backend is handed it
    only when it is not 64, as it is handed `lens` only when there are lengths: same calls, same kernels, same bits by default.
    `row_lens` -- int32 [B] on the device, a pass that skips (`ragged_skip_training`; include/ns2hip_train.h): the products
    over the B seq_len frame rows -- q | k | v or the cross attention's q, to_out, their dgrads and row-plane weight gradients -- are
    handed the lengths (`_rl`); the cross attention's k | v projection, whose rows are the context's, never is.  The attention kernels
    keep `lens`.  Absent by default, like the others."""

    @staticmethod
    def forward(ctx, h, film, ctxt, wq, wkv, wout, seq_len, heads, ctx_len, gamma=None, kmask=None, drop=None, resid=None, lens=None,
                head_dim=64, masked_rows_zero=False, row_lens=None):
        assert resid is None or (film is None and gamma is None)
        assert lens is None or (ctxt is None and kmask is None and drop is None), "lens: the plain self-attention only"
        bk = _begin(ctx)
        M, d = h.shape
        B, a = M // seq_len, heads * head_dim
        hd = {} if head_dim == 64 else {"head_dim": head_dim}
        rl = ctx.rl = _rl(row_lens, seq_len)
        xn = _norm_in_front(bk, h, seq_len, film, gamma)
        if ctxt is None:                                                    # self attention: one GEMM for q | k | v
            wqkv = bk.pack(("qkv", id(wq), id(wkv)), (wq, wkv), lambda: torch.cat((wq.detach(), wkv.detach()), 0),
                           parts=[(0, "n", 0, 0), (1, "n", a, 0)])
            qkv = bk.gemm_split(wqkv, xn, attn=True, **rl)
            q, k, v, qc, kc, vc, Nk, cp = qkv, qkv, qkv, 0, a, 2 * a, seq_len, None
        else:
            q = bk.gemm_split(_fwd_pack(bk, wq), xn, attn=True, **rl)
            cp = bk.split(ctxt)
            kv = bk.gemm_split(_fwd_pack(bk, wkv), cp, attn=True)
            k, v, qc, kc, vc, Nk = kv, kv, 0, 0, a, ctx_len
        vt = bk.transpose(v, vc, a, Nk, per_batch=True)
        if lens is not None:
            o, lse = bk.attention(q, qc, k, kc, vt, B, heads, seq_len, Nk, lens=lens, **hd)
        elif kmask is None and drop is None:
            o, lse = bk.attention(q, qc, k, kc, vt, B, heads, seq_len, Nk, **hd)
        else:
            o, lse = bk.attention_masked(q, qc, k, kc, vt, B, heads, seq_len, Nk, kmask=kmask, drop=drop, **hd)
        y = bk.gemm_f32(_fwd_pack(bk, wout), o, resid=h if resid is None else resid, **rl)
        ctx.save_for_backward(h, film, wq, wkv, wout, lse, gamma)
        ctx.pl, ctx.cfg, ctx.md, ctx.lens = (xn, q, k, v, o, cp), (seq_len, heads, Nk, qc, kc, vc, ctxt is not None), (kmask, drop), lens
        ctx.own_resid, ctx.hd = resid is None, hd
        ctx.plain_bwd = bool(masked_rows_zero) and kmask is not None and drop is None
        return y[:, :d]

    @staticmethod
    def backward(ctx, dy):
        bk = ctx.bk
        h, film, wq, wkv, wout, lse, gamma = ctx.saved_tensors
        xn, q, k, v, o, cp = ctx.pl
        seq_len, heads, Nk, qc, kc, vc, cross = ctx.cfg
        kmask, drop = ctx.md
        M, d = h.shape
        hd = ctx.hd
        B, a = M // seq_len, heads * hd.get("head_dim", 64)
        dy = _rowmajor(dy)
        ng = ctx.needs_input_grad                                           # (h, film, ctxt, wq, wkv, wout, ...)
        rl = ctx.rl
        if ctx.lens is not None:
            def attention_bwd(*args, **kw):
                bk.attention_bwd(*args, lens=ctx.lens, **hd, **kw)
        elif (kmask is None and drop is None) or ctx.plain_bwd:
            def attention_bwd(*args, **kw):
                bk.attention_bwd(*args, **hd, **kw)
        else:
            def attention_bwd(*args, **kw):
                bk.attention_bwd_masked(*args, kmask=kmask, drop=drop, **hd, **kw)
        dy_row, dwout, _ = _grads(bk, dy, d, o, a, need_w=ng[5], rl=rl)
        do = bk.gemm_f32(_bwd_pack(bk, wout), dy_row, **rl)                 # [M, a]
        delta = bk.attention_delta(do, o, B, heads, seq_len, **hd)
        # (the backward kernels form K^T, Q^T and dO^T inside the CU: LDS transpose reads of the row-major tiles)
        do_row, _, _ = bk.grad_prep(do, a, want_row=True, attn=True)
        if not cross:
            need_w = ng[3] or ng[4]
            if not need_w or bk.wgrad_rows_ok(3 * a, 1, d, 0, M):
                # dq | dk | dv feed two GEMMs only (the projection's dgrad and wgrad): they leave the attention backward as operand planes
                g_row = bk.new_planes(M, 3 * a)
                attention_bwd(q, qc, k, kc, v, vc, do_row, lse, delta, B, heads, seq_len, Nk, planes=(g_row, 0, a, 2 * a))
                dwqkv = bk.wgrad_rows(g_row, xn, 3 * a, 1, d, **rl)[:, :, 0] if need_w else None
            else:
                dqkv = torch.empty(M, 3 * a, dtype=torch.float32, device=h.device)
                attention_bwd(q, qc, k, kc, v, vc, do_row, lse, delta, B, heads, seq_len, Nk, dq=(dqkv, 0), dkv=(dqkv, a, 2 * a))
                g_row, dwqkv, _ = _grads(bk, dqkv, 3 * a, xn, d, need_w=need_w, rl=rl)
            dwq = dwkv = None
            if need_w:
                dwq, dwkv = dwqkv[:a], dwqkv[a:]
            wqkv = bk.pack(("qkv_b", id(wq), id(wkv)), (wq, wkv), lambda: torch.cat((wq.detach(), wkv.detach()), 0).t(),
                           parts=[(0, "t", 0, 0), (1, "t", 0, a)])
            dxn = bk.gemm_f32(wqkv, g_row, **rl)
            dctx = None
        else:
            dq = torch.empty(M, a, dtype=torch.float32, device=h.device)
            dkv = torch.empty(B * Nk, 2 * a, dtype=torch.float32, device=h.device)
            attention_bwd(q, qc, k, kc, v, vc, do_row, lse, delta, B, heads, seq_len, Nk, dq=(dq, 0), dkv=(dkv, 0, a))
            q_row, dwq, _ = _grads(bk, dq, a, xn, d, need_w=ng[3], rl=rl)
            dxn = bk.gemm_f32(_bwd_pack(bk, wq), q_row, **rl)
            kv_row, dwkv, _ = _grads(bk, dkv, 2 * a, cp, d, need_row=ng[2], need_w=ng[4])
            dctx = bk.gemm_f32(_bwd_pack(bk, wkv), kv_row)[:, :d] if ng[2] else None
        if ctx.own_resid:
            dh, dfilm, dgamma = _norm_in_front_bwd(bk, h, dxn, dy, B, seq_len, film, gamma)
            dresid = None
        else:
            dh, dfilm, dgamma, dresid = dxn[:, :d], None, None, dy
        dfilm, dwq, dwkv, dwout, dgamma = _un(ctx, dfilm, dwq, dwkv, dwout, dgamma)
        return dh, dfilm, dctx, dwq, dwkv, dwout, None, None, None, dgamma, None, None, dresid, None, None, None, None


def attn_apply(*args, head_dim=64, masked_rows_zero=False, row_lens=None):
    """`AttnFn.apply(*args)`; a head dim other than 64 (`head_dim_training`) is appended behind the optional arguments, 64 leaves the
    call exactly what it was; `masked_rows_zero` (the ragged conditioning passes) likewise behind the head dim, and `row_lens` (a pass
    that skips, `ragged_skip_training`) behind that"""
    if row_lens is not None:
        return AttnFn.apply(*args, *([None] * (14 - len(args))), head_dim, masked_rows_zero, row_lens)
    if masked_rows_zero:
        return AttnFn.apply(*args, *([None] * (14 - len(args))), head_dim, True)
    if head_dim == 64:
        return AttnFn.apply(*args)
    return AttnFn.apply(*args, *([None] * (14 - len(args))), head_dim)


def train_head_dim(owner, dim_head):
    """the head dim a training pass hands to `AttnFn`: `dim_head` where `owner` has `head_dim_training` on, else the kernels' 64"""
    return dim_head if getattr(owner, "head_dim_training", False) else 64


HEAD_DIMS_TRAIN = (32, 64, 128)                 # what `head_dim_training=True` accepts (include/ns2hip_train.h)


class FeedForwardFn(torch.autograd.Function):
    """h + Linear(CausalConv1d_k3(GEGLU(Linear(norm(h)))))   (NS2:1004-1025 with the adaptive RMSNorm in front, NS2:805-807).
    `film = None`: no norm; `wc = None`: no conv -- the PerceiverResampler's FeedForward (NS2:564, 575); `gamma` (with `film = None`): the
    learned-gamma RMSNorm in front -- the plain Transformer's FeedForward (NS2:1098-1101)"""

    @staticmethod
    def forward(ctx, h, film, w1, b1, wc, bc, w2, b2, seq_len, gamma=None, lens=None):
        bk = _begin(ctx)
        M, d = h.shape
        f = w2.shape[1]
        rl = ctx.rl = _rl(lens, seq_len)
        xn = _norm_in_front(bk, h, seq_len, film, gamma)
        pre = bk.gemm_f32(_fwd_pack(bk, w1), xn, bias=b1, **rl)             # [M, 2 f]: x | gate
        hp = bk.geglu_fwd(pre, f)
        cp = bk.gemm_split(_fwd_pack(bk, wc), hp, bias=bc, taps=3, dil=1, seq_len=seq_len, **rl) if wc is not None else hp
        y = bk.gemm_f32(_fwd_pack(bk, w2), cp, bias=b2, resid=h, **rl)
        ctx.save_for_backward(h, film, w1, wc, w2, pre, gamma)
        ctx.pl, ctx.cfg = (xn, hp, cp), (seq_len, f)
        return y[:, :d]

    @staticmethod
    def backward(ctx, dy):
        bk = ctx.bk
        h, film, w1, wc, w2, pre, gamma = ctx.saved_tensors
        xn, hp, cp = ctx.pl
        seq_len, f = ctx.cfg
        M, d = h.shape
        B = M // seq_len
        dy = _rowmajor(dy)
        ng = ctx.needs_input_grad                                           # (h, film, w1, b1, wc, bc, w2, b2, -)
        rl = ctx.rl
        planes_dc = wc is not None and bk.wgrad_rows_ok(f, 3, f, seq_len, M)
        dy_row, dw2, db2 = _grads(bk, dy, d, cp, f, need_w=ng[6], need_b=ng[7] or (planes_dc and ng[5]), rl=rl)
        dwc = dbc = None
        if planes_dc:
            # dc = dy W2 feeds two GEMMs only (the conv's dgrad and wgrad): it leaves the dgrad GEMM as operand planes and never exists in
            # fp32; the conv's bias gradient, colsum(dy W2), is colsum(dy) W2 -- a [d] x [d, f] product of what the FF-out bias gradient sums anyway
            dc_row = bk.gemm_split(_bwd_pack(bk, w2), dy_row, **rl)
            dwc = bk.wgrad_rows(dc_row, hp, f, 3, f, 1, seq_len, **rl) if ng[4] else None
            dbc = db2 @ w2.detach() if ng[5] else None
            db2 = db2 if ng[7] else None
            dhh = bk.gemm_f32(_bwd_pack(bk, wc), dc_row, taps=3, dil=1, seq_len=seq_len, pad_left=0, **rl)
        else:
            dc = bk.gemm_f32(_bwd_pack(bk, w2), dy_row, **rl)               # [M, f]
            if wc is not None:
                dc_row, dwc, dbc = _grads(bk, dc, f, hp, f, 3, 1, seq_len, need_w=ng[4], need_b=ng[5], rl=rl)
                dhh = bk.gemm_f32(_bwd_pack(bk, wc), dc_row, taps=3, dil=1, seq_len=seq_len, pad_left=0, **rl)
            else:
                dhh = dc
        dpre = bk.geglu_bwd(dhh, pre, f)                                    # [M, 2 f]
        p_row, dw1, db1 = _grads(bk, dpre, 2 * f, xn, d, need_w=ng[2], need_b=ng[3], rl=rl)
        dxn = bk.gemm_f32(_bwd_pack(bk, w1), p_row, **rl)
        dh, dfilm, dgamma = _norm_in_front_bwd(bk, h, dxn, dy, B, seq_len, film, gamma)
        return dh, *_un(ctx, dfilm, dw1, db1, dwc, dbc, dw2, db2), None, *_un(ctx, dgamma), None


class NormLinearFn(torch.autograd.Function):
    """Linear(RMSNorm(h) * gamma), no bias: `to_pred` (NS2:781-784)"""

    @staticmethod
    def forward(ctx, h, gamma, w, seq_len, lens=None):
        bk = _begin(ctx)
        xn = bk.rmsnorm(h, seq_len, gamma=gamma)
        ctx.rl = _rl(lens, seq_len)
        y = bk.gemm_f32(_fwd_pack(bk, w), xn, **ctx.rl)
        ctx.save_for_backward(h, gamma, w)
        ctx.xn, ctx.seq_len = xn, seq_len
        return y[:, :w.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        bk = ctx.bk
        h, gamma, w = ctx.saved_tensors
        M, d = h.shape
        dy = _rowmajor(dy)
        dy_row, dw, _ = _grads(bk, dy, w.shape[0], ctx.xn, d, need_w=ctx.needs_input_grad[2], rl=ctx.rl)
        dxn = bk.gemm_f32(_bwd_pack(bk, w), dy_row, **ctx.rl)
        dh, _, dgamma = bk.rmsnorm_bwd(h, dxn, M // ctx.seq_len, ctx.seq_len, d, gamma=gamma)
        return dh, *_un(ctx, dgamma, dw), None, None


class RmsNormFn(torch.autograd.Function):
    """RMSNorm(h) * gamma as a tensor of the graph: the PerceiverResampler's final norm (NS2:579, 727-746 with scale = True)"""

    @staticmethod
    def forward(ctx, h, gamma):
        ctx.save_for_backward(h, gamma)
        return _begin(ctx).rmsnorm_f32(h, gamma)

    @staticmethod
    def backward(ctx, dy):
        h, gamma = ctx.saved_tensors
        M, d = h.shape
        dy = _rowmajor(dy)
        dh, _, dgamma = ctx.bk.rmsnorm_bwd(h, dy, 1, M, d, gamma=gamma)      # one "utterance" of M rows: the norm is per row
        return dh, *_un(ctx, dgamma)


class SiluFn(torch.autograd.Function):
    """SiLU on fp32 rows with the pre-activation kept (the encoders' k = 9 convolutions, NS2:247, 306-311: inference runs it in the GEMM
    epilogue and keeps nothing)"""

    @staticmethod
    def forward(ctx, pre):
        bk = _begin(ctx)
        ctx.save_for_backward(pre)
        return bk.silu_fwd(pre, pre.shape[1])[:, :pre.shape[1]]

    @staticmethod
    def backward(ctx, dy):
        pre, = ctx.saved_tensors
        dy = _rowmajor(dy)
        return ctx.bk.silu_bwd(dy, pre, pre.shape[1])[:, :pre.shape[1]]


class ReluFn(torch.autograd.Function):
    """ReLU on fp32 rows with the pre-activation kept: between the Aligner's convolutions (aligner.py:30-51; inference runs ns2_relu_split and
    keeps nothing)"""

    @staticmethod
    def forward(ctx, pre):
        bk = _begin(ctx)
        ctx.save_for_backward(pre)
        return bk.relu_fwd(pre, pre.shape[1])[:, :pre.shape[1]]

    @staticmethod
    def backward(ctx, dy):
        pre, = ctx.saved_tensors
        dy = _rowmajor(dy)
        return ctx.bk.relu_bwd(dy, pre, pre.shape[1])[:, :pre.shape[1]]


class AlignAttnFn(torch.autograd.Function):
    """AlignerNet's attention (aligner.py:72-90): queries [B T, C], keys [B n, C], int32 text lengths [B] on the device -> (aln_log [B, 1, T, n]
    = the distances, -FLT_MAX at masked phonemes; aln_soft [B, n, T] = their softmax).  Forward: the inference kernel ns2_align_attn, the same
    bits; backward: ns2_align_attn_bwd (direct-form sums in fixed orders)"""

    @staticmethod
    def forward(ctx, q, k, text_lens, B):
        bk = _begin(ctx)
        log, soft = bk.align_attn(q, k, text_lens, B)
        ctx.save_for_backward(q, k, log, soft, text_lens)
        return log, soft

    @staticmethod
    def backward(ctx, g_log, g_soft):
        q, k, log, soft, text_lens = ctx.saved_tensors
        g_log = None if g_log is None else _c(g_log.float())
        g_soft = None if g_soft is None else _c(g_soft.float())
        dq, dk = ctx.bk.align_attn_bwd(q, k, log, soft, g_log, g_soft, text_lens)
        return dq, dk, None, None


class RvqCrossEntropyFn(torch.autograd.Function):
    """the RVQ cross-entropy term of the training loss (NS2:1668-1684; codec.py `ResidualVQCrossEntropy`): x [M, 128] fp32, codebooks [Q, C, 128]
    and their half-norms [Q, C], indices [M, Q] int64 -> (loss 0-dim, quantized_out [M, 128]).  One launch (ns2_rvq_ce) computes the loss and
    the unit gradient G = d loss / d x, the only tensor kept; the backward is grad_out * G.  The codebooks are buffers and the indices
    integers: neither gets a gradient; quantized_out is a sum of (detached) codes.
    lens [B] int32 on the device (M = B n; None: today's call): the ragged batch of ns2_rvq_ce_lens -- the loss is the mean over utterances
    of each one's own mean, G's rows at or behind a length are exact zeros, and nothing reads the lengths on the host."""

    @staticmethod
    def forward(ctx, x, codebooks, cb_norm, indices, lens=None):
        bk = _begin(ctx)
        kw = {} if lens is None else dict(lens=lens)
        loss, quant, G = bk.rvq_cross_entropy(x, codebooks, cb_norm, indices, need_grad=ctx.needs_input_grad[0], **kw)
        ctx.save_for_backward(G)
        ctx.mark_non_differentiable(quant)
        return loss, quant

    @staticmethod
    def backward(ctx, g_loss, _g_quant):
        G, = ctx.saved_tensors
        return (g_loss * G if G is not None else None), None, None, None, None


class GroupNormSiluFn(torch.autograd.Function):
    """silu(GroupNorm(x)) (+ resid) over the rows of utterances of `seq_len` tokens: a Block of the DurationPitchPredictor's ResnetBlock, the
    last one with the ResnetBlock's input as `resid` (NS2:346-400).  The backward normalises with the forward's own statistics slots.
    `row_lens` -- int32 [B] on the device, the utterances' row counts of a ragged batch (include/ns2hip_train.h): statistics
    and gradient sums stop at a length, rows of y and of dx from it on are exact zeros (so `resid` gets no gradient there either), and
    nothing there is read.  The kernels alone read it.  Absent by default: the backend gets the calls without it, same kernels, same bits."""

    @staticmethod
    def forward(ctx, x, weight, bias, resid, seq_len, groups, eps, row_lens=None):
        bk = _begin(ctx)
        B = x.shape[0] // seq_len
        kw = {} if row_lens is None else dict(row_lens=row_lens)
        y, rows, stats = bk.groupnorm_silu_fwd(x, B, seq_len, weight.detach(), bias.detach(), groups, eps, resid=resid, **kw)
        ctx.save_for_backward(rows, weight, bias, stats)
        ctx.cfg = (B, seq_len, groups, eps, resid is not None)
        ctx.kw = kw
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, weight, bias, stats = ctx.saved_tensors
        B, seq_len, groups, eps, has_resid = ctx.cfg
        dy = _rowmajor(dy)
        dx, dw, db = ctx.bk.groupnorm_silu_bwd(dy, rows, stats, B, seq_len, weight.detach(), bias.detach(), groups, eps, **ctx.kw)
        dres = None
        if has_resid:
            # the residual was not added behind a length: its gradient there is 0, whatever dy holds (a "same" conv's dgrad reaches back there)
            dres = ctx.bk.keep_rows(dy, B, seq_len, ctx.kw["row_lens"]) if ctx.kw else dy
        return dx, *_un(ctx, dw, db), dres, None, None, None, None


class KeepRowsFn(torch.autograd.Function):
    """the rows [B seq_len, C] of a ragged batch with those from lens[b] on selected to exact 0 -- a select, not a product: what lies there
    may be NaN -- in a fresh buffer (ns2_zero_rows_lens); the backward is the same select on the cotangent.  lens: int32 [B] on the
    device, read by the kernel alone."""

    @staticmethod
    def forward(ctx, x, seq_len, lens):
        bk = _begin(ctx)
        ctx.cfg = (x.shape[0] // seq_len, seq_len, lens)
        return bk.keep_rows(x, *ctx.cfg)

    @staticmethod
    def backward(ctx, dy):
        return ctx.bk.keep_rows(dy, *ctx.cfg), None, None


class RowDotReluFn(torch.autograd.Function):
    """relu(Linear(dim, 1)(h)) -> [M]: a `to_pred` head of the DurationPitchPredictor (NS2:451-455); w [1, dim], b [1]"""

    @staticmethod
    def forward(ctx, h, w, b):
        bk = _begin(ctx)
        out = bk.row_dot_relu(h, w.detach().reshape(-1), b.detach())
        ctx.save_for_backward(h, w, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, w, out = ctx.saved_tensors
        dh, dw, db = ctx.bk.row_dot_relu_bwd(dout, out, h, w.detach().reshape(-1))
        dw, db = _un(ctx, dw, db)
        return dh, dw.reshape(w.shape), db


class EmbeddingFn(torch.autograd.Function):
    """token_emb(ids) with negative ids read as `pad_id` (NS2:281-284) -> [M, d]; the table's gradient is summed per id in a fixed order
    (bit-reproducible, unlike index_add_ on the GPU); the padding row gets its gradient like any other row, as upstream"""

    @staticmethod
    def forward(ctx, ids, table, pad_id):
        bk = _begin(ctx)
        ctx.ids, ctx.pad_id, ctx.rows = ids, pad_id, table.shape[0]
        return bk.embedding(ids, table.detach(), pad_id).reshape(ids.numel(), table.shape[1])

    @staticmethod
    def backward(ctx, dy):
        dy = _rowmajor(dy)
        return None, ctx.bk.embedding_bwd(ctx.ids, dy, ctx.rows, ctx.pad_id), None


class SkinnyLinearFn(torch.autograd.Function):
    """nn.Linear on rows = batch entries: `to_time_cond.1`, every FiLM / adaptive-norm `to_gamma_beta` / block `to_time_cond`
    (NS2:623, 744, 841), `to_prompt_cond.1` (NS2:860).  The weight-streaming fp32 kernel of the inference path in all three roles:
    y = x W^T + b;  dx = dy W (the weight as stored is already K-major for this product);  dW = dy^T x;  db = column sums."""

    @staticmethod
    def forward(ctx, x, w, b):
        bk = _begin(ctx)
        wt = bk.transpose_f32(w.detach())                                   # [K, J]
        y = bk.skinny(x.detach(), wt, b.detach() if b is not None else None)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        bk = ctx.bk
        x, w = ctx.saved_tensors
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = bk.skinny(dy, w.detach()) if ctx.needs_input_grad[0] else None  # [B, J] @ [J, K]
        dw = bk.skinny(bk.transpose_f32(dy), x.detach())                     # [J, B] @ [B, K]
        db = bk.colsum_rows(dy) if ctx.has_bias else None
        return dx, dw, db


def _lin(lin, x):
    return SkinnyLinearFn.apply(_c(x), lin.weight, lin.bias)


class CondProjectionsFn(torch.autograd.Function):
    """EVERY FiLM / adaptive-norm projection of one forward (the 32 Wavenet `to_time_cond`, the 24-36 `to_gamma_beta` Linears:
    NS2:623, 744) as ONE weight-streaming product, the way the sampler's executor runs them (model_exec.cpp: one [K, Jtot] matrix).
    They all read the same conditioning rows t [B, K]; per module the kernel had 32 workgroups on 256 CUs and the step paid
    171 launches of ~40 us.  y_all = t W_all^T + b_all;  dt = dy_all W_all;  dW_all = dy_all^T t, whose row blocks ARE the
    parameters' gradients (returned as views);  db_all = column sums.  Same fp32 FMAs per output as the per-module product, in
    another K split (the split follows the column count)."""

    @staticmethod
    def forward(ctx, t, *wb):
        bk = _begin(ctx)
        ws, bs = wb[0::2], wb[1::2]
        sizes = [int(w.shape[0]) for w in ws]
        W = torch.cat([w.detach() for w in ws], 0)                           # [Jtot, K]
        bias = torch.cat([b.detach() for b in bs], 0)
        y = bk.skinny(t.detach(), bk.transpose_f32(W), bias)                 # [B, Jtot]
        ctx.save_for_backward(t, W)
        ctx.sizes = sizes
        return tuple(o.contiguous() for o in y.split(sizes, dim=1))

    @staticmethod
    def backward(ctx, *dys):
        bk = ctx.bk
        t, W = ctx.saved_tensors
        B = t.shape[0]
        dy = torch.cat([d if d is not None else torch.zeros(B, n, dtype=t.dtype, device=t.device) for d, n in zip(dys, ctx.sizes)], 1)
        dt = bk.skinny(dy, W) if ctx.needs_input_grad[0] else None           # [B, Jtot] @ [Jtot, K]
        dW = bk.skinny(bk.transpose_f32(dy), t.detach())                     # [Jtot, B] @ [B, K]
        db = bk.colsum_rows(dy)
        grads = []
        for gw, gb in zip(dW.split(ctx.sizes, 0), db.split(ctx.sizes, 0)):
            grads += [gw, gb]
        return (dt, *grads)
