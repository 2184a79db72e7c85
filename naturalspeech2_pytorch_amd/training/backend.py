"""The ctypes backend: every method of `HipBackend` = launches of libns2hip on the current stream (C ABI: include/ns2hip.h "training")"""
import ctypes

import torch

from .. import _lib, ops
from .._lib import check
from ..ops import _p, _stream, round_up
from .packs import _PackedCache


class TPlanes:
    """transposed operand planes: `rows` rows of `ld` token columns, interleaved 128-byte lines along the token axis --
    bf16 [hi32 | lo32] (precision 3) or FMT_H8 [half32 | e5m2 | e5m2 remainder] (precision 4): 4 bytes per element either way"""
    __slots__ = ("buf", "rows", "ld", "precision")

    def __init__(self, rows, ld, device, precision=3):
        self.buf = torch.empty(rows, 2 * ld, dtype=torch.bfloat16, device=device)
        self.rows, self.ld, self.precision = rows, ld, precision

    def ptr(self, row_off=0):
        return self.buf.data_ptr() + row_off * 4 * self.ld          # 2 planes x 2 bytes per logical column


class HipBackend:
    """every method = launches of libns2hip on the current stream; torch provides the buffers.

    `precision` = the arithmetic of the GEMMs (forward, dgrad, wgrad) and the format of their operand planes: 3 = bf16 hi / lo
    planes, three bf16 products ("exact"); 4 = FMT_H8 lines, one IEEE-half product + both correction terms on the fp8 MFMA
    ("mixed": 2 MFMA units instead of 3; needs the loss scaling of `passes._Scale`).  The attention products and their operands
    (q, k, v, dO and the per-utterance transposes) are bf16 x3 at both precisions (`attn=True` arguments)."""
    name = "hip"

    def __init__(self, precision=3):
        assert precision in (3, 4)
        self.lib = _lib.load()
        self.prec = precision
        self.packs = _PackedCache(precision)

    # ---- weights
    def pack(self, key, params, make_src, parts=None):
        return self.packs.get(key, params, make_src, parts=parts)

    # ---- forward pieces
    def split(self, x, C=None):
        x = x if x.is_contiguous() else x.contiguous()
        return ops.split(x, precision=self.prec)

    @staticmethod
    def _rows(t, d):
        """[M, d] fp32 with row stride exactly d (kernels that take no stride for this operand)"""
        return t if (t.stride(1) == 1 and t.stride(0) == d) else t.contiguous()

    def rmsnorm(self, x, seq_len, gamma=None, cond=None):
        return ops.rmsnorm(x, seq_len=seq_len, gamma=gamma, cond=cond, precision=self.prec)

    def rmsnorm_f32(self, x, gamma):
        """RMSNorm(x) * gamma as fp32 [M, d] (the resampler's final norm, NS2:579: its output is a tensor of the graph, not an operand)"""
        return ops.rmsnorm(x, seq_len=0, gamma=gamma, want_f32=True, precision=3)[1]

    @staticmethod
    def _lens_kw(row_lens):
        """`row_lens` is handed on only when present: by default the calls below are the calls they were"""
        return {} if row_lens is None else {"row_lens": row_lens}

    def gemm_f32(self, pw, a, bias=None, resid=None, taps=0, dil=1, seq_len=0, pad_left=-1, row_lens=None):
        """-> fp32 [M, ldo] with ldo = round_up(N, 32); columns >= N are NOT written.  row_lens = (int32 [B] on the device, frames per
        utterance) of a ragged batch whose products skip (include/ns2hip_train.h): the row tiles hidden behind a length are
        not computed and come back as zero bits (with a residual too); an anticausal product (pad_left = 0 under taps > 1) needs zeros in
        the hidden rows of `a`"""
        return ops.linear_f32(pw, a, bias=bias, resid=resid, conv_taps=taps, dilation=dil, seq_len=seq_len, precision=self.prec,
                              pad_left=pad_left, ldo=round_up(pw.rows, 32), **self._lens_kw(row_lens))

    def gemm_split(self, pw, a, bias=None, taps=0, dil=1, seq_len=0, attn=False, row_lens=None):
        """-> operand planes; attn=True: attention operands (q | k | v), bf16 hi / lo lines whatever the GEMM arithmetic; row_lens: as in
        `gemm_f32` (hidden row tiles of the planes are zero bits)"""
        return ops.linear_split(pw, a, bias=bias, conv_taps=taps, dilation=dil, seq_len=seq_len, precision=self.prec,
                                out_precision=3 if attn and self.prec != 3 else None, **self._lens_kw(row_lens))

    def film_gate_fwd(self, h, film, seq_len, d):
        out = torch.empty(h.shape[0], d, dtype=torch.float32, device=h.device)
        check(self.lib.ns2_film_gate_fwd(h.data_ptr(), h.stride(0), film.data_ptr(), film.stride(0), seq_len, h.shape[0], d, out.data_ptr(), d,
                                         _stream()), "ns2_film_gate_fwd")
        return out

    def geglu_fwd(self, pre, f):
        M = pre.shape[0]
        out = ops._out_planes(M, round_up(f, 32), pre.device, self.prec)
        check(self.lib.ns2_geglu_fwd(pre.data_ptr(), pre.stride(0), M, f, out.hi, out.lo, out.ld, self.prec, _stream()), "ns2_geglu_fwd")
        return out

    def attention(self, q, q_col0, k, k_col0, vt, B, H, Nq, Nk, lens=None, head_dim=64):
        """bf16 x3 products on bf16 operands; the output o (the out-projection's operand) in the GEMM format.  lens: int32 [B] on the
        device, the utterances' lengths of a ragged batch (self-attention; include/ns2hip_train.h): rows of o from a length on are
        zero bits, their lse +inf.  head_dim 32 / 64 / 128 (include/ns2hip_train.h): head h at columns col0 + head_dim h"""
        return ops._attention_fwd(q, q_col0, k, k_col0, vt.ptr(), vt.ptr() + 64, vt.ld, B, H, Nq, Nk, head_dim ** -0.5, 3, head_dim=head_dim,
                                  o_precision=self.prec, want_lse=True, train_lens=lens)

    def attention_masked(self, q, q_col0, k, k_col0, vt, B, H, Nq, Nk, kmask=None, drop=None, head_dim=64):
        """`attention` with a key-padding mask (uint8 [B, Nk], 1 = attend) and / or dropout on P (`drop` = (p, seed tensor on the device, call
        index): csrc/dropout_keep.h) -- the attention of the conditioning encoders' training pass.  The products are bf16 x3 on bf16 operands
        whatever the backend's arithmetic; with a key mask alone the output o takes the GEMM format like `attention`'s (the kernel writes
        o in the format it is handed: `Model`'s resampler under `prompt_lens` in the mixed arithmetic).  Dropout stays with the exact one."""
        assert self.prec == 3 or drop is None, "the encoders train in the exact arithmetic"
        return ops._attention_fwd(q, q_col0, k, k_col0, vt.ptr(), vt.ptr() + 64, vt.ld, B, H, Nq, Nk, head_dim ** -0.5, 3, head_dim=head_dim,
                                  o_precision=self.prec, key_mask=kmask, want_lse=True, drop=drop)

    def dropout_keep_mask(self, seed, call, p, B, H, Nq, Nk):
        """debugging / tests: the keep mask the training attention kernels apply for these arguments, uint8 [B, H, Nq, Nk]"""
        out = torch.empty(B, H, Nq, Nk, dtype=torch.uint8, device=seed.device)
        check(self.lib.ns2_dropout_keep_mask(seed.data_ptr(), call, p, B, H, Nq, Nk, out.data_ptr(), _stream()), "ns2_dropout_keep_mask")
        return out

    def silu_fwd(self, pre, C):
        """SiLU of the fp32 pre-activation pre [M, >= C] -> fp32 [M, round_up(C, 32)] (columns >= C not written)"""
        out = torch.empty(pre.shape[0], round_up(C, 32), dtype=torch.float32, device=pre.device)
        check(self.lib.ns2_silu_fwd(pre.data_ptr(), pre.stride(0), pre.shape[0], C, out.data_ptr(), out.stride(0), _stream()), "ns2_silu_fwd")
        return out

    def silu_bwd(self, dy, pre, C):
        dx = torch.empty(pre.shape[0], round_up(C, 32), dtype=torch.float32, device=pre.device)
        check(self.lib.ns2_silu_bwd(dy.data_ptr(), dy.stride(0), pre.data_ptr(), pre.stride(0), pre.shape[0], C, dx.data_ptr(), dx.stride(0), _stream()),
              "ns2_silu_bwd")
        return dx

    def relu_fwd(self, pre, C):
        """ReLU of the fp32 pre-activation pre [M, >= C] -> fp32 [M, round_up(C, 32)] (columns >= C not written): the Aligner's conv stacks"""
        out = torch.empty(pre.shape[0], round_up(C, 32), dtype=torch.float32, device=pre.device)
        check(self.lib.ns2_relu_fwd(pre.data_ptr(), pre.stride(0), pre.shape[0], C, out.data_ptr(), out.stride(0), _stream()), "ns2_relu_fwd")
        return out

    def relu_bwd(self, dy, pre, C):
        dx = torch.empty(pre.shape[0], round_up(C, 32), dtype=torch.float32, device=pre.device)
        check(self.lib.ns2_relu_bwd(dy.data_ptr(), dy.stride(0), pre.data_ptr(), pre.stride(0), pre.shape[0], C, dx.data_ptr(), dx.stride(0), _stream()),
              "ns2_relu_bwd")
        return dx

    # ---- Aligner: distances + softmax and their backward, the forward-sum / bin losses (aligner.py:62-90, 132-183)
    def align_attn(self, q, k, text_lens, B):
        """queries [B T, C], keys [B n, C] fp32 -> (aln_log [B, 1, T, n], aln_soft [B, n, T]): ns2_align_attn, the inference kernel"""
        return ops.align_attn(q, k, text_lens, B)

    def align_attn_bwd(self, q, k, log, soft, g_log, g_soft, text_lens):
        """-> (dq [B T, C], dk [B n, C]); g_log [B, 1, T, n] / g_soft [B, n, T]: either may be None"""
        B, _, T, n = log.shape
        C = q.shape[1]
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        nbytes = self.lib.ns2_align_attn_bwd_workspace_bytes(B, T, n, C)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
        check(self.lib.ns2_align_attn_bwd(q.data_ptr(), k.data_ptr(), log.data_ptr(), soft.data_ptr(), _p(g_log), _p(g_soft), text_lens.data_ptr(),
                                          B, T, n, C, dq.data_ptr(), dk.data_ptr(), ws.data_ptr(), nbytes, _stream()), "ns2_align_attn_bwd")
        return dq, dk

    def align_losses_fwd(self, log, text_lens, mel_lens, blank, hard=None, want_fs=True, want_bin=False):
        """aln_log [B, 1, T, n] fp32 contiguous, int32 lengths on the device, hard [B, n, T] (bin loss) -> (fs_loss, bin_loss, workspace):
        0-dim device tensors (None where not wanted); `workspace` is what `align_losses_bwd` reads"""
        B, _, T, n = log.shape
        out = torch.empty(2, dtype=torch.float32, device=log.device)
        nbytes = self.lib.ns2_align_losses_workspace_bytes(B, T, n)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=log.device)
        check(self.lib.ns2_align_losses_fwd(log.data_ptr(), _p(hard), text_lens.data_ptr(), _p(mel_lens), B, T, n, float(blank),
                                            out[0:].data_ptr() if want_fs else None, out[1:].data_ptr() if want_bin else None, ws.data_ptr(), nbytes,
                                            _stream()), "ns2_align_losses_fwd")
        return (out[0] if want_fs else None), (out[1] if want_bin else None), ws

    def align_losses_bwd(self, log, text_lens, mel_lens, blank, ws, hard=None, g_fs=None, g_bin=None):
        """-> d aln_log [B, 1, T, n]; g_fs / g_bin: fp32 device scalars (None = that loss takes no part)"""
        B, _, T, n = log.shape
        d_log = torch.empty_like(log)
        check(self.lib.ns2_align_losses_bwd(log.data_ptr(), _p(hard), text_lens.data_ptr(), _p(mel_lens), _p(g_fs), _p(g_bin), B, T, n, float(blank),
                                            d_log.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ns2_align_losses_bwd")
        return d_log

    # ---- the RVQ cross-entropy term of the training loss (codec.py ResidualVQCrossEntropy; csrc/rvq_ce.hip)
    def rvq_cross_entropy(self, x, codebooks, cb_norm, indices, need_grad=True, lens=None):
        """x [M, 128] fp32, indices [M, Q] int64 -> (loss 0-dim, quantized_out [M, 128], G [M, 128] = d loss / d x or None); fp32 whatever
        the arithmetic of the pass.  lens [B] int32 on the device: the ragged batch of ns2_rvq_ce_lens (M = B n)"""
        loss, _, quant, G = ops.rvq_cross_entropy(x, codebooks, cb_norm, indices, need_grad, **({} if lens is None else dict(lens=lens)))
        return loss, quant, G

    def embedding(self, ids, table, pad_id):
        return ops.embedding(ids, table, pad_id)

    def embedding_bwd(self, ids, dy, rows, pad_id):
        """d table [rows, d] from dy [M, >= d] rows, summed per id in ascending token order (bit-reproducible; negative ids = pad_id)"""
        d = dy.shape[1]
        ids = ids.reshape(-1).to(torch.int64).contiguous()
        dw = torch.empty(rows, d, dtype=torch.float32, device=dy.device)
        check(self.lib.ns2_embedding_bwd(ids.data_ptr(), ids.numel(), pad_id, dy.data_ptr(), dy.stride(0), rows, d, dw.data_ptr(), _stream()),
              "ns2_embedding_bwd")
        return dw

    # ---- DurationPitchPredictor: GroupNorm + SiLU (+ residual) of a ResnetBlock, the Linear(dim, 1) + ReLU heads
    def groupnorm_silu_fwd(self, x, B, n, weight, bias, groups, eps, resid=None, row_lens=None):
        """x fp32 [B n, >= C] -> (y [B n, C] fp32, the rows [B n, C] the kernel read, stats): `stats` holds the per-chunk statistics slots
        of ns2_groupnorm_silu, which `groupnorm_silu_bwd` recombines (the same mean and rstd, bit for bit).  row_lens: int32 [B] on the
        device, rows per utterance of a ragged batch (ns2_groupnorm_silu_lens: statistics over the rows before a length, rows of x and
        resid from it on not read, rows of y there zeros); hand the same lengths to `groupnorm_silu_bwd`"""
        C = weight.shape[0]
        x = self._rows(x[:, :C], C)
        if resid is not None:
            resid = self._rows(resid[:, :C], C)
        y = torch.empty(B * n, C, dtype=torch.float32, device=x.device)
        stats = torch.empty(self.lib.ns2_groupnorm_workspace_bytes(B, n, C, groups), dtype=torch.uint8, device=x.device)
        if row_lens is not None:
            assert row_lens.dtype == torch.int32 and row_lens.is_cuda and row_lens.shape == (B,) and row_lens.is_contiguous()
            check(self.lib.ns2_groupnorm_silu_lens(x.data_ptr(), B, n, C, groups, weight.data_ptr(), bias.data_ptr(), float(eps), _p(resid),
                                                   row_lens.data_ptr(), y.data_ptr(), None, None, 0, 3, stats.data_ptr(), stats.numel(), _stream()),
                  "ns2_groupnorm_silu_lens")
            return y, x, stats
        check(self.lib.ns2_groupnorm_silu(x.data_ptr(), B, n, C, groups, weight.data_ptr(), bias.data_ptr(), float(eps), _p(resid), y.data_ptr(), None, None,
                                          0, 3, stats.data_ptr(), stats.numel(), _stream()), "ns2_groupnorm_silu")
        return y, x, stats

    def groupnorm_silu_bwd(self, dy, x, stats, B, n, weight, bias, groups, eps, row_lens=None):
        """-> (dx [B n, C], dweight [C], dbias [C]); x, stats: what `groupnorm_silu_fwd` returned.  row_lens: what it got
        (ns2_groupnorm_silu_bwd_lens, include/ns2hip_train.h): rows of dy and x from a length on are not read, rows of dx
        there are zero bits"""
        C = weight.shape[0]
        dx = torch.empty(B * n, C, dtype=torch.float32, device=x.device)
        dwb = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        ws = torch.empty(self.lib.ns2_groupnorm_silu_bwd_workspace_bytes(B, n, C), dtype=torch.uint8, device=x.device)
        if row_lens is not None:
            assert row_lens.dtype == torch.int32 and row_lens.is_cuda and row_lens.shape == (B,) and row_lens.is_contiguous()
            check(self.lib.ns2_groupnorm_silu_bwd_lens(dy.data_ptr(), dy.stride(0), x.data_ptr(), B, n, C, groups, weight.data_ptr(), bias.data_ptr(),
                                                       float(eps), stats.data_ptr(), stats.numel(), row_lens.data_ptr(), dx.data_ptr(), dwb.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), _stream()), "ns2_groupnorm_silu_bwd_lens")
            return dx, dwb[:C], dwb[C:]
        check(self.lib.ns2_groupnorm_silu_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), B, n, C, groups, weight.data_ptr(), bias.data_ptr(), float(eps),
                                              stats.data_ptr(), stats.numel(), dx.data_ptr(), dwb.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "ns2_groupnorm_silu_bwd")
        return dx, dwb[:C], dwb[C:]

    def keep_rows(self, t, B, n, lens):
        """a fresh contiguous copy of the fp32 rows t [B n, C] (C % 4 == 0) whose rows from lens[b] on are zero bits (ns2_zero_rows_lens):
        the select of a ragged conditioning pass, and its backward on the cotangent.  lens: int32 [B] on the device.  Rows that are not
        whole 16-byte vectors (C % 4 != 0: a codebook dimension) take the same select as a torch.where on the device"""
        if t.shape[1] % 4:
            keep = torch.arange(n, device=t.device)[None] < lens.clamp(1, n)[:, None]
            return torch.where(keep.reshape(B * n, 1), t, torch.zeros((), dtype=t.dtype, device=t.device))
        return ops.zero_rows(t.clone(memory_format=torch.contiguous_format), B, n, lens)

    def row_dot_relu(self, h, w, b):
        """relu(h[:, :K] . w + b) -> [M]"""
        return ops.row_dot(h, w, b, relu=True)

    def row_dot_relu_bwd(self, dout, out, h, w):
        """-> (dh [M, K], dw [K], db [1]) of out = relu(h . w + b)"""
        M, K = h.shape[0], w.numel()
        dout = dout if dout.is_contiguous() else dout.contiguous()
        dh = torch.empty(M, K, dtype=torch.float32, device=h.device)
        dwb = torch.empty(K + 1, dtype=torch.float32, device=h.device)
        ws = torch.empty(self.lib.ns2_row_dot_relu_bwd_workspace_bytes(M, K), dtype=torch.uint8, device=h.device)
        check(self.lib.ns2_row_dot_relu_bwd(dout.data_ptr(), out.data_ptr(), h.data_ptr(), h.stride(0), w.data_ptr(), M, K, dh.data_ptr(), K,
                                            dwb.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ns2_row_dot_relu_bwd")
        return dh, dwb[:K], dwb[K:]

    # ---- rows = batch entries: the conditioning Linears (weight-streaming kernel of the inference path, fp32)
    def skinny(self, x, wt, bias=None):
        """x [R, K] @ wt [K, J] (+ bias) in fp32 (ns2_skinny_linear: deterministic split-K)"""
        return ops.skinny_linear(x if x.is_contiguous() else x.contiguous(), wt if wt.is_contiguous() else wt.contiguous(), bias)

    def transpose_f32(self, x):
        x = x if x.is_contiguous() else x.contiguous()
        R, C = x.shape
        out = torch.empty(C, R, dtype=torch.float32, device=x.device)
        check(self.lib.ns2_transpose_f32(x.data_ptr(), 1, R, C, out.data_ptr(), _stream()), "ns2_transpose_f32")
        return out

    def colsum_rows(self, x):
        """sum over the rows of a small [R, J] matrix in a fixed order (bias gradients of the conditioning Linears)"""
        x = x if x.is_contiguous() else x.contiguous()
        out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
        check(self.lib.ns2_reduce_slices(x.data_ptr(), 1, x.shape[0], x.shape[1], out.data_ptr(), 0, _stream()), "ns2_reduce_slices")
        return out

    # ---- backward pieces
    def grad_prep(self, x, C, want_row=False, want_t=False, want_colsum=False, seq_len=0, per_batch=False, t_rows=None, attn=False):
        """x fp32 [M, >= C] -> (row planes [M, round_up(C, 32)], transposed planes, column sums [C]); attn=True: operands of the
        attention backward (bf16 hi / lo), else GEMM operands in the backend's format"""
        M, dev = x.shape[0], x.device
        if not (want_row or want_t or want_colsum):
            return None, None, None
        prec = 3 if attn else self.prec
        row = ops._out_planes(M, round_up(C, 32), dev, prec) if want_row else None
        tp, ld_t = None, 0
        if want_t:
            ld_t = round_up(seq_len if per_batch else M, 32)
            t_rows = t_rows or C
            tp = TPlanes((M // seq_len) * t_rows if per_batch else t_rows, ld_t, dev, prec)
        part = None
        if want_colsum:
            S = self.lib.ns2_grad_prep_slices(M, ld_t)
            part = torch.empty(S, C, dtype=torch.float32, device=dev)
        check(self.lib.ns2_grad_prep(x.data_ptr(), x.stride(0), M, C, seq_len, 0, row.hi if row else None, row.lo if row else None,
                                     row.ld if row else 0, tp.ptr() if tp else None, tp.ptr() + 64 if tp else None, ld_t, t_rows or 0,
                                     int(per_batch and want_t), _p(part), prec, _stream()), "ns2_grad_prep")
        cs = None
        if want_colsum:
            cs = torch.empty(C, dtype=torch.float32, device=dev)
            check(self.lib.ns2_reduce_slices(part.data_ptr(), 1, part.shape[0], C, cs.data_ptr(), 0, _stream()), "ns2_reduce_slices")
        return row, tp, cs

    def transpose(self, p, col0, C, seq_len, shifts=(0,), per_batch=False, pad_rows=256):
        """planes [M, ld] columns [col0, col0 + C) -> transposed planes; one row block of Cp = round_up(C, 32) rows per shift
        (the taps of a conv's weight gradient), rows zero-padded to what a W operand of ns2_wgrad may read"""
        M = p.rows
        Cp = round_up(C, 32)
        prec = p.precision                       # the transposed planes keep the format of the planes they come from
        assert prec in (3, 4)
        if per_batch:
            B = M // seq_len
            tp = TPlanes(B * C, round_up(seq_len, 32), p.device, prec)
            check(self.lib.ns2_planes_transpose(p.hi, p.lo, p.ld, col0, M, C, seq_len, 0, tp.ptr(), tp.ptr() + 64, tp.ld, C, 1, prec, _stream()),
                  "ns2_planes_transpose")
            return tp
        T = len(shifts)
        # a W operand is read in whole 256-row tiles from wherever a wgrad starts (row 0 for all taps, row 2 Cp for res_conv)
        rows = max((T - 1) * Cp + round_up(Cp, pad_rows), round_up(T * Cp, pad_rows))
        tp = TPlanes(rows, round_up(M, 32), p.device, prec)
        for t, sh in enumerate(shifts):
            t_rows = Cp if t < T - 1 else rows - (T - 1) * Cp
            check(self.lib.ns2_planes_transpose(p.hi, p.lo, p.ld, col0, M, C, seq_len, sh, tp.ptr(t * Cp), tp.ptr(t * Cp) + 64, tp.ld, t_rows, 0,
                                                prec, _stream()), "ns2_planes_transpose")
        return tp

    def wgrad(self, dyt, xt, R, T, K, row_off=0):
        """dW [R, K, T] = dY^T X_t ; xt: T blocks of Kp = round_up(K, 32) rows starting at row_off"""
        Kp = round_up(K, 32)
        assert dyt.precision == xt.precision == self.prec, "wgrad operands must be in the backend's GEMM format"
        nbytes = self.lib.ns2_wgrad_workspace_bytes(R, T * Kp, dyt.ld)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dyt.buf.device)
        dw = torch.empty(R, K, T, dtype=torch.float32, device=dyt.buf.device)
        check(self.lib.ns2_wgrad(dyt.ptr(), dyt.ptr() + 64, xt.ptr(row_off), xt.ptr(row_off) + 64, dyt.ld, R, T, Kp, K, dw.data_ptr(), ws.data_ptr(),
                                 nbytes, self.prec, _stream()), "ns2_wgrad")
        return dw

    def wgrad_rows_ok(self, R, T, K, seq_len, M):
        """does ns2_wgrad_rows form this gradient from the token-major planes (else: transposed copies + ns2_wgrad)"""
        return (T == 1 or seq_len >= 32) and bool(self.lib.ns2_wgrad_rows_preferred(R, T * round_up(K, 32), M))

    def wgrad_rows(self, dy, x, R, T, K, dil=1, seq_len=0, row_lens=None):
        """dW [R, K, T] = sum_m dY[m, r] X[m - (T - 1 - t) dil, k] from the ROW planes dy [M, >= R] and x [M, >= round_up(K, 32)] themselves
        (gemm2.hip TR: LDS transpose reads; the shifts of a conv's taps are row offsets of the loads).  row_lens = (int32 [B] on the
        device, frames per utterance): ns2_wgrad_rows_lens -- the 32-token K tiles hidden behind a length are neither fetched nor
        multiplied; same slots, same order of their sum"""
        Kp = round_up(K, 32)
        assert dy.precision == x.precision == self.prec and dy.rows == x.rows, "wgrad operands must be planes of the same tokens in the backend's GEMM format"
        M = dy.rows
        nbytes = self.lib.ns2_wgrad_workspace_bytes(R, T * Kp, round_up(M, 32))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
        dw = torch.empty(R, K, T, dtype=torch.float32, device=dy.device)
        if row_lens is not None:
            lens, n = row_lens
            assert lens.dtype == torch.int32 and lens.is_cuda and lens.is_contiguous() and lens.numel() * n == M and seq_len in (0, n)
            check(self.lib.ns2_wgrad_rows_lens(dy.hi, dy.lo, dy.ld, x.hi, x.lo, x.ld, M, R, T, Kp, K, dil, n, dw.data_ptr(), ws.data_ptr(),
                                               nbytes, self.prec, lens.data_ptr(), _stream()), "ns2_wgrad_rows_lens")
            return dw
        check(self.lib.ns2_wgrad_rows(dy.hi, dy.lo, dy.ld, x.hi, x.lo, x.ld, M, R, T, Kp, K, dil, seq_len if T > 1 else 0, dw.data_ptr(), ws.data_ptr(),
                                      nbytes, self.prec, _stream()), "ns2_wgrad_rows")
        return dw

    def film_gate_bwd(self, dg, h, film, B, seq_len, d):
        S = self.lib.ns2_film_gate_slices(seq_len)
        dh = torch.empty(h.shape[0], d, dtype=torch.float32, device=h.device)
        part = torch.empty(B * S, 2 * d, dtype=torch.float32, device=h.device)
        check(self.lib.ns2_film_gate_bwd(dg.data_ptr(), dg.stride(0), h.data_ptr(), h.stride(0), film.data_ptr(), film.stride(0), B, seq_len, d,
                                         dh.data_ptr(), d, part.data_ptr(), _stream()), "ns2_film_gate_bwd")
        dfilm = torch.empty(B, 2 * d, dtype=torch.float32, device=h.device)
        check(self.lib.ns2_reduce_slices(part.data_ptr(), B, S, 2 * d, dfilm.data_ptr(), 0, _stream()), "ns2_reduce_slices")
        return dh, dfilm

    def geglu_bwd(self, dh, pre, f):
        M = pre.shape[0]
        dpre = torch.empty(M, round_up(2 * f, 32), dtype=torch.float32, device=pre.device)
        check(self.lib.ns2_geglu_bwd(dh.data_ptr(), dh.stride(0), pre.data_ptr(), pre.stride(0), M, f, dpre.data_ptr(), dpre.stride(0), _stream()),
              "ns2_geglu_bwd")
        return dpre

    def rmsnorm_bwd(self, x, dy, B, seq_len, d, gamma=None, cond=None, dx_add=None):
        """-> (dx [M, d] = dx_add + dL/dx, dcond [B, 2 d] or None, dgamma [d] or None)"""
        S = self.lib.ns2_rmsnorm_bwd_slices(seq_len)
        dev = x.device
        dx = torch.empty(B * seq_len, d, dtype=torch.float32, device=dev)
        cpart = torch.empty(B * S, 2 * d, dtype=torch.float32, device=dev) if cond is not None else None
        gpart = torch.empty(B * S, d, dtype=torch.float32, device=dev) if gamma is not None else None
        if dx_add is not None:
            dx_add = self._rows(dx_add[:, :d], d)          # the kernel reads dx_add with dx's row stride (= d)
        check(self.lib.ns2_rmsnorm_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), _p(gamma), _p(cond),
                                       cond.stride(0) if cond is not None else 0, B, seq_len, d, _p(dx_add), dx.data_ptr(), d, _p(cpart),
                                       _p(gpart), _stream()), "ns2_rmsnorm_bwd")
        dcond = dgamma = None
        if cond is not None:
            dcond = torch.empty(B, 2 * d, dtype=torch.float32, device=dev)
            check(self.lib.ns2_reduce_slices(cpart.data_ptr(), B, S, 2 * d, dcond.data_ptr(), 0, _stream()), "ns2_reduce_slices")
        if gamma is not None:
            dgamma = torch.empty(d, dtype=torch.float32, device=dev)
            check(self.lib.ns2_reduce_slices(gpart.data_ptr(), 1, B * S, d, dgamma.data_ptr(), 0, _stream()), "ns2_reduce_slices")
        return dx, dcond, dgamma

    def attention_delta(self, do, o, B, H, Nq, head_dim=64):
        delta = torch.empty(B, H, Nq, dtype=torch.float32, device=do.device)
        if head_dim != 64:
            check(self.lib.ns2_attention_delta_hd(do.data_ptr(), do.stride(0), o.hi, o.lo, o.ld, B, H, Nq, head_dim, delta.data_ptr(), o.precision,
                                                  _stream()), "ns2_attention_delta_hd")
            return delta
        check(self.lib.ns2_attention_delta(do.data_ptr(), do.stride(0), o.hi, o.lo, o.ld, B, H, Nq, delta.data_ptr(), o.precision, _stream()),
              "ns2_attention_delta")
        return delta

    def new_planes(self, M, C):
        """uninitialised operand planes [M, round_up(C, 32)] in the backend's GEMM format (a kernel is about to fill every column)"""
        return ops._out_planes(M, round_up(C, 32), torch.device("cuda", torch.cuda.current_device()), self.prec)

    def attention_bwd_masked(self, *args, kmask=None, drop=None, **kw):
        """`attention_bwd` of a forward that ran `attention_masked` with the same `kmask` / `drop`"""
        self.attention_bwd(*args, **kw, kmask=kmask, drop=drop)

    def attention_bwd(self, q, q_col0, k, k_col0, v, v_col0, do_row, lse, delta, B, H, Nq, Nk, dq=None, dkv=None, planes=None, kmask=None,
                      drop=None, lens=None, head_dim=64):
        """dq: (fp32 tensor [B*Nq, ld], col0) or None; dkv: (tensor [B*Nk, ld], k col0, v col0) or None;
        planes: (operand planes [B*N, ld], dq col0, dk col0, dv col0) -- self attention: the three gradients leave the kernels as the
        operand of the q | k | v projection's dgrad / wgrad GEMMs instead of fp32 + a conversion pass;
        kmask / drop: what the forward (`attention_masked`) got, None = neither; lens: what the forward (`attention`) got -- gradient rows
        from a length on are written as zeros; head_dim: what the forward got (other than 64: ns2_attention_bwd_hd)"""
        a = _lib.AttnBwdArgs()
        a.q_hi, a.q_lo, a.ldq, a.q_col0 = q.hi, q.lo, q.ld, q_col0
        a.k_hi, a.k_lo, a.ldk, a.k_col0 = k.hi, k.lo, k.ld, k_col0
        a.v_hi, a.v_lo, a.ldv, a.v_col0 = v.hi, v.lo, v.ld, v_col0
        a.do_hi, a.do_lo, a.lddo = do_row.hi, do_row.lo, do_row.ld
        a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
        if dq is not None:
            a.dq, a.lddq, a.dq_col0 = dq[0].data_ptr(), dq[0].stride(0), dq[1]
        if dkv is not None:
            a.dk, a.lddk, a.dk_col0 = dkv[0].data_ptr(), dkv[0].stride(0), dkv[1]
            a.dv, a.lddv, a.dv_col0 = dkv[0].data_ptr(), dkv[0].stride(0), dkv[2]
        if planes is not None:
            gp, a.dq_col0, a.dk_col0, a.dv_col0 = planes
            assert gp.precision == self.prec
            a.gp_hi, a.gp_lo, a.gp_ld, a.gp_precision, a.gp_q, a.gp_kv = gp.hi, gp.lo, gp.ld, self.prec, 1, 1
        a.B, a.H, a.Nq, a.Nk, a.scale = B, H, Nq, Nk, head_dim ** -0.5
        a.key_mask = _p(kmask)
        if drop is not None:
            a.dropout_p, a.dropout_seed, a.dropout_call = drop[0], _p(drop[1]), drop[2]
        if head_dim != 64:
            check(self.lib.ns2_attention_bwd_hd(ctypes.byref(a), head_dim, _p(lens), _stream()), "ns2_attention_bwd_hd")
        elif lens is not None:
            check(self.lib.ns2_attention_bwd_lens(ctypes.byref(a), lens.data_ptr(), _stream()), "ns2_attention_bwd_lens")
        else:
            check(self.lib.ns2_attention_bwd(a, _stream()), "ns2_attention_bwd")
