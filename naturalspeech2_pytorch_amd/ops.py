"""Thin torch-tensor wrappers over the op-level C ABI of libns2hip (include/ns2hip.h).

PyTorch is plumbing here: device memory and the current HIP stream.  Every function launches hand-written HIP
kernels through ctypes; nothing in this module computes with torch ops.
"""
import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import check

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f32(t: torch.Tensor) -> torch.Tensor:
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expected a contiguous fp32 CUDA tensor"
    return t


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class Planes:
    """A split-plane matrix [rows, ld] held by the library's layout (csrc/ns2_common.h).  `ld` is always the LOGICAL column
    count (a multiple of 32).  Formats (`fmt`):

      "bf16"  with a lo plane ("interleaved", what precision 3 needs) `buf` is ONE bf16 tensor [rows, 2*ld]: every 32 logical
              columns occupy a 128-byte line [hi(32) | lo(32)], so the lo pointer is the hi pointer + 32 elements; without
              (precision 1) `buf` is the dense [rows, ld] hi plane;
      "f16"   one dense IEEE-half plane [rows, ld] (precision 2, and the attention operands of precision 4);
      "h8"    interleaved 128-byte lines [half(32) | e5m2(x)(32 bytes) | e5m2((x - half(x)) * 2^12)(32 bytes)] (precision 4).
    """
    __slots__ = ("buf", "rows", "ld", "has_lo", "fmt")

    def __init__(self, buf: torch.Tensor, rows: int, ld: int, has_lo: bool, fmt: str = "bf16"):
        assert fmt in ("bf16", "f16", "h8")
        assert not (fmt == "f16" and has_lo), "IEEE-half planes have no lo part"
        assert not (fmt == "h8" and not has_lo), "h8 planes are interleaved lines"
        self.buf, self.rows, self.ld, self.has_lo, self.fmt = buf, rows, ld, has_lo, fmt

    @property
    def f16(self):
        return self.fmt == "f16"

    @property
    def precision(self):
        """a precision whose kernels read / write this format"""
        return {"bf16": 3 if self.has_lo else 1, "f16": 2, "h8": 4}[self.fmt]

    @property
    def device(self):
        return self.buf.device

    @property
    def hi(self) -> int:
        """device address of the hi plane (what the C ABI takes as x_hi)"""
        return self.buf.data_ptr()

    @property
    def lo(self) -> Optional[int]:
        """device address of the second half of the lines = hi + 32 elements, or None for a dense single plane"""
        return self.buf.data_ptr() + 64 if self.has_lo else None

    def hi_plane(self) -> torch.Tensor:
        """the logical hi plane as a dense [rows, ld] 16-bit tensor (copy)"""
        if not self.has_lo:
            return self.buf.reshape(self.rows, self.ld).clone()
        return self.buf.reshape(self.rows, self.ld // 32, 2, 32)[:, :, 0, :].reshape(self.rows, self.ld).contiguous()

    def byte_planes(self):
        """h8 only: (e5m2(x), e5m2((x - half(x)) * 2^12)) as uint8 tensors [rows, ld]"""
        assert self.fmt == "h8"
        b = self.buf.reshape(self.rows, self.ld // 32, 2, 32)[:, :, 1, :].contiguous().view(torch.uint8)
        b = b.reshape(self.rows, self.ld // 32, 64)
        return b[:, :, :32].reshape(self.rows, self.ld).contiguous(), b[:, :, 32:].reshape(self.rows, self.ld).contiguous()

    def hi_only(self) -> "Planes":
        return Planes(self.hi_plane(), self.rows, self.ld, False, "f16" if self.fmt != "bf16" else "bf16")


def _fmt_of(precision: int, attention_operand: bool = False):
    """(has_lo, fmt) of what a kernel writes at `precision`; attention operands (q, k, V^T) are IEEE half at precision 4"""
    if precision == 2 or (precision == 4 and attention_operand):
        return False, "f16"
    if precision == 4:
        return True, "h8"
    return True, "bf16"              # precision 1 kernels read the hi plane of the interleaved layout too


def empty_planes(rows: int, cols: int, device, lo: bool = True, zero: bool = False, fmt: str = "bf16") -> Planes:
    lo = (lo and fmt == "bf16") or fmt == "h8"
    assert cols % 32 == 0 or not lo, "interleaved split planes come in 32-column blocks"
    alloc = torch.zeros if zero else torch.empty
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    return Planes(alloc(rows, cols * (2 if lo else 1), dtype=dt, device=device), rows, cols, lo, fmt)


def _out_planes(rows, cols, device, precision, attention_operand=False, zero=False):
    lo, fmt = _fmt_of(precision, attention_operand)
    return empty_planes(rows, cols, device, lo, zero, fmt)


def split(x: torch.Tensor, ldo: Optional[int] = None, lo: bool = True, precision: int = 3) -> Planes:
    """fp32 [M, d] -> split planes [M, ldo] (zero padded) in the operand format of `precision`."""
    x = _f32(x)
    M, d = x.shape
    ldo = ldo or round_up(d, 32)
    has_lo, fmt = _fmt_of(precision)
    out = empty_planes(M, ldo, x.device, lo and has_lo, fmt=fmt)
    check(_lib.load().ns2_split_f32(x.data_ptr(), d, M, d, out.hi, out.lo, ldo, out.precision, _stream()), "ns2_split_f32")
    return out


def join(p: Planes, d: Optional[int] = None) -> torch.Tensor:
    M, ld = p.rows, p.ld
    d = d or ld
    out = torch.empty(M, d, dtype=torch.float32, device=p.device)
    check(_lib.load().ns2_join_f32(p.hi, p.lo, ld, out.data_ptr(), d, M, d, p.precision, _stream()), "ns2_join_f32")
    return out


class PackedWeight:
    """Library-owned packed weight (ns2_weight)."""

    def __init__(self, w: torch.Tensor, geglu: bool = False, extra1x1: Optional[torch.Tensor] = None, precision: int = 3):
        """precision 1 / 3: interleaved bf16 planes (serve both); 2: dense IEEE half; 4: h8 lines (each serves only itself)"""
        import ctypes
        w = _f32(w)
        self.precision = precision
        self.rows, self.cols = w.shape[0], w.shape[1]
        self.taps = w.shape[2] if w.ndim == 3 else 1
        self.geglu = geglu
        self.has_extra = extra1x1 is not None
        self.cols_p = round_up(self.cols, 32)
        h = ctypes.c_void_p()
        ex = _f32(extra1x1) if extra1x1 is not None else None
        check(_lib.load().ns2_weight_pack(w.data_ptr(), self.rows, self.cols, self.taps, int(geglu), _p(ex), precision,
                                          ctypes.byref(h), _stream()), "ns2_weight_pack")
        self.handle = h

    def tile_conv3(self) -> "PackedWeight":
        """give a k = 3 conv weight packed at precision 2 the tiled images of the dedicated FF causal conv kernel (include/ns2hip.h)"""
        check(_lib.load().ns2_weight_tile_conv3(self.handle, _stream()), "ns2_weight_tile_conv3")
        return self

    def tile_wavenet(self) -> "PackedWeight":
        """give a WavenetResBlock weight (taps = 3 + extra1x1) packed at precision 4 the tiled images of the lean block kernel (include/ns2hip.h)"""
        check(_lib.load().ns2_weight_tile_wavenet(self.handle, _stream()), "ns2_weight_tile_wavenet")
        return self

    def tile_linear(self) -> "PackedWeight":
        """give a linear weight packed at precision 4 the tiled images of the lean mixed linear kernel (include/ns2hip.h)"""
        check(_lib.load().ns2_weight_tile_linear(self.handle, _stream()), "ns2_weight_tile_linear")
        return self

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().ns2_weight_free(self.handle)
                self.handle = None
        except Exception:
            pass


def _linear(w: PackedWeight, a: Planes, M: int, precision: int, row_lens=None, **fields):
    """The one place that fills a ns2_linear_args (include/ns2hip.h) and calls ns2_linear.  `fields`: the block's other fields by name
    (device addresses or ints; what is not named stays zero = feature off).  row_lens = (int32 [B] on the device, frames per utterance)
    of a ragged TRAINING batch: the same block goes to ns2_linear_lens_zero (include/ns2hip.h) -- hidden row tiles are
    skipped and stored as zero bits in every output; None (the default): ns2_linear, the same call and bits as ever."""
    args = _lib.LinearArgs(w=w.handle, a_hi=a.hi, a_lo=a.lo, lda=a.ld, M=M, precision=precision, **fields)
    if row_lens is not None:
        lens, n = row_lens
        assert lens.dtype == torch.int32 and lens.is_cuda and lens.is_contiguous() and lens.numel() * n == M
        import ctypes
        check(_lib.load().ns2_linear_lens_zero(ctypes.byref(args), lens.data_ptr(), n, _stream()), "ns2_linear_lens_zero")
        return
    check(_lib.load().ns2_linear(args, _stream()), "ns2_linear")


def linear_f32(w: PackedWeight, a: Planes, M: Optional[int] = None, bias=None, resid=None, conv_taps=0, dilation=1,
               seq_len=0, precision=3, pad_left=-1, act=0, ldo: Optional[int] = None, row_lens=None) -> torch.Tensor:
    """-> fp32 [M, ldo] (ldo defaults to the weight's rows; columns beyond them are NOT written); resid: fp32 rows of any row stride;
    row_lens: `_linear`'s (a ragged training batch: hidden row tiles come back as zeros)"""
    M = M or a.rows
    out = torch.empty(M, ldo or w.rows, dtype=torch.float32, device=a.device)
    _linear(w, a, M, precision, row_lens=row_lens, conv_taps=conv_taps, dilation=dilation, seq_len=seq_len, pad_left=pad_left, bias=_p(bias), act=act,
            out_f32=out.data_ptr(), ldo_f=out.shape[1], resid=_p(resid), ldr=resid.stride(0) if resid is not None else 0)
    return out


def conv3_input_ld(cols: int) -> int:
    """row length (elements) of the dense-half activations the dedicated FF causal conv kernel reads for `cols` input channels"""
    return _lib.load().ns2_conv3_input_ld(cols)


def linear_split(w: PackedWeight, a: Planes, bias=None, conv_taps=0, dilation=1, seq_len=0, precision=3, ldo=None, pad_left=-1,
                 act=0, out_precision=None, row_lens=None) -> Planes:
    """out_precision: write the output planes in the operand format of another precision, e.g. FMT_H8 lines (4) from a precision-2
    product -- what the hybrid plan's FF causal conv does -- or bf16 hi / lo lines (3) for the attention of the mixed training arithmetic"""
    M = a.rows
    ldo = ldo or round_up(w.rows, 32)
    out = _out_planes(M, ldo, a.device, out_precision or precision)
    _linear(w, a, M, precision, row_lens=row_lens, conv_taps=conv_taps, dilation=dilation, seq_len=seq_len, pad_left=pad_left, bias=_p(bias), act=act,
            out_hi=out.hi, out_lo=out.lo, ldo=ldo, out_precision=out_precision or 0)
    return out


def geglu_pack_bias(bias: torch.Tensor, f: int) -> torch.Tensor:
    n = round_up(2 * round_up(f, 32), 256)
    out = torch.empty(n, dtype=torch.float32, device=bias.device)
    check(_lib.load().ns2_geglu_pack_bias(_f32(bias).data_ptr(), f, out.data_ptr(), n, _stream()), "ns2_geglu_pack_bias")
    return out


def linear_geglu(w: PackedWeight, a: Planes, packed_bias: torch.Tensor, precision=3) -> Planes:
    M = a.rows
    ldo = round_up(w.rows // 2, 32)
    out = _out_planes(M, ldo, a.device, precision)
    _linear(w, a, M, precision, bias=packed_bias.data_ptr(), out_hi=out.hi, out_lo=out.lo, ldo=ldo)
    return out


def linear_qkv(w: PackedWeight, a: Planes, seq_len: int, split_col: int, precision=3):
    """returns (row-major planes [M, split_col], transposed planes [B * (rows - split_col), vt_ld])."""
    M = a.rows
    B = M // seq_len
    vt_ld = round_up(seq_len, 32)
    out = _out_planes(M, split_col, a.device, precision, attention_operand=True)
    vt = _out_planes(B * (w.rows - split_col), vt_ld, a.device, precision, attention_operand=True, zero=True)
    _linear(w, a, M, precision, seq_len=seq_len, split_col=split_col, out_hi=out.hi, out_lo=out.lo, ldo=split_col,
            vt_hi=vt.hi, vt_lo=vt.lo, vt_ld=vt_ld)
    return out, vt


def wavenet_block(w: PackedWeight, a: Planes, seq_len: int, dilation: int, conv_bias, res_bias, film: torch.Tensor,
                  precision=3) -> Planes:
    M = a.rows
    ldo = round_up(w.rows, 32)
    out = _out_planes(M, ldo, a.device, 4 if precision == 5 else precision)      # 5: precision-4 planes, dilated conv as one half product
    check(_lib.load().ns2_wavenet_block(w.handle, a.hi, a.lo, a.ld, M, seq_len, dilation, conv_bias.data_ptr(),
                                        res_bias.data_ptr(), _f32(film).data_ptr(), film.shape[1], out.hi,
                                        out.lo, ldo, precision, _stream()), "ns2_wavenet_block")
    return out


def _attention_fwd(q: Planes, q_col0, k: Planes, k_col0, vt_hi, vt_lo, vt_ld, B, H, Nq, Nk, scale, precision, head_dim=64, o_precision=0,
                   key_mask=None, want_lse=False, drop=None, key_lens=None, train_lens=None):
    """The one place that fills a ns2_attn_args (include/ns2hip.h) and calls ns2_attention_fwd -> (o, lse or None).  vt_hi / vt_lo:
    device addresses of the transposed value planes; o_precision: the format of o when it is not the operands' (0 = `precision`);
    key_mask: uint8 [B, Nk] on the device; drop = (p, seed tensor on the device, call index) or None; key_lens: int32 [B] on the
    device, the call then goes through ns2_attention_fwd_lens (include/ns2hip.h); train_lens: int32 [B] on the device, the
    utterances' lengths of a ragged TRAINING batch (with want_lse): ns2_attention_train_fwd_lens (include/ns2hip_train.h).
    want_lse at a head_dim other than 64 -- the training forward at head dims 32 / 128 -- goes through ns2_attention_train_fwd_hd
    (include/ns2hip_train.h), with or without train_lens."""
    o = _out_planes(B * Nq, H * head_dim, q.device, o_precision or precision)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device) if want_lse else None
    p, seed, call = drop if drop is not None else (0.0, None, 0)
    a = _lib.AttnArgs(q_hi=q.hi, q_lo=q.lo, ldq=q.ld, q_col0=q_col0, k_hi=k.hi, k_lo=k.lo, ldk=k.ld, k_col0=k_col0,
                      vt_hi=vt_hi, vt_lo=vt_lo, vt_ld=vt_ld, o_hi=o.hi, o_lo=o.lo, ldo=o.ld, B=B, H=H, Nq=Nq, Nk=Nk, scale=scale,
                      head_dim=head_dim, precision=precision, o_precision=o_precision, key_mask=_p(key_mask), lse=_p(lse),
                      dropout_p=p, dropout_seed=_p(seed), dropout_call=call)
    if want_lse and head_dim != 64:
        check(_lib.load().ns2_attention_train_fwd_hd(ctypes.byref(a), _p(train_lens), _stream()), "ns2_attention_train_fwd_hd")
    elif train_lens is not None:
        check(_lib.load().ns2_attention_train_fwd_lens(ctypes.byref(a), train_lens.data_ptr(), _stream()), "ns2_attention_train_fwd_lens")
    elif key_lens is not None:
        check(_lib.load().ns2_attention_fwd_lens(ctypes.byref(a), key_lens.data_ptr(), _stream()), "ns2_attention_fwd_lens")
    else:
        check(_lib.load().ns2_attention_fwd(a, _stream()), "ns2_attention_fwd")
    return o, lse


def attention(q: Planes, k: Planes, vt: Planes, B: int, H: int, Nq: int, Nk: int, q_col0=0, k_col0=0, scale=None,
              precision=3, key_mask: Optional[torch.Tensor] = None, head_dim: int = 64, key_lens: Optional[torch.Tensor] = None) -> Planes:
    """vt: transposed value planes [B * H*head_dim, vt_ld]; key_mask: optional bool/uint8 [B, Nk], True = attend (ATT:92-94);
    head_dim 32 / 64 / 128, scale defaults to head_dim ** -0.5 (ATT:128).  key_lens (not in the reference): optional integer [B]
    on the device, utterance b attends to keys [0, key_lens[b]) -- read by the kernel alone, clamped into [1, Nk]; Nk stays the
    stride, and what lies at or beyond a length may hold anything.  Not together with key_mask."""
    if scale is None:
        scale = head_dim ** -0.5
    km = None
    if key_mask is not None:
        km = key_mask.to(torch.uint8).contiguous()
        assert km.shape == (B, Nk)
    kl = None
    if key_lens is not None:
        kl = key_lens.to(device=q.device, dtype=torch.int32).contiguous()
        assert kl.shape == (B,)
    return _attention_fwd(q, q_col0, k, k_col0, vt.hi, vt.lo, vt.ld, B, H, Nq, Nk, scale, precision, head_dim=head_dim, key_mask=km,
                          key_lens=kl)[0]


def rmsnorm(x: torch.Tensor, seq_len: int = 0, gamma=None, cond=None, want_f32=False, precision: int = 3):
    x = _f32(x)
    M, d = x.shape
    ldo = round_up(d, 32)
    out = _out_planes(M, ldo, x.device, precision)
    of = torch.empty(M, d, dtype=torch.float32, device=x.device) if want_f32 else None
    check(_lib.load().ns2_rmsnorm(x.data_ptr(), d, M, d, seq_len, _p(gamma), _p(cond), cond.shape[1] if cond is not None else 0,
                                  out.hi, out.lo, ldo, _p(of), d, precision, _stream()), "ns2_rmsnorm")
    return (out, of) if want_f32 else out


def embedding(ids: torch.Tensor, table: torch.Tensor, pad_id: int) -> torch.Tensor:
    """ids [..] int64 (negative = padding -> pad_id), table [V, dim] -> [.., dim] fp32."""
    ids = ids.contiguous().to(torch.int64)
    out = torch.empty(*ids.shape, table.shape[1], dtype=torch.float32, device=table.device)
    check(_lib.load().ns2_embedding(ids.data_ptr(), _f32(table).data_ptr(), out.data_ptr(), ids.numel(), table.shape[1], pad_id,
                                    _stream()), "ns2_embedding")
    return out


def groupnorm_silu(x: torch.Tensor, B: int, weight: torch.Tensor, bias: torch.Tensor, groups: int = 8, eps: float = 1e-5,
                   resid: Optional[torch.Tensor] = None, want_f32: bool = True, precision: Optional[int] = None,
                   lens: Optional[torch.Tensor] = None):
    """GroupNorm(groups, C) + SiLU (+ resid after the SiLU) over token-major fp32 rows x [B * n, C] (ns2_groupnorm_silu).
    Returns the fp32 rows, the operand planes of `precision` (when given), or (rows, planes).  lens (not in the reference): optional
    integer [B] on the device, rows per utterance (ns2_groupnorm_silu_lens, include/ns2hip_frontend.h) -- the statistics of
    utterance b run over its rows [0, lens[b]) and are bit-equal to the utterance alone; rows from lens[b] on come out as zeros."""
    x = _f32(x)
    M, C = x.shape
    n = M // B
    assert n * B == M, "rows must be B utterances of equal length"
    lib = _lib.load()
    ws = torch.empty(max(lib.ns2_groupnorm_workspace_bytes(B, n, C, groups), 16), dtype=torch.uint8, device=x.device)
    of = torch.empty(M, C, dtype=torch.float32, device=x.device) if want_f32 else None
    pl = _out_planes(M, C, x.device, precision) if precision is not None else None
    if lens is not None:
        rl = _front_lens(lens, B, x.device)          # held until the launch
        check(lib.ns2_groupnorm_silu_lens(x.data_ptr(), B, n, C, groups, _f32(weight).data_ptr(), _f32(bias).data_ptr(), float(eps),
                                          _p(None if resid is None else _f32(resid)), rl.data_ptr(), _p(of), pl.hi if pl else None,
                                          pl.lo if pl else None, C, pl.precision if pl else 3, ws.data_ptr(), ws.numel(), _stream()),
              "ns2_groupnorm_silu_lens")
    else:
        check(lib.ns2_groupnorm_silu(x.data_ptr(), B, n, C, groups, _f32(weight).data_ptr(), _f32(bias).data_ptr(), float(eps),
                                     _p(None if resid is None else _f32(resid)), _p(of), pl.hi if pl else None, pl.lo if pl else None,
                                     C, pl.precision if pl else 3, ws.data_ptr(), ws.numel(), _stream()), "ns2_groupnorm_silu")
    if of is not None and pl is not None:
        return of, pl
    return of if of is not None else pl


def _front_lens(lens, B: int, device) -> torch.Tensor:
    """lengths as the kernels of include/ns2hip_frontend.h read them: int32 [B], contiguous, on `device` (no host read; a tensor
    that already is one comes back as it is)"""
    l = torch.as_tensor(lens).to(device=device, dtype=torch.int32).contiguous()
    assert l.shape == (B,), f"lengths must hold one count per utterance: [{B}]"
    return l


def zero_rows(t, B: int, n: int, lens: torch.Tensor):
    """Zero rows [lens[b], n) of every utterance of `t` IN PLACE and return it (ns2_zero_rows_lens): `t` is operand Planes of
    B * n rows, or a contiguous tensor whose B * n rows are whole 16-byte vectors (fp32 [B * n, C] with C % 4 == 0, [B, n, C]
    likewise).  All-zero bits are 0.0 in fp32 and in every plane format.  lens: integer [B] on the device, clamped into [1, n]."""
    buf = t.buf if isinstance(t, Planes) else t
    assert buf.is_cuda and buf.is_contiguous() and buf.numel() % (B * n) == 0, "expected B * n contiguous rows on the device"
    row_bytes = buf.numel() // (B * n) * buf.element_size()
    rl = _front_lens(lens, B, buf.device)            # held until the launch
    check(_lib.load().ns2_zero_rows_lens(buf.data_ptr(), row_bytes, B, n, rl.data_ptr(), _stream()), "ns2_zero_rows_lens")
    return t


# f0_to_coarse's fp32 constants, evaluated as the reference does (NS2:164-166)
F0_MEL_MIN = float(1127 * torch.log(1 + torch.tensor(50.0) / 700))
F0_MEL_MAX = float(1127 * torch.log(1 + torch.tensor(1100.0) / 700))


def length_regulate(duration: torch.Tensor, pitch: torch.Tensor, enc: torch.Tensor, pitch_table: torch.Tensor, return_totals: bool = False):
    """duration / pitch [B, n_ph], enc [B, n_ph, D], pitch_table [>= 256, D] -> the frame-aligned conditioning [B, D, n_frames]
    of NaturalSpeech2.sample (ns2_length_regulate).  n_frames = the longest utterance's sum of int(duration): one host read,
    as the reference's `.item()` (NS2:92).  return_totals: (that, the utterances' own frame totals, int32 [B] on the device)."""
    duration, pitch, enc, table = _f32(duration), _f32(pitch), _f32(enc), _f32(pitch_table)
    B, n_ph = duration.shape
    D = enc.shape[-1]
    assert pitch.shape == (B, n_ph) and enc.shape == (B, n_ph, D) and table.shape[1] == D and table.shape[0] >= 256
    lib = _lib.load()
    totals = torch.empty(B, dtype=torch.int32, device=duration.device)
    check(lib.ns2_length_regulate_totals(duration.data_ptr(), B, n_ph, totals.data_ptr(), _stream()), "ns2_length_regulate_totals")
    n_frames = int(totals.max().item())
    out = torch.empty(B, D, n_frames, dtype=torch.float32, device=duration.device)
    if n_frames > 0:
        check(lib.ns2_length_regulate(duration.data_ptr(), pitch.data_ptr(), enc.data_ptr(), table.data_ptr(), B, n_ph, D, n_frames,
                                      F0_MEL_MIN, F0_MEL_MAX, out.data_ptr(), _stream()), "ns2_length_regulate")
    return (out, totals) if return_totals else out


def row_dot(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """x [M, K] . w [K] (+ bias[0]) (ReLU) -> [M] (ns2_row_dot): a Linear(K, 1) head"""
    x, w = _f32(x), _f32(w.reshape(-1))
    M, K = x.shape
    out = torch.empty(M, dtype=torch.float32, device=x.device)
    check(_lib.load().ns2_row_dot(x.data_ptr(), K, M, K, w.data_ptr(), _p(None if bias is None else _f32(bias)), int(relu),
                                  out.data_ptr(), _stream()), "ns2_row_dot")
    return out


def _skinny_ws(B, K, J, device):
    n = _lib.load().ns2_skinny_linear_workspace_bytes(B, K, J)
    return torch.empty(max(n, 16), dtype=torch.uint8, device=device), n


def skinny_linear(x: torch.Tensor, wt: torch.Tensor, bias=None, act=0, use_workspace=True) -> torch.Tensor:
    """x [B, K] @ wt [K, J] (+bias) ; act 1 = SiLU.  The split-K scratch is caller-owned (here: a torch tensor)."""
    x, wt = _f32(x), _f32(wt)
    B, K = x.shape
    J = wt.shape[1]
    out = torch.empty(B, J, dtype=torch.float32, device=x.device)
    ws, n = _skinny_ws(B, K, J, x.device) if use_workspace else (None, 0)
    check(_lib.load().ns2_skinny_linear(x.data_ptr(), K, wt.data_ptr(), _p(bias), out.data_ptr(), J, B, K, J, act, _p(ws), n,
                                        _stream()), "ns2_skinny_linear")
    return out


def time_embed(times: torch.Tensor, freqs: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    B = times.shape[0]
    dim = freqs.shape[0] * 2
    dt = wt.shape[1]
    feat = torch.empty(B, dim + 1, dtype=torch.float32, device=times.device)
    out = torch.empty(B, dt, dtype=torch.float32, device=times.device)
    ws, n = _skinny_ws(B, dim + 1, dt, times.device)
    check(_lib.load().ns2_time_embed(_f32(times).data_ptr(), _f32(freqs).data_ptr(), _f32(wt).data_ptr(), _f32(bias).data_ptr(),
                                     feat.data_ptr(), out.data_ptr(), dt, B, dim, dt, ws.data_ptr(), n, _stream()), "ns2_time_embed")
    return out


def saturation_count(reset: bool = True, device=None) -> int:
    """conversions to IEEE half (precisions "half" / "mixed") that met a value outside the half range since the last reset, on
    `device` (default: the current one).  Synchronises; see include/ns2hip.h."""
    import ctypes
    n = ctypes.c_int64(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(_lib.load().ns2_saturation_count(int(reset), ctypes.byref(n)), "ns2_saturation_count")
    return n.value


OBJECTIVES = {"v": 0, "eps": 1, "x0": 2}
SCHEDULES = {"sigmoid": 0, "cosine": 1, "linear": 2}


def ddim_step(audio, model_out, times, times_next, objective="v", schedule="sigmoid", scale=1.0, out=None):
    audio, model_out = _f32(audio), _f32(model_out)
    B = audio.shape[0]
    per = audio.numel() // B
    out = torch.empty_like(audio) if out is None else out
    check(_lib.load().ns2_ddim_step(audio.data_ptr(), model_out.data_ptr(), out.data_ptr(), _f32(times).data_ptr(),
                                    _f32(times_next).data_ptr(), B, per, OBJECTIVES[objective], SCHEDULES[schedule], float(scale),
                                    _stream()), "ns2_ddim_step")
    return out


def cfg_mix(cond_out, null_out, cond_scale: float, out=None):
    out = torch.empty_like(cond_out) if out is None else out
    check(_lib.load().ns2_cfg_mix(_f32(cond_out).data_ptr(), _f32(null_out).data_ptr(), out.data_ptr(), cond_out.numel(),
                                  float(cond_scale), _stream()), "ns2_cfg_mix")
    return out


def rvq_prepare(codebooks: torch.Tensor) -> torch.Tensor:
    cb = _f32(codebooks)
    Q, C, D = cb.shape
    out = torch.empty(Q, C, dtype=torch.float32, device=cb.device)
    check(_lib.load().ns2_rvq_prepare(cb.data_ptr(), out.data_ptr(), Q, C, D, _stream()), "ns2_rvq_prepare")
    return out


def rvq_encode(x: torch.Tensor, codebooks: torch.Tensor, cb_norm: Optional[torch.Tensor] = None, tie_eps: float = 1e-4,
               want_residual=False, count_ties=False, want_emb=True):
    """x [M, 128] fp32, codebooks [Q, C, 128] -> codes [M, Q] int64, emb [M, 128] (, residual, n_near_ties).
    want_emb=False skips the decode launch that sums the selected code vectors (emb is returned as None)."""
    x, cb = _f32(x), _f32(codebooks)
    M, D = x.shape
    Q, C, _ = cb.shape
    cb_norm = rvq_prepare(cb) if cb_norm is None else cb_norm
    codes = torch.empty(M, Q, dtype=torch.int64, device=x.device)
    emb = torch.empty(M, D, dtype=torch.float32, device=x.device) if want_emb else None
    resid = torch.empty(M, D, dtype=torch.float32, device=x.device) if want_residual else None
    ties = torch.zeros(1, dtype=torch.int32, device=x.device) if count_ties else None
    check(_lib.load().ns2_rvq_encode(x.data_ptr(), cb.data_ptr(), cb_norm.data_ptr(), codes.data_ptr(), _p(emb), _p(resid),
                                     _p(ties), M, Q, C, D, float(tie_eps), _stream()), "ns2_rvq_encode")
    res = [codes, emb]
    if want_residual:
        res.append(resid)
    if count_ties:
        res.append(ties)
    return tuple(res)


def rvq_decode(codes: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    cb = _f32(codebooks)
    Q, C, D = cb.shape
    M = codes.shape[0]
    emb = torch.empty(M, D, dtype=torch.float32, device=cb.device)
    check(_lib.load().ns2_rvq_decode(codes.contiguous().data_ptr(), cb.data_ptr(), emb.data_ptr(), M, Q, C, D, _stream()),
          "ns2_rvq_decode")
    return emb


def rvq_cross_entropy(x: torch.Tensor, codebooks: torch.Tensor, cb_norm: Optional[torch.Tensor], indices: torch.Tensor, need_grad: bool,
                       need_quantized: bool = True, lens: Optional[torch.Tensor] = None):
    """the RVQ cross-entropy of the training loss in one launch (ns2_rvq_ce, csrc/rvq_ce.hip): x [M, 128] fp32, codebooks [Q, C, 128],
    indices [M, Q] int64 -> (loss 0-dim, row_loss [M, Q], quantized_out [M, 128] or None, G [M, 128] = d loss / d x or None).
    An index outside [0, C) gives a NaN loss; nothing is read back to the host.
    lens [B] (a CUDA integer tensor; M = B n): the ragged batch of ns2_rvq_ce_lens (include/ns2hip_train.h) -- the loss is the mean
    over utterances of each one's own mean, and every output row at or behind a length is 0 whatever x and indices hold there."""
    x, cb = _f32(x), _f32(codebooks)
    M, D = x.shape
    Q, C, _ = cb.shape
    assert indices.dtype == torch.int64 and tuple(indices.shape) == (M, Q), "indices must be int64 [M, Q]"
    idx = indices if indices.is_contiguous() else indices.contiguous()
    cb_norm = rvq_prepare(cb) if cb_norm is None else cb_norm
    lib = _lib.load()
    row_loss = torch.empty(M, Q, dtype=torch.float32, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    quant = torch.empty(M, D, dtype=torch.float32, device=x.device) if need_quantized else None
    grad = torch.empty(M, D, dtype=torch.float32, device=x.device) if need_grad else None
    nbytes = lib.ns2_rvq_ce_workspace_bytes(M, Q, int(need_quantized))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    if lens is not None:
        ln = _lens(lens)              # held until the launch
        B = ln.shape[0]
        assert B > 0 and M % B == 0, f"lens [{B}] must divide the {M} rows into utterances of equal padded length"
        check(lib.ns2_rvq_ce_lens(x.data_ptr(), cb.data_ptr(), cb_norm.data_ptr(), idx.data_ptr(), row_loss.data_ptr(), loss.data_ptr(),
                                  _p(quant), _p(grad), B, M // B, ln.data_ptr(), Q, C, D, _p(ws), nbytes, _stream()), "ns2_rvq_ce_lens")
        return loss[0], row_loss, quant, grad
    check(lib.ns2_rvq_ce(x.data_ptr(), cb.data_ptr(), cb_norm.data_ptr(), idx.data_ptr(), row_loss.data_ptr(), loss.data_ptr(), _p(quant),
                         _p(grad), M, Q, C, D, _p(ws), nbytes, _stream()), "ns2_rvq_ce")
    return loss[0], row_loss, quant, grad


# ---- Aligner and the text-conditioned training pass (csrc/aligner.hip).  Lengths are int32 [B] device tensors.
def _lens(t: torch.Tensor) -> torch.Tensor:
    assert t.is_cuda and t.dim() == 1, "lengths are [B] CUDA tensors"
    return t.to(torch.int32).contiguous()


def relu_split(x: torch.Tensor, ldo: Optional[int] = None, precision: int = 3) -> Planes:
    """fp32 [M, N] -> operand planes of ReLU(x) [M, ldo], padding columns zero (ns2_relu_split)"""
    x = _f32(x)
    M, N = x.shape
    out = _out_planes(M, ldo or round_up(N, 32), x.device, precision)
    check(_lib.load().ns2_relu_split(x.data_ptr(), M, N, out.hi, out.lo, out.ld, out.precision, _stream()), "ns2_relu_split")
    return out


def align_attn(queries: torch.Tensor, keys: torch.Tensor, text_lens: torch.Tensor, B: int):
    """queries [B * T, C], keys [B * n, C] -> (aln_log [B, 1, T, n], aln_soft [B, n, T]) (ns2_align_attn)"""
    q, k = _f32(queries), _f32(keys)
    C = q.shape[1]
    T, n = q.shape[0] // B, k.shape[0] // B
    tl = _lens(text_lens)             # held until the launch: a freed temporary could be reused by the next allocation
    log = torch.empty(B, 1, T, n, dtype=torch.float32, device=q.device)
    soft = torch.empty(B, n, T, dtype=torch.float32, device=q.device)
    check(_lib.load().ns2_align_attn(q.data_ptr(), k.data_ptr(), tl.data_ptr(), B, T, n, C, log.data_ptr(),
                                     soft.data_ptr(), _stream()), "ns2_align_attn")
    return log, soft


def maximum_path(value: torch.Tensor, text_lens: torch.Tensor, mel_lens: torch.Tensor):
    """value [B, t_x, t_y] fp32 -> (path [B, t_x, t_y] 0/1 fp32, durations [B, t_x] int32) (ns2_maximum_path)"""
    value = _f32(value)
    B, t_x, t_y = value.shape
    lib = _lib.load()
    n = lib.ns2_maximum_path_workspace_bytes(B, t_x, t_y)
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=value.device)
    path = torch.empty_like(value)
    dur = torch.empty(B, t_x, dtype=torch.int32, device=value.device)
    tl, ml = _lens(text_lens), _lens(mel_lens)       # held until the launch
    check(lib.ns2_maximum_path(value.data_ptr(), tl.data_ptr(), ml.data_ptr(), B, t_x, t_y, path.data_ptr(),
                               dur.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ns2_maximum_path")
    return path, dur


def average_over_durations(pitch: torch.Tensor, durations: torch.Tensor) -> torch.Tensor:
    """pitch [B, T] fp32, durations [B, n] int -> [B, n] (ns2_average_over_durations)"""
    pitch = _f32(pitch)
    d = durations.to(torch.int32).contiguous()
    B, T = pitch.shape
    out = torch.empty(B, d.shape[1], dtype=torch.float32, device=pitch.device)
    check(_lib.load().ns2_average_over_durations(pitch.data_ptr(), d.data_ptr(), B, T, d.shape[1], out.data_ptr(), _stream()),
          "ns2_average_over_durations")
    return out


def expand_frames(duration: torch.Tensor, pitch: torch.Tensor, enc: torch.Tensor, pitch_table: torch.Tensor, n_frames: int) -> torch.Tensor:
    """the length regulator into exactly n_frames frames (ns2_length_regulate, no host read): [B, D, n_frames]"""
    duration, pitch, enc, table = _f32(duration), _f32(pitch), _f32(enc), _f32(pitch_table)
    B, n_ph = duration.shape
    D = enc.shape[-1]
    assert pitch.shape == (B, n_ph) and enc.shape == (B, n_ph, D) and table.shape[1] == D and table.shape[0] >= 256
    out = torch.empty(B, D, n_frames, dtype=torch.float32, device=duration.device)
    check(_lib.load().ns2_length_regulate(duration.data_ptr(), pitch.data_ptr(), enc.data_ptr(), table.data_ptr(), B, n_ph, D, n_frames,
                                          F0_MEL_MIN, F0_MEL_MAX, out.data_ptr(), _stream()), "ns2_length_regulate")
    return out


def expand_backward(d_cond: torch.Tensor, duration: torch.Tensor, pitch: torch.Tensor, n_bins: Optional[int]):
    """gradients of expand_frames: (d_enc [B, n, D], d_table [n_bins, D] or None) (ns2_expand_backward)"""
    d_cond, duration, pitch = _f32(d_cond), _f32(duration), _f32(pitch)
    B, D, n_frames = d_cond.shape
    n = duration.shape[1]
    lib = _lib.load()
    ws = torch.empty(max(lib.ns2_expand_backward_workspace_bytes(B, n), 16), dtype=torch.uint8, device=d_cond.device)
    d_enc = torch.empty(B, n, D, dtype=torch.float32, device=d_cond.device)
    d_table = torch.empty(n_bins, D, dtype=torch.float32, device=d_cond.device) if n_bins else None
    check(lib.ns2_expand_backward(d_cond.data_ptr(), duration.data_ptr(), pitch.data_ptr(), B, n, D, n_frames, n_bins or 0, F0_MEL_MIN,
                                  F0_MEL_MAX, d_enc.data_ptr(), _p(d_table), ws.data_ptr(), ws.numel(), _stream()), "ns2_expand_backward")
    return d_enc, d_table


# ---- AudioToMel (csrc/audio_to_mel.hip)
def audio_to_mel(audio: torch.Tensor, n_fft: int, hop_length: int, n_mels: int, log: bool, plan: dict,
                 lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio [B, L] fp32 -> [B, n_mels, 1 + L // hop_length] (ns2_audio_to_mel); `plan`: the device tables of
    audio_to_mel._plan (window, twiddle, meta, weights) and their sizes n_w, n_bins.
    lens [B] (a CUDA integer tensor of sample counts): ns2_audio_to_mel_lens (include/ns2hip_audio.h)"""
    audio = _f32(audio)
    B, L = audio.shape
    T = 1 + L // hop_length
    out = torch.empty(B, n_mels, T, dtype=torch.float32, device=audio.device)
    lib = _lib.load()
    ln = None if lens is None else _lens(lens)     # held until the launch
    assert ln is None or ln.shape[0] == B, f"lens must hold one sample count per utterance: [{B}]"
    for b0 in range(0, B, 65535):                 # grid.y holds at most 65535 utterances
        nb = min(65535, B - b0)
        if lens is not None:
            check(lib.ns2_audio_to_mel_lens(audio[b0].data_ptr(), nb, L, n_fft, hop_length, plan["window"].data_ptr(),
                                            plan["twiddle"].data_ptr(), plan["meta"].data_ptr(), plan["weights"].data_ptr(), plan["n_w"],
                                            n_mels, plan["n_bins"], int(bool(log)), out[b0].data_ptr(), ln[b0:].data_ptr(), _stream()),
                  "ns2_audio_to_mel_lens")
            continue
        check(lib.ns2_audio_to_mel(audio[b0].data_ptr(), nb, L, n_fft, hop_length, plan["window"].data_ptr(),
                                   plan["twiddle"].data_ptr(), plan["meta"].data_ptr(), plan["weights"].data_ptr(), plan["n_w"],
                                   n_mels, plan["n_bins"], int(bool(log)), out[b0].data_ptr(), _stream()), "ns2_audio_to_mel")
    return out


# ---- PitchExtractor (csrc/pitch.hip)
def pitch_yin(audio: torch.Tensor, sample_rate: int, hop_length: int, tau_min: int, tau_max: int, threshold: float,
              lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio [B, L] fp32 -> f0 [B, 1 + L // hop_length] in Hz, 0 where unvoiced (ns2_pitch_yin, include/ns2hip_audio.h).
    lens [B] (a CUDA integer tensor of sample counts): ns2_pitch_yin_lens (include/ns2hip_audio.h)"""
    audio = _f32(audio)
    B, L = audio.shape
    out = torch.empty(B, 1 + L // hop_length, dtype=torch.float32, device=audio.device)
    lib = _lib.load()
    ln = None if lens is None else _lens(lens)     # held until the launch
    assert ln is None or ln.shape[0] == B, f"lens must hold one sample count per utterance: [{B}]"
    for b0 in range(0, B, 65535):                 # grid.y holds at most 65535 utterances
        nb = min(65535, B - b0)
        if lens is not None:
            check(lib.ns2_pitch_yin_lens(audio[b0].data_ptr(), nb, L, sample_rate, hop_length, tau_min, tau_max, threshold,
                                         out[b0].data_ptr(), ln[b0:].data_ptr(), _stream()), "ns2_pitch_yin_lens")
            continue
        check(lib.ns2_pitch_yin(audio[b0].data_ptr(), nb, L, sample_rate, hop_length, tau_min, tau_max, threshold, out[b0].data_ptr(),
                                _stream()), "ns2_pitch_yin")
    return out


# ---- Resample (csrc/resample.hip)
def resample(audio: torch.Tensor, up: int, down: int, width: int, taps: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio [B, L] fp32 -> [B, ceil(up L / down)] (ns2_resample, include/ns2hip_audio.h); taps: the transposed table [T, up] fp32 on
    the device, T = 2 width + down.  lens [B] (a CUDA integer tensor of sample counts): ns2_resample_lens.  A shape the kernel does
    not take raises (rc NS2_UNAVAILABLE): callers ask ns2_resample_frames_per_block first."""
    audio, taps = _f32(audio), _f32(taps)
    B, L = audio.shape
    assert taps.shape == (2 * width + down, up), f"taps must be the transposed table [{2 * width + down}, {up}]"
    L_out = (L * up + down - 1) // down
    out = torch.empty(B, L_out, dtype=torch.float32, device=audio.device)
    lib = _lib.load()
    ln = None if lens is None else _lens(lens)     # held until the launch
    assert ln is None or ln.shape[0] == B, f"lens must hold one sample count per utterance: [{B}]"
    for b0 in range(0, B, 65535):                 # grid.y holds at most 65535 utterances
        nb = min(65535, B - b0)
        if lens is not None:
            check(lib.ns2_resample_lens(audio[b0].data_ptr(), nb, L, up, down, width, taps.data_ptr(), out[b0].data_ptr(), L_out,
                                        ln[b0:].data_ptr(), _stream()), "ns2_resample_lens")
            continue
        check(lib.ns2_resample(audio[b0].data_ptr(), nb, L, up, down, width, taps.data_ptr(), out[b0].data_ptr(), L_out, _stream()),
              "ns2_resample")
    return out
