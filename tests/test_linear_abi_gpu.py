"""ns2_linear (include/ns2hip.h) called with hand-filled argument blocks on real weights: every refusal of capi.cpp linear_args_from that
needs a packed weight, and that a block with only the required fields set is the plain call of each kind -- bit-equal to the ops wrapper."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")


def test_linear_blocks_on_real_weights_refusals_and_the_zeroed_block_is_the_plain_call():
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: (torch.randn(*shape, generator=g) / 8).to(DEV)                      # noqa: E731
    M, K, seq_len = 64, 64, 32
    lin, conv = ops.PackedWeight(rnd(64, K)), ops.PackedWeight(rnd(64, K, 3))
    geglu, gbias = ops.PackedWeight(rnd(128, K), geglu=True), ops.geglu_pack_bias(rnd(128), 64)
    a = ops.split(rnd(M, K))
    stream = torch.cuda.current_stream().cuda_stream
    f32 = torch.empty(M, 64, device=DEV)
    pl, vt = ops.empty_planes(M, 64, DEV), ops.empty_planes(2 * 32, 32, DEV, zero=True)

    def block(w, **kw):
        return _lib.LinearArgs(w=w.handle, a_hi=a.hi, a_lo=a.lo, lda=a.ld, M=M, precision=3, **kw)

    to_f32, to_planes = dict(out_f32=f32.data_ptr(), ldo_f=64), dict(out_hi=pl.hi, out_lo=pl.lo, ldo=64)
    to_qkv = dict(out_hi=pl.hi, out_lo=pl.lo, ldo=32, seq_len=seq_len, split_col=32, vt_hi=vt.hi, vt_lo=vt.lo, vt_ld=32)

    def refused(args, word):
        """a non-zero code before any launch, and the message is this refusal's own (the last error is sticky)"""
        rc = lib.ns2_linear(args, stream)
        msg = (lib.ns2_last_error() or b"").decode()
        return rc != 0 and msg.startswith("ns2_linear:") and word in msg

    def but(d, **kw):
        return dict(d, **kw)

    # ---- what every old entry point refused
    b2 = block(lin, **to_f32)
    b2.precision = 2
    assert refused(b2, "packed for a different precision")
    assert refused(block(conv, **to_f32), "does not match conv_taps")                       # a k = 3 weight called as a Linear
    assert refused(block(lin, conv_taps=3, pad_left=-1, seq_len=seq_len, **to_f32), "does not match conv_taps")
    short = block(lin, **to_f32)
    short.lda = 32
    assert refused(short, "lda smaller than the padded K")
    assert refused(block(lin, **but(to_planes, ldo=63)), "ldo must be even")
    assert refused(block(conv, conv_taps=3, pad_left=3, seq_len=seq_len, **to_f32), "pad_left must be")
    assert refused(block(lin, act=3, **to_f32), "act must be")
    assert refused(block(lin, out_precision=2, **to_planes), "out_lo must be null")
    assert refused(block(geglu, bias=gbias.data_ptr(), **but(to_planes, ldo=32)), "ldo must be round_up(f, 32)")
    assert refused(block(lin, **but(to_qkv, split_col=48)), "q | k | v shapes")
    assert refused(block(lin, **but(to_qkv, split_col=64, ldo=64)), "split_col must lie below")
    # ---- destinations no kernel covers (tests/test_gemm_dest_gpu.py): q | k rows that overlap, interleaved V^T lines that overlap, plane
    # columns beyond the last column tile of the 128 x 128 kernel and the split-K finish (also on ns2_wavenet_block)
    assert refused(block(lin, **but(to_qkv, ldo=0)), "ldo smaller than split_col")
    assert refused(block(lin, **but(to_qkv, vt_ld=40)), "vt_ld must be a multiple of 32 with vt_lo")
    assert refused(block(lin, **but(to_planes, ldo=160)), "ldo larger than the rows of w rounded up to 128")
    wide = ops.empty_planes(M, 160, DEV, zero=True)
    assert refused(block(lin, out_hi=wide.hi, out_lo=wide.lo, ldo=160), "ldo larger than")
    wn = ops.PackedWeight(rnd(64, K, 3), extra1x1=rnd(64, K, 1))
    cb, film = rnd(64), rnd(M // seq_len, 128)
    rc = lib.ns2_wavenet_block(wn.handle, a.hi, a.lo, a.ld, M, seq_len, 1, cb.data_ptr(), cb.data_ptr(), film.data_ptr(), 128, wide.hi, wide.lo, 160, 3, stream)
    msg = (lib.ns2_last_error() or b"").decode()
    assert rc != 0 and msg.startswith("ns2_wavenet_block:") and "ldo larger than" in msg
    torch.cuda.synchronize()
    assert not bool(wide.buf.view(torch.int16).any())                                      # refused before any launch: nothing was written
    # ---- combinations no old entry point offered
    assert refused(block(lin, bias=gbias.data_ptr(), **to_qkv), "vt_hi (the fused q | k | v) excludes bias")
    assert refused(block(lin, out_precision=3, **to_f32), "out_precision need out_hi")
    assert refused(block(lin, resid=f32.data_ptr(), ldr=64, **to_planes), "resid needs out_f32")
    assert refused(block(geglu, **to_planes), "a geglu weight needs the packed bias")
    assert refused(block(geglu, bias=gbias.data_ptr(), act=1, **to_planes), "a geglu weight needs")
    assert refused(block(geglu, bias=gbias.data_ptr(), **to_f32), "a geglu weight needs")
    # ---- the two kinds of malformed calls the old q | k | v and GEGLU entries let through
    assert refused(block(geglu, **to_qkv), "a geglu weight needs")
    assert refused(block(conv, **to_qkv), "does not match conv_taps")
    for kind in (block(lin, **to_qkv), block(geglu, bias=gbias.data_ptr(), **to_planes)):
        kind.lda = 32
        assert refused(kind, "lda smaller than the padded K")

    # ---- only the required fields set = the plain call of each kind, bit for bit
    def run(args):
        _lib.check(lib.ns2_linear(args, stream), "ns2_linear")

    run(block(lin, **to_f32))
    assert torch.equal(f32, ops.linear_f32(lin, a))
    run(block(lin, **to_planes))
    assert torch.equal(pl.buf, ops.linear_split(lin, a).buf)
    run(block(geglu, bias=gbias.data_ptr(), **to_planes))
    assert torch.equal(pl.buf, ops.linear_geglu(geglu, a, gbias).buf)
    qk = ops.empty_planes(M, 32, DEV)
    run(block(lin, **but(to_qkv, out_hi=qk.hi, out_lo=qk.lo)))
    ref_qk, ref_vt = ops.linear_qkv(lin, a, seq_len, 32)
    assert torch.equal(qk.buf, ref_qk.buf) and torch.equal(vt.buf, ref_vt.buf)
