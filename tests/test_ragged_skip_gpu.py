"""Skipping the hidden row tiles of a ragged sampling batch on the MI355X (include/ns2hip.h).  The reference in every test is
the same entry WITHOUT lengths, or with lengths and the switch off -- never the skipping code itself.  Rows before an utterance's computed
extent H_i = min(N, 256 ceil(lens_i / 256)) must keep their bits; hidden rows must not be touched (sentinels), except an fp32 output
without a residual, which gets exact zeros.

Batch A: 3 x 768 frames, lens [768, 300, 1] -> extents [768, 512, 256]: no, one and two hidden tiles.  Batch B: 3 x 512, lens [1, 257, 512]."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, ops  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")
BATCHES = {"A": (3, 768, [768, 300, 1]), "B": (3, 512, [1, 257, 512])}
SENT16, SENT32 = 0x1234, -7.25


def extent(l, n):
    return min(n, 256 * ((min(max(l, 1), n) + 255) // 256))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _force_gemm(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


ROUTES = dict(splitk=0, tile128=1, tile256=2, ffconv3=3, linear3=4, wavenet3=5)


def _route_counts():
    lib = _lib.load()
    return [int(lib.ns2_debug_gemm_route_launches(r)) for r in range(6)]


def _routes_taken(before):
    """{route index: products} launch_gemm has routed since `before`"""
    return {r: n - b for r, (n, b) in enumerate(zip(_route_counts(), before)) if n != b}


def _sentinel_planes(rows, cols, precision, attention_operand=False):
    lo, fmt = ops._fmt_of(precision, attention_operand)
    p = ops.empty_planes(rows, cols, DEV, lo, fmt=fmt)
    p.buf.view(torch.int16).fill_(SENT16)
    return p


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _check_rows(got, ref, B, N, lens, what, zeros=False):
    """got / ref: 2-D buffers with one row per frame.  Rows before H_b: the reference's bits; rows from H_b on: untouched (or exact zeros)"""
    g, r = got.reshape(B, N, -1), ref.reshape(B, N, -1)
    hidden = 0
    for b, l in enumerate(lens):
        h = extent(l, N)
        assert torch.equal(g[b, :h], r[b, :h]), f"{what}: utterance {b}, rows before {h} differ from the entry without lengths"
        if h < N:
            tail = g[b, h:]
            hidden += tail.numel()
            if zeros:
                assert torch.count_nonzero(tail.view(torch.int32)) == 0, f"{what}: utterance {b}, hidden rows are not exact zeros"
            elif tail.dtype == torch.float32:
                assert bool((tail == SENT32).all()), f"{what}: utterance {b}, hidden fp32 rows were written"
            else:
                assert bool((tail.view(torch.int16) == SENT16).all()), f"{what}: utterance {b}, hidden rows were written"
    assert hidden > 0


# ------------------------------------------------------------------------------------------------ 1. the GEMM routes, stand-alone
def _linear(w, a, M, precision, lens, N, **fields):
    args = _lib.LinearArgs(w=w.handle, a_hi=a.hi, a_lo=a.lo, lda=a.ld, M=M, precision=precision, **fields)
    lib = _lib.load()
    if lens is None:
        _lib.check(lib.ns2_linear(args, _stream()), "ns2_linear")
    else:
        _lib.check(lib.ns2_linear_lens(ctypes.byref(args), lens.data_ptr(), N, _stream()), "ns2_linear_lens")


LINEAR_CASES = [  # (kind, precision, output columns, K, residual)
    ("f32", 4, 256, 96, False), ("f32", 4, 320, 160, True), ("f32", 3, 320, 96, False), ("f32", 3, 256, 160, True),
    ("split", 4, 320, 96, False), ("split", 3, 256, 160, False), ("split", 4, 256, 160, False),
    ("qkv", 4, 384, 96, False), ("qkv", 3, 384, 160, False),
    ("geglu", 4, 320, 96, False), ("geglu", 3, 320, 160, False),
    ("conv3", 2, 320, 96, False), ("conv3_f32", 2, 256, 160, True), ("conv3_f32", 2, 320, 160, False),
]


@pytest.mark.parametrize("mode", [1, 2, 5])
@pytest.mark.parametrize("batch", ["A", "B"])
@pytest.mark.parametrize("kind,precision,ncol,K,resid", LINEAR_CASES)
def test_gemm_routes_skip_hidden_row_tiles(mode, batch, kind, precision, ncol, K, resid):
    B, N, lens_l = BATCHES[batch]
    M, lens = B * N, _lens(lens_l)
    x = _rand((M, K), 11)
    conv = kind.startswith("conv3")
    if conv:
        w = ops.PackedWeight(_rand((ncol, K, 3), 12, 0.1), precision=precision).tile_conv3()
        a = ops.split(x, ldo=ops.conv3_input_ld(K), precision=precision)
    elif kind == "geglu":
        w = ops.PackedWeight(_rand((ncol, K), 12, 0.1), geglu=True, precision=precision)
        a = ops.split(x, precision=precision)
    else:
        w = ops.PackedWeight(_rand((ncol, K), 12, 0.1), precision=precision)
        a = ops.split(x, precision=precision)
    if precision == 4 and not conv:
        w.tile_linear()
    bias = _rand((ncol,), 13)
    res = _rand((M, ncol), 14) if resid else None
    common = dict(conv_taps=3, dilation=1, seq_len=N, pad_left=-1) if conv else {}      # (-1: causal, what the FF conv kernel takes)

    def run(with_lens):
        outs = {}
        if kind in ("f32", "conv3_f32"):
            out = torch.full((M, ncol), SENT32, device=DEV)
            r = None if res is None else res.clone()
            _linear(w, a, M, precision, lens if with_lens else None, N, bias=bias.data_ptr(), out_f32=out.data_ptr(), ldo_f=ncol,
                    resid=ops._p(r), ldr=ncol if r is not None else 0, **common)
            outs["out"] = out
            if r is not None:
                outs["resid"] = r
        elif kind in ("split", "conv3"):
            op = 4 if conv else precision                     # the FF conv of the hybrid plan writes FMT_H8 lines
            out = _sentinel_planes(M, ops.round_up(ncol, 32), op)
            _linear(w, a, M, precision, lens if with_lens else None, N, bias=bias.data_ptr(), out_hi=out.hi, out_lo=out.lo, ldo=out.ld,
                    out_precision=op if conv else 0, **common)
            outs["planes"] = out.buf
        elif kind == "geglu":
            f = ncol // 2
            out = _sentinel_planes(M, ops.round_up(f, 32), precision)
            _linear(w, a, M, precision, lens if with_lens else None, N, bias=ops.geglu_pack_bias(bias[:ncol], f).data_ptr(), out_hi=out.hi,
                    out_lo=out.lo, ldo=out.ld)
            outs["planes"] = out.buf
        else:                                                 # q | k | v with V^T
            split_col = 256
            out = _sentinel_planes(M, split_col, precision, attention_operand=True)
            vt = _sentinel_planes(B * (ncol - split_col), N, precision, attention_operand=True)
            _linear(w, a, M, precision, lens if with_lens else None, N, seq_len=N, split_col=split_col, out_hi=out.hi, out_lo=out.lo,
                    ldo=split_col, vt_hi=vt.hi, vt_lo=vt.lo, vt_ld=N)
            outs["planes"] = out.buf
            outs["vt"] = (vt.buf, vt.has_lo)
        torch.cuda.synchronize()
        return outs

    try:
        _force_gemm(mode)
        before = _route_counts()
        ref, got = run(False), run(True)
        taken = _routes_taken(before)
    finally:
        _force_gemm(0)
    # the kernel under test really ran, with and without lengths: mode 5 = the dedicated kernel of the product (the lean linear kernel for
    # FMT_H8 operands, the FF conv kernel for the half conv; bf16 x3 has none: by shape, 18 tiles of 256 x 256 -> the 128 x 128 kernel)
    want = {1: "tile128", 2: "tile256", 5: "ffconv3" if conv else ("linear3" if precision == 4 else "tile128")}[mode]
    assert taken == {ROUTES[want]: 2}, (taken, want)
    what = f"{kind} p{precision} {ncol}x{K} mode {mode} batch {batch}"
    if "out" in got:
        _check_rows(got["out"], ref["out"], B, N, lens_l, what, zeros=not resid)
    if "resid" in got:
        assert torch.equal(got["resid"], res), "the residual rows are read-only here"
    if "planes" in got:
        _check_rows(got["planes"], ref["planes"], B, N, lens_l, what)
    if "vt" in got:
        (g, has_lo), (r, _) = got["vt"], ref["vt"]
        rows = g.shape[0] // B
        g, r = g.view(B, rows, -1), r.view(B, rows, -1)
        for b, l in enumerate(lens_l):
            h = extent(l, N) * (2 if has_lo else 1)           # interleaved lines: 32 logical columns take 64 physical ones
            assert torch.equal(g[b, :, :h].view(torch.int16), r[b, :, :h].view(torch.int16)), (what, b)
            assert bool((g[b, :, h:].view(torch.int16) == SENT16).all()), f"{what}: V^T columns of hidden frames were written ({b})"


@pytest.mark.parametrize("mode", [1, 2, 5])
@pytest.mark.parametrize("precision", [3, 5])
def test_wavenet_block_skips_hidden_row_tiles(mode, precision):
    """256 channels, dilation 4: under mode 5 precision 5 takes wavenet3_kernel, every other combination the two tile kernels"""
    B, N, lens_l = BATCHES["A"]
    M, C, lens = B * N, 256, _lens(lens_l)
    wp = 4 if precision == 5 else precision
    w = ops.PackedWeight(_rand((C, C, 3), 21, 0.05), extra1x1=_rand((C, C, 1), 22, 0.05), precision=wp)
    if precision == 5:
        w.tile_wavenet()
    a = ops.split(_rand((M, C), 23), precision=wp)
    cb, rb, film = _rand((C,), 24), _rand((C,), 25), _rand((B, 2 * C), 26)
    lib = _lib.load()

    def run(with_lens):
        out = _sentinel_planes(M, C, wp)
        if with_lens:
            _lib.check(lib.ns2_wavenet_block_lens(w.handle, a.hi, a.lo, a.ld, M, N, 4, cb.data_ptr(), rb.data_ptr(), film.data_ptr(), 2 * C,
                                                  out.hi, out.lo, C, precision, lens.data_ptr(), _stream()), "ns2_wavenet_block_lens")
        else:
            _lib.check(lib.ns2_wavenet_block(w.handle, a.hi, a.lo, a.ld, M, N, 4, cb.data_ptr(), rb.data_ptr(), film.data_ptr(), 2 * C,
                                             out.hi, out.lo, C, precision, _stream()), "ns2_wavenet_block")
        torch.cuda.synchronize()
        return out.buf

    try:
        _force_gemm(mode)
        before = _route_counts()
        ref, got = run(False), run(True)
        taken = _routes_taken(before)
    finally:
        _force_gemm(0)
    want = {1: "tile128", 2: "tile256", 5: "wavenet3" if precision == 5 else "tile128"}[mode]
    assert taken == {ROUTES[want]: 2}, (taken, want)
    _check_rows(got, ref, B, N, lens_l, f"wavenet block p{precision} mode {mode}")


# ------------------------------------------------------------------------------------------------ 2. attention, stand-alone
def _attn(q, k, vt, B, H, Nq, Nk, D, precision, key_lens, query_lens):
    o = _sentinel_planes(B * Nq, H * D, precision)
    a = _lib.AttnArgs(q_hi=q.hi, q_lo=q.lo, ldq=q.ld, k_hi=k.hi, k_lo=k.lo, ldk=k.ld, vt_hi=vt.hi, vt_lo=vt.lo, vt_ld=vt.ld, o_hi=o.hi,
                      o_lo=o.lo, ldo=o.ld, B=B, H=H, Nq=Nq, Nk=Nk, scale=D ** -0.5, head_dim=D, precision=precision)
    lib = _lib.load()
    if query_lens is not None:
        _lib.check(lib.ns2_attention_fwd_skip(ctypes.byref(a), None if key_lens is None else key_lens.data_ptr(), query_lens.data_ptr(),
                                              _stream()), "ns2_attention_fwd_skip")
    elif key_lens is not None:
        _lib.check(lib.ns2_attention_fwd_lens(ctypes.byref(a), key_lens.data_ptr(), _stream()), "ns2_attention_fwd_lens")
    else:
        _lib.check(lib.ns2_attention_fwd(a, _stream()), "ns2_attention_fwd")
    torch.cuda.synchronize()
    return o.buf


@pytest.mark.parametrize("batch", ["A", "B"])
@pytest.mark.parametrize("precision,D,cross", [(2, 64, False), (4, 64, False), (3, 32, False), (3, 64, False), (3, 128, False),
                                               (3, 64, True), (2, 64, True), (2, 64, "nokeys"), (4, 64, "nokeys"), (3, 64, "nokeys")])
def test_attention_skips_hidden_query_tiles(batch, precision, D, cross):
    """precisions 2 / 4 at D = 64 take attn_fast_kernel, precision 3 attn_kernel; cross: Nk = 32 keys, query lengths without key lengths;
    "nokeys": Nk = N with null key lengths (attn_fast_kernel's instantiation with query lengths alone)"""
    B, N, lens_l = BATCHES[batch]
    H, lens = 2, _lens(lens_l)
    Nk = 32 if cross is True else N
    sp = 2 if precision == 4 else precision
    q = ops.split(_rand((B * N, H * D), 31), precision=sp)
    k = ops.split(_rand((B * Nk, H * D), 32), precision=sp)
    vt = ops.split(_rand((B * H * D, Nk), 33), ldo=Nk, precision=sp)
    n0 = int(_lib.load().ns2_debug_attention_fast_launches())
    ref = _attn(q, k, vt, B, H, N, Nk, D, precision, None if cross else lens, None)
    got = _attn(q, k, vt, B, H, N, Nk, D, precision, None if cross else lens, lens)
    fast = int(_lib.load().ns2_debug_attention_fast_launches()) - n0
    assert fast == (2 if precision in (2, 4) and D == 64 and cross is not True else 0)
    _check_rows(got, ref, B, N, lens_l, f"attention p{precision} D{D} cross={cross} batch {batch}")


# ------------------------------------------------------------------------------------------------ 3, 4, 6. the model
CFG = {"uncond": dict(dim=256, depth=2, heads=4, dim_head=64),
       "cond": dict(dim=256, depth=2, heads=4, dim_head=64, dim_prompt=48, condition_on_prompt=True, num_latents_m=32)}


def _build(name, precision, **kw):
    m = Model(**CFG[name], precision=precision, **kw)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m.to(DEV).eval()


def _inputs(name, B, N, seed=2):
    x = make_input("x", (B, N, 256), seed=seed).to(DEV)
    t = make_input("times", (B,), seed=seed, uniform=True).to(DEV)
    kw = {}
    if name == "cond":
        kw = dict(prompt=make_input("prompt", (B, 7, 48), seed=seed).to(DEV), cond=make_input("cond", (B, 48, N), seed=seed).to(DEV))
    return x, t, kw


def _masked(y, lens_l):
    """where(row < H_i, y, 0)"""
    N = y.shape[1]
    keep = torch.arange(N, device=y.device)[None] < torch.tensor([extent(l, N) for l in lens_l], device=y.device)[:, None]
    return torch.where(keep[:, :, None], y, torch.zeros_like(y))


def _tapped(m, x, t, lens, kw, names):
    """names: {tap: columns per frame}"""
    lib, ns = _lib.load(), m._ensure_native()
    bufs = {k: torch.full((x.shape[0] * x.shape[1] * c,), SENT32, device=DEV) for k, c in names.items()}
    for k, b in bufs.items():
        _lib.check(lib.ns2_model_debug_tap(ns.handle, k.encode(), b.data_ptr(), b.numel()), "debug_tap")
    try:
        y = m(x, t, lens=lens, **kw).clone()
        torch.cuda.synchronize()
    finally:
        for k in bufs:
            lib.ns2_model_debug_tap(ns.handle, k.encode(), None, 0)
    return y, {k: b.view(x.shape[0], x.shape[1], -1) for k, b in bufs.items()}


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("precision", ["exact", "hybrid"])
@pytest.mark.parametrize("name", ["uncond", "cond"])
def test_model_skipping_step_keeps_the_visible_rows_and_zeroes_the_hidden_ones(name, precision, mode):
    B, N, lens_l = BATCHES["A"]
    lib, lens = _lib.load(), _lens(lens_l)
    m = _build(name, precision)
    x, t, kw = _inputs(name, B, N)
    taps = {"wavenet.out": 256, "layer0": 256}
    # operand planes, copied out as fp32: the init conv's output and the four Wavenet stacks' (8 grid-z layers of 256 columns side by side)
    plane_taps = {"wavenet.init": 256, **{f"wavenet.stack{s}": 8 * 256 for s in range(4)}}
    taps_all = {**taps, **plane_taps}
    try:
        _force_gemm(mode)
        ops.saturation_count(reset=True)
        with torch.no_grad():
            m.ragged_skip = False
            off, taps_off = _tapped(m, x, t, lens, kw, taps_all)
            assert int(lib.ns2_debug_skip_last()) == 0
            # 4. stale rows: today's forward gives its own bits on a workspace of 0xFF bytes (it carries no state between calls) ...
            ns = m._ensure_native()
            ns.ws.fill_(0xFF)
            assert torch.equal(m(x, t, lens=lens, **kw), off), "precondition: the workspace carries state between calls"
            # ... so the skipping forward starts from hidden rows that would move bits or trip the guard if anything read them
            ns.ws.fill_(0xFF)
            m.ragged_skip = True
            before = _route_counts()
            on, taps_on = _tapped(m, x, t, lens, kw, taps_all)
            taken = _routes_taken(before)
            assert int(lib.ns2_debug_skip_last()) == 1
        torch.cuda.synchronize()
        sat = ops.saturation_count(reset=True)
    finally:
        _force_gemm(0)
    # the kernels of the mode ran the skipping step: 256 x 256 alone, or (hybrid plan) the four grid-z launches of the lean Wavenet kernel,
    # the FF conv kernel once per layer and the lean linear kernel, the 128 x 128 kernel for the rest; nothing split K
    if mode == 2:
        assert set(taken) == {ROUTES["tile256"]}, taken
    else:
        assert ROUTES["splitk"] not in taken, taken
        if precision == "hybrid":
            assert taken.get(ROUTES["wavenet3"]) == 4 and taken.get(ROUTES["ffconv3"]) == 2 and taken.get(ROUTES["linear3"], 0) > 0, taken
    assert torch.isfinite(on).all() and torch.equal(on, _masked(off, lens_l))
    for k in taps:
        assert torch.isfinite(taps_on[k]).all() and torch.equal(taps_on[k], _masked(taps_off[k], lens_l)), k
    # every grid-z layer of every stack skipped its hidden row tiles: those rows of the planes still hold the 0xFF bytes the workspace was
    # filled with (NaN in every operand format), the rows before H_i have the bits of the step without skipping -- in all 8 column blocks
    for k in plane_taps:
        assert torch.isfinite(taps_off[k]).all(), k
        for b, l in enumerate(lens_l):
            h = extent(l, N)
            assert torch.equal(taps_on[k][b, :h], taps_off[k][b, :h]), (k, b)
            assert bool(torch.isnan(taps_on[k][b, h:]).all()), f"{k}: hidden rows of utterance {b} were written"
    assert sat == 0 and m.precision == precision            # the range guard saw nothing, hidden rows included


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_two_chains_equal_one_chain(precision):
    lib = _lib.load()
    B, N, lens_l = 4, 512, [512, 257, 1, 300]
    m = _build("uncond", precision, ragged_skip=True)
    x, t, _ = _inputs("uncond", B, N, seed=3)
    lens = _lens(lens_l)
    try:
        _force_gemm(5)
        with torch.no_grad():
            _lib.check(lib.ns2_debug_force_chains(1), "ns2_debug_force_chains")
            one = m(x, t, lens=lens).clone()
            ran_one, skip_one = int(lib.ns2_debug_chains_last()), int(lib.ns2_debug_skip_last())
            _lib.check(lib.ns2_debug_force_chains(2), "ns2_debug_force_chains")
            two = m(x, t, lens=lens).clone()
            ran_two, skip_two = int(lib.ns2_debug_chains_last()), int(lib.ns2_debug_skip_last())
            m.ragged_skip = False
            off = m(x, t, lens=lens).clone()
        torch.cuda.synchronize()
    finally:
        lib.ns2_debug_force_chains(0)
        _force_gemm(0)
    assert (ran_one, ran_two, skip_one, skip_two) == (1, 2, 1, 1)
    assert torch.equal(one, two) and torch.equal(two, _masked(off, lens_l))      # chain 1 reads lens + 2


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_guidance_path_equals_the_switch_off_result_before_the_extents(precision):
    B, N, lens_l = BATCHES["A"]
    m = _build("cond", precision)
    x, t, kw = _inputs("cond", B, N)
    lens = _lens(lens_l)
    try:
        _force_gemm(5)
        with torch.no_grad():
            off = m.forward_with_cond_scale(x, t, cond_scale=1.5, lens=lens, **kw).clone()
            m.ragged_skip = True
            on = m.forward_with_cond_scale(x, t, cond_scale=1.5, lens=lens, **kw).clone()
            ran = int(_lib.load().ns2_debug_skip_last())
        torch.cuda.synchronize()
    finally:
        _force_gemm(0)
    assert ran == 1 and torch.isfinite(on).all()
    for b, l in enumerate(lens_l):
        h = extent(l, N)
        assert torch.equal(on[b, :h], off[b, :h]), b
        assert torch.count_nonzero(on[b, h:]) == 0


@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_fallback_where_the_rule_refuses(precision):
    """N = 320 is no whole number of granules: the launches of the switch-off call, bit for bit"""
    m = _build("uncond", precision)
    x, t, _ = _inputs("uncond", 3, 320, seed=4)
    lens = _lens([320, 100, 1])
    with torch.no_grad():
        off = m(x, t, lens=lens).clone()
        m.ragged_skip = True
        on = m(x, t, lens=lens).clone()
        ran = int(_lib.load().ns2_debug_skip_last())
    assert ran == 0 and torch.equal(on, off)


# ------------------------------------------------------------------------------------------------ 5. the sampler
@pytest.mark.parametrize("precision", ["exact", "hybrid"])
def test_sampler_with_the_switch_on(precision):
    """every utterance equals itself sampled alone at its own length, bit for bit -- the yardstick tests/test_ragged_gpu.py established
    at 0.0 -- eager and captured, also after the lengths are rewritten in place between two replays"""
    B, N, lens_l = BATCHES["A"]
    m = _build("uncond", precision, ragged_skip=True)
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=8)
    noise = make_input("noise", (B, N, 256), seed=5)
    try:
        # 3 utterances: by shape the step would split K and the rule would refuse.  Mode 2 puts every product of the batch AND of the solo
        # runs (300 frames and 1 frame are no whole row tiles: no dedicated kernel takes them) on one kernel, the premise of the yardstick
        _force_gemm(2)
        out = d.sample(length=lens_l, batch_size=B, noise=noise)
        assert int(_lib.load().ns2_debug_skip_last()) == 1
        lens_dev = _lens(lens_l)
        graph = d.sample(length=lens_dev, batch_size=B, noise=noise, use_graph=True)
        assert torch.equal(graph, out) and torch.isfinite(out).all()
        for i, n in enumerate(lens_l):
            alone = d.sample(length=n, batch_size=1, noise=noise[i:i + 1, :n])
            assert torch.equal(out[i:i + 1, :n], alone), f"utterance {i} ({n} frames) differs from the utterance alone"
            assert torch.count_nonzero(out[i, n:]) == 0
        # a captured step reads no length on the host: a second replay after the lengths were rewritten in place follows them
        other = [256, 768, 513]
        x, t = noise.to(DEV), torch.full((B,), 0.5, device=DEV)
        with torch.no_grad():
            m(x, t, lens=lens_dev)                           # warm-up, outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                y = m(x, t, lens=lens_dev)
            g.replay()
            first = y.clone()
            lens_dev.copy_(_lens(other))
            g.replay()
            second = y.clone()
            assert torch.equal(first, m(x, t, lens=_lens(lens_l))) and torch.equal(second, m(x, t, lens=_lens(other)))
            assert int(_lib.load().ns2_debug_skip_last()) == 1
        for i, n in enumerate(other):
            h = extent(n, N)
            assert torch.count_nonzero(second[i, h:]) == 0 and torch.count_nonzero(second[i, :h]) > 0
        assert not torch.equal(first, second)
    finally:
        _force_gemm(0)
    assert m.precision == precision
