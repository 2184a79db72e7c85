"""Skipping the hidden row tiles of a ragged sampling batch (include/ns2hip.h), the parts that need no GPU: the header and
its exports, the skip rule (host arithmetic over the described step), the refusals that come before any device call, the computed-extent
formula of the measurement tool, and the `ragged_skip` switch of Model on a recording stand-in for the library."""
import ctypes
import importlib.util
import os

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, Model
from tests.emu_skip_lib import plumbed

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ["ns2_attention_fwd_skip", "ns2_debug_gemm_route_launches", "ns2_debug_skip_last", "ns2_debug_skip_rule", "ns2_linear_lens", "ns2_model_forward_lens_skip",
           "ns2_wavenet_block_lens"]


def test_ragged_skip_header_parses_and_the_library_exports_it():
    P, I, L, PTR = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER
    S = _lib.ABI["ns2hip.h"].signatures
    assert set(ENTRIES) <= set(_lib.header_symbols("ns2hip.h"))
    assert S["ns2_linear_lens"] == (I, [PTR(_lib.LinearArgs), P, I, P]) and S["ns2_attention_fwd_skip"] == (I, [PTR(_lib.AttnArgs), P, P, P])
    assert S["ns2_model_forward_lens_skip"] == _lib.SIGNATURES["ns2_model_forward_lens"] == (I, [P, P, P, P, P, P, I, P, I, I, P, L, P])
    assert S["ns2_wavenet_block_lens"] == (I, [P, P, P, I, I, I, I, P, P, P, I, P, P, I, I, P, P])
    assert S["ns2_debug_skip_rule"] == (I, [PTR(_lib.ModelConfig), I, I, P])
    assert S["ns2_debug_skip_last"] == (I, []) and S["ns2_debug_gemm_route_launches"] == (L, [I])
    _lib.load()                                                                  # raises unless the library exports them


def _cfg(dim, depth, precision, heads=8, dim_head=64):
    return _lib.ModelConfig(dim=dim, depth=depth, dim_head=dim_head, heads=heads, ff_mult=4, wavenet_layers=8, wavenet_stacks=4,
                            dim_cond_mult=4, condition_on_prompt=0, dim_prompt=0, num_latents_m=32, resampler_depth=2, precision=precision)


def _rule(cfg, B, N):
    skips = ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_skip_rule(ctypes.byref(cfg), B, N, ctypes.byref(skips)), "ns2_debug_skip_rule")
    return skips.value


@pytest.mark.parametrize("precision", [3, 5])
def test_skip_rule(precision):
    """whole 256-row granules per utterance and no split-K product: d512 / L12 skips at 32 x 1024 and at 3 x 768 under hook mode 5 (no
    split); N = 1000 never skips; one utterance of 1024 frames plans split-K products (ns2_debug_splitk_plan's rule) and does not skip"""
    lib = _lib.load()
    cfg = _cfg(512, 12, precision)
    try:
        _lib.check(lib.ns2_debug_force_gemm(0), "ns2_debug_force_gemm")
        assert _rule(cfg, 32, 1024) == 1
        assert _rule(cfg, 32, 1000) == 0
        assert _rule(cfg, 1, 1024) == 0                    # split-K is planned: the rule refuses
        _lib.check(lib.ns2_debug_force_gemm(5), "ns2_debug_force_gemm")      # never split K
        assert _rule(cfg, 3, 768) == 1 and _rule(cfg, 1, 1024) == 1 and _rule(cfg, 3, 1000) == 0
    finally:
        lib.ns2_debug_force_gemm(0)
    bad = lib.ns2_debug_skip_rule(ctypes.byref(cfg), 0, 1024, None)
    assert bad == _lib.NS2_ERR_ARG and lib.ns2_last_error().decode().startswith("ns2_debug_skip_rule:")


def test_3_x_768_does_not_skip_by_shape():
    """3 x 768 = 2304 rows under the default hook: 18 x 4 tiles of 128 x 128 are fewer than the chip's CUs, the K = 8 dim skip-sum and the
    folded FF conv split K (ns2_debug_splitk_plan says so for their shapes), and the rule refuses -- batches that small are out of scope"""
    lib = _lib.load()
    S, c = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.ns2_debug_splitk_plan(3 * 768, 512, 8 * 512 // 32, 8 * 512 // 32, 0, ctypes.byref(S), ctypes.byref(c)), "ns2_debug_splitk_plan")
    assert S.value >= 2
    for precision in (3, 5):
        assert _rule(_cfg(512, 12, precision), 3, 768) == 0
        assert _rule(_cfg(512, 12, precision), 16, 768) == 1       # 96 x 4 tiles of 128 x 128: nothing splits any more


def test_refusals_come_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error"""
    lib = _lib.load()
    fake = 1 << 20
    lens = (ctypes.c_int * 3)(768, 300, 1)

    def refused(rc, name, word):
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith(name + ":") and word in msg, (rc, msg)

    block = _lib.LinearArgs(w=fake, a_hi=fake, a_lo=fake + 64, lda=96, M=900, precision=3, out_f32=fake, ldo_f=256)
    refused(lib.ns2_linear_lens(ctypes.byref(block), lens, 300, None), "ns2_linear_lens", "multiple of 256")
    refused(lib.ns2_linear_lens(ctypes.byref(block), None, 256, None), "ns2_linear_lens", "row_lens is null")
    refused(lib.ns2_linear_lens(ctypes.byref(block), lens, 256, None), "ns2_linear_lens", "whole utterances")     # 900 % 256
    refused(lib.ns2_linear_lens(None, lens, 256, None), "ns2_linear_lens", "null argument block")
    refused(lib.ns2_wavenet_block_lens(fake, fake, fake, 256, 900, 300, 1, fake, fake, fake, 512, fake, fake, 256, 3, lens, None),
            "ns2_wavenet_block_lens", "multiple of 256")
    a = _lib.AttnArgs(q_hi=fake, k_hi=fake, vt_hi=fake, o_hi=fake, ldq=128, ldk=128, vt_ld=320, ldo=64, B=3, H=1, Nq=320, Nk=320, scale=0.125,
                      head_dim=64, precision=2)
    refused(lib.ns2_attention_fwd_skip(ctypes.byref(a), lens, lens, None), "ns2_attention_fwd_skip", "multiple of 256")
    a.Nq = a.Nk = 256
    refused(lib.ns2_attention_fwd_skip(ctypes.byref(a), lens, None, None), "ns2_attention_fwd_skip", "query_lens is null")
    a.key_mask = fake
    refused(lib.ns2_attention_fwd_skip(ctypes.byref(a), None, lens, None), "ns2_attention_fwd_skip", "key_mask")
    refused(lib.ns2_model_forward_lens_skip(None, fake, fake, None, None, None, 0, fake, 3, 768, None, 0, None),
            "ns2_model_forward_lens_skip", "frame_lens is null")
    assert lib.ns2_debug_skip_last() in (0, 1) and lib.ns2_debug_gemm_route_launches(6) == -1 and lib.ns2_debug_gemm_route_launches(0) >= 0


def _tool():
    spec = importlib.util.spec_from_file_location("bench_ragged_skip", os.path.join(ROOT, "tools", "bench_ragged_skip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_computed_extent_and_hidden_shares_of_the_tool():
    tool = _tool()
    H = lambda l, n: min(n, 256 * ((min(max(l, 1), n) + 255) // 256))                      # noqa: E731  (the header's formula, restated)
    share = lambda lens, n: sum((n - H(l, n)) // 256 for l in lens) / (len(lens) * n // 256)   # noqa: E731
    for n in (256, 768, 1024):
        for l in (-3, 0, 1, 255, 256, 257, 300, 512, 513, 767, 768, 1024, 5000):
            assert tool.computed_extent(l, n) == H(l, n), (l, n)
    assert [tool.computed_extent(l, 768) for l in (768, 300, 1)] == [768, 512, 256]
    assert [tool.computed_extent(l, 512) for l in (1, 257, 512)] == [256, 512, 512]
    spread = torch.linspace(256, 1024, 32).round().to(torch.int32).tolist()                 # the spread of tools/bench_ragged_sampling.py
    assert tool.hidden_share(spread, 1024) == share(spread, 1024)
    assert 0.2 < tool.hidden_share(spread, 1024) < 0.3                                       # about a quarter of the tiles: what a step can save
    assert tool.hidden_share([1024] * 32, 1024) == 0.0 and tool.hidden_share([768, 300, 1], 768) == share([768, 300, 1], 768) == 3 / 9


def test_model_switch_reaches_the_new_entry_only_with_lengths_and_without_autograd():
    m = Model(dim=64, depth=1, ragged_skip=True).eval()
    assert m.ragged_skip is True and Model(dim=64, depth=1).ragged_skip is False
    x, t, lens = torch.zeros(2, 256, 64), torch.zeros(2), torch.tensor([256, 3], dtype=torch.int32)
    with plumbed(m) as rec, torch.no_grad():
        m(x, t, lens=lens)
        assert rec.calls == ["ns2_model_forward_lens_skip"]
        del rec.calls[:]
        m(x, t)                                               # without lengths the switch does nothing
        m(x, t, lens=None)
        assert rec.calls == ["ns2_model_forward", "ns2_model_forward"]
        del rec.calls[:]
        m.ragged_skip = False                                 # a plain attribute
        m(x, t, lens=lens)
        assert rec.calls == ["ns2_model_forward_lens"]
    # under autograd the switch changes nothing: the training pass refuses lengths exactly as it does without it ...
    m.ragged_skip = True
    m.train()
    with pytest.raises(NotImplementedError, match="lens"):
        m(torch.zeros(2, 8, 64), torch.zeros(2), lens=torch.tensor([8, 3]))
    # ... and a model that trains on ragged batches gives the bits it gives with the switch off
    mt = Model(dim=64, depth=1, ragged_training=True).train()
    xs, ts, ls = torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(0)), torch.tensor([0.3, 0.6]), torch.tensor([8, 3])
    off = mt(xs, ts, lens=ls)
    mt.ragged_skip = True
    on = mt(xs, ts, lens=ls)
    assert on.requires_grad and torch.equal(on, off)
