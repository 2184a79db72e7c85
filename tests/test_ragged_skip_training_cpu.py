"""Skipping the hidden row tiles of a ragged TRAINING batch, on the CPU (include/ns2hip.h ns2_linear_lens_zero, include/ns2hip_train.h ns2_wgrad_rows_lens): the three entries of the
C ABI and what its two entries refuse, the `ragged_skip_training` switch of Model and where it does nothing, and the host logic of the
skipping pass (functions.py / model_pass.py on tests/emu_backend_ragged_skip_train.py, which asserts who is handed the lengths) against
torch autograd through the composite with the same lengths."""
import ctypes
import inspect

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, Model, compat, training
from naturalspeech2_pytorch_amd.autograd_path import model_forward_autograd_ragged
from tests.emu_backend_ragged_skip_train import EmuBackendRaggedSkipTrain, extent
from tests.golden.gen import make_input, make_weights

B, N, LENS = 3, 512, [512, 200, 7]                          # extents 512, 256, 256: no hidden tile, one behind a partial granule, one behind a short utterance
NC = N - 8                                                  # frames of cond: another row count than the b n frame rows (padded behind the projection)
CONFIGS = {"uncond": dict(dim=64, depth=2),
           "cond": dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


def _model(name, **kw):
    m = Model(**CONFIGS[name], **kw).train()
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m


def _inputs(name, n=N, nc=NC):
    x = make_input("x", (B, n, 64), seed=2)
    t = make_input("times", (B,), seed=2, uniform=True)
    cot = make_input("gw", (B, n, 64), seed=3)
    prompt = cond = None
    if CONFIGS[name].get("condition_on_prompt"):
        prompt, cond = make_input("prompt", (B, 7, 48), seed=2), make_input("cond", (B, 48, nc), seed=2)
    return x, t, prompt, cond, cot


def _run(m, fwd, x, t, prompt, cond, cot):
    for p in m.parameters():
        p.grad = None
    kw = {} if prompt is None else dict(prompt=prompt, cond=cond, cond_drop_prob=0.)
    y = fwd(x, t, **kw)
    (y * cot).sum().backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


# ---- the C ABI
def test_ragged_skip_train_header_parses_and_the_library_exports_it():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert {"ns2_debug_train_skip_launches", "ns2_linear_lens_zero"} <= set(_lib.header_symbols("ns2hip.h"))       # beside ns2_linear_lens
    assert "ns2_wgrad_rows_lens" in _lib.header_symbols("ns2hip_train.h")                                          # beside ns2_wgrad_rows
    sig = {k: _lib.SIGNATURES[k] for k in ("ns2_debug_train_skip_launches", "ns2_linear_lens_zero", "ns2_wgrad_rows_lens")}
    assert sig["ns2_linear_lens_zero"] == (I, [ctypes.POINTER(_lib.LinearArgs), P, I, P]) == _lib.SIGNATURES["ns2_linear_lens"]
    assert sig["ns2_debug_train_skip_launches"] == (L, [])
    # ns2_wgrad_rows with the lengths in front of the stream
    res, args = _lib.SIGNATURES["ns2_wgrad_rows"]
    assert sig["ns2_wgrad_rows_lens"] == (res, args[:-1] + [P, args[-1]])
    lib = _lib.load()                                         # raises unless the library exports them
    assert lib.ns2_debug_train_skip_launches() >= 0           # host arithmetic: no device needed


def test_the_two_entries_refuse_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error; a refused call
    is not counted"""
    lib = _lib.load()
    fake = 1 << 20                                          # addresses that are compared against null and never read
    lens = (ctypes.c_int * 3)(512, 200, 7)
    n0 = lib.ns2_debug_train_skip_launches()

    def refused(rc, name, word):
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith(name) and word in msg, (name, rc, msg)

    blk = _lib.LinearArgs(w=fake, a_hi=fake, a_lo=fake + 64, lda=64, M=1536, precision=3, out_f32=fake, ldo_f=64)
    lin = lib.ns2_linear_lens_zero
    refused(lin(None, lens, 512, None), "ns2_linear_lens_zero:", "null argument block")
    refused(lin(ctypes.byref(blk), None, 512, None), "ns2_linear_lens_zero:", "row_lens is null")
    refused(lin(ctypes.byref(blk), lens, 0, None), "ns2_linear_lens_zero:", "multiple of 256")
    refused(lin(ctypes.byref(blk), lens, 384, None), "ns2_linear_lens_zero:", "multiple of 256")
    refused(lin(ctypes.byref(blk), lens, 1024, None), "ns2_linear_lens_zero:", "whole utterances")
    blk.seq_len = 256
    refused(lin(ctypes.byref(blk), lens, 512, None), "ns2_linear_lens_zero:", "args->seq_len differs")
    blk.seq_len, blk.w = 0, None
    refused(lin(ctypes.byref(blk), lens, 512, None), "ns2_linear:", "w is null")      # whatever ns2_linear refuses is refused alike

    def wg(M=1536, seq=512, ln=lens, prec=3, ws=fake):
        return lib.ns2_wgrad_rows_lens(fake, fake + 64, 64, fake, fake + 64, 64, M, 64, 1, 64, 64, 1, seq, fake, ws, 1 << 30, prec, ln, None)

    refused(wg(ln=None), "ns2_wgrad_rows_lens:", "row_lens is null")
    refused(wg(seq=0), "ns2_wgrad_rows_lens:", "multiple of 256")
    refused(wg(seq=320), "ns2_wgrad_rows_lens:", "multiple of 256")
    refused(wg(M=1000), "ns2_wgrad_rows_lens:", "whole utterances")
    refused(wg(prec=2), "ns2_wgrad_rows:", "precision 3")                              # ... and whatever ns2_wgrad_rows refuses
    refused(wg(ws=None), "ns2_wgrad_rows:", "null pointer")
    assert lib.ns2_debug_train_skip_launches() == n0


def test_the_granule_is_the_one_of_the_sampling_header():
    assert extent(torch.tensor([0, 1, 255, 256, 257, 512, 513, 9999], dtype=torch.int32), 768).tolist() == [256, 256, 256, 256, 512, 512, 768, 768]


# ---- the switch
def test_the_switch_is_a_keyword_and_a_plain_attribute_and_defaults_to_off():
    assert Model(dim=64, depth=1).ragged_skip_training is False
    m = Model(dim=64, depth=1, ragged_training=True, ragged_skip_training=True)
    assert m.ragged_skip_training is True and m.ragged_skip is False           # `ragged_skip` keeps its meaning: sampling only
    m.ragged_skip_training = False

    class Ref(torch.nn.Module):                             # stands in for the reference class: the keyword is compat's own
        def __init__(self, dim, depth=1, dim_head=64, heads=8, ff_mult=4, wavenet_layers=8, wavenet_stacks=4, dim_cond_mult=4,
                     condition_on_prompt=False, dim_prompt=None, num_latents_m=32, resampler_depth=2):
            super().__init__()

    assert "ragged_skip_training" in inspect.signature(compat.hip_backed_model_class(Ref).__init__).parameters


def test_on_the_cpu_the_switch_does_nothing():
    """Model.forward under autograd on the CPU is the composite: the same values with the switch on, with NaN behind the lengths"""
    m = _model("uncond", ragged_training=True)
    x, t, _, _, cot = _inputs("uncond", n=256)
    lens = torch.tensor([256, 100, 7])
    for i, n in enumerate(lens.tolist()):
        x[i, n:] = float("nan")
    y0, g0 = _run(m, lambda xs, ts: m(xs, ts, lens=lens), x, t, None, None, cot)
    m.ragged_skip_training = True
    y1, g1 = _run(m, lambda xs, ts: m(xs, ts, lens=lens), x, t, None, None, cot)
    assert torch.isfinite(y1).all() and torch.equal(y0, y1) and all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.fixture()
def emu_factory():
    prev = []

    def make(frame_rows):
        bk = EmuBackendRaggedSkipTrain(frame_rows)
        prev.append(training.set_backend(bk))
        return bk
    yield make
    if prev:
        training.set_backend(prev[0])


def test_without_lens_or_with_n_not_a_multiple_of_256_no_product_is_handed_lengths(emu_factory):
    bk = emu_factory(None)                                  # any row_lens trips the backend's assertion
    m = _model("uncond", ragged_training=True, ragged_skip_training=True)
    x, t, _, _, cot = _inputs("uncond", n=64)
    _run(m, lambda xs, ts: training.model_forward_train(m, xs, ts), x, t, None, None, cot)                                  # no lens
    _run(m, lambda xs, ts: training.model_forward_train(m, xs, ts, lens=torch.tensor([64, 20, 7])), x, t, None, None, cot)  # 64 % 256 != 0
    m.ragged_skip_training = False
    x, t, _, _, cot = _inputs("uncond", n=256)
    _run(m, lambda xs, ts: training.model_forward_train(m, xs, ts, lens=torch.tensor([256, 20, 7])), x, t, None, None, cot)  # the switch off
    assert bk.skipped == []


# ---- the host logic of the skipping pass
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_skipping_pass_matches_the_composite_and_the_pass_that_computes_every_row(emu_factory, name):
    """functions.py / model_pass.py with the switch on, on the emulated backend whose skipping products write zeros into hidden tiles and
    which asserts who is handed the lengths, against torch autograd through the composite with the same lengths (the tolerances of
    tests/test_ragged_training_cpu.py) and against the same pass with the switch off.  NaN lies behind the lengths in x and cond."""
    m = _model(name, ragged_training=True)
    x, t, prompt, cond, cot = _inputs(name)
    for i, n in enumerate(LENS):
        x[i, n:] = float("nan")
        if cond is not None:
            cond[i, :, n:] = float("nan")
    lens = torch.tensor(LENS, dtype=torch.int32)
    y0, g0 = _run(m, lambda xs, ts, **kw: model_forward_autograd_ragged(m, xs, ts, lens, **kw), x, t, prompt, cond, cot)
    emu_factory(None)                                       # the switch off: no product may carry lengths
    y1, g1 = _run(m, lambda xs, ts, **kw: training.model_forward_train(m, xs, ts, lens=lens, **kw), x, t, prompt, cond, cot)
    bk = emu_factory(B * N)                                 # the switch on: every frame-row product must, no other may
    m.ragged_skip_training = True
    y2, g2 = _run(m, lambda xs, ts, **kw: training.model_forward_train(m, xs, ts, lens=lens, **kw), x, t, prompt, cond, cot)
    kinds = {k for k, _ in bk.skipped}
    assert kinds == {"gemm_f32", "gemm_split", "wgrad_rows"} and all(rows == B * N for _, rows in bk.skipped)
    assert all(c[1] is lens for c in bk.calls if isinstance(c, tuple))      # the attention kernels keep the caller's own tensor
    assert torch.isfinite(y2).all() and all(torch.count_nonzero(y2[i, n:]) == 0 for i, n in enumerate(LENS))
    assert rel(y2, y0) < 1e-5 and rel(y2, y1) < 1e-6
    worst = ("", 0.0)
    for k, ref in g0.items():
        if ref is None or ref.norm() == 0:
            assert g2[k] is None or g2[k].abs().max() == 0, k
            continue
        assert g2[k] is not None and g2[k].shape == ref.shape and torch.isfinite(g2[k]).all(), k
        e = rel(g2[k], ref)
        worst = max(worst, (k, e), key=lambda z: z[1])
        assert e < 2e-4, (k, e)
        assert rel(g2[k], g1[k]) < 1e-6, (k, rel(g2[k], g1[k]))            # only exact zeros left the sums
    print("worst parameter gradient against the composite:", worst)
    xr = x.clone().requires_grad_(True)
    kw = {} if prompt is None else dict(prompt=prompt, cond=cond, cond_drop_prob=0.)
    (training.model_forward_train(m, xr, t, lens=lens, **kw) * cot).sum().backward()
    xc = x.clone().requires_grad_(True)
    (model_forward_autograd_ragged(m, xc, t, lens, **kw) * cot).sum().backward()
    assert rel(xr.grad, xc.grad) < 1e-4 and all(torch.count_nonzero(xr.grad[i, n:]) == 0 for i, n in enumerate(LENS))
