"""Training at head dims 32 and 128 on the CPU (include/ns2hip_train.h): the three *_hd entries of the C ABI and what they
refuse, the `head_dim_training` switch of Model / Transformer / the encoders / DurationPitchPredictor, and the host logic of the
HIP pass (functions.py AttnFn: column offsets heads * head_dim, scale head_dim ** -0.5; model_pass.py: self, cross and perceiver attention)
on tests/emu_backend_head_dim.py against the composite's autograd."""
import ctypes

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, DurationPitchPredictor, Model, PhonemeEncoder, SpeechPromptEncoder, Transformer, training
from naturalspeech2_pytorch_amd.autograd_path import model_forward_autograd
from tests.emu_backend_head_dim import EmuBackendHeadDim
from tests.golden.gen import make_input, make_weights


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


# ---- the C ABI
def test_head_dim_train_header_parses_and_the_library_exports_it():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert {"ns2_attention_bwd_hd", "ns2_attention_delta_hd", "ns2_attention_train_fwd_hd"} <= set(_lib.header_symbols("ns2hip_train.h"))
    S = _lib.ABI["ns2hip_train.h"].signatures
    assert S["ns2_attention_train_fwd_hd"] == (I, [ctypes.POINTER(_lib.AttnArgs), P, P])
    assert S["ns2_attention_delta_hd"] == (I, [P, L, P, P, I, I, I, I, I, P, I, P])
    assert S["ns2_attention_bwd_hd"] == (I, [ctypes.POINTER(_lib.AttnBwdArgs), I, P, P])
    _lib.load()                                                                  # raises unless the library exports them


def test_the_three_entries_refuse_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error"""
    lib = _lib.load()
    fake = 1 << 20                                          # addresses that are compared against null and never read
    lens = (ctypes.c_int * 2)(3, 1)

    def fwd_block(**kw):
        f = dict(q_hi=fake, q_lo=fake + 64, k_hi=fake, k_lo=fake + 64, vt_hi=fake, vt_lo=fake + 64, o_hi=fake, o_lo=fake + 64, ldq=128, ldk=128,
                 vt_ld=64, ldo=64, B=2, H=1, Nq=64, Nk=64, scale=32 ** -0.5, head_dim=32, precision=3, lse=fake)
        f.update(kw)
        return _lib.AttnArgs(**f)

    def bwd_block(**kw):
        f = dict(q_hi=fake, q_lo=fake + 64, k_hi=fake, k_lo=fake + 64, v_hi=fake, v_lo=fake + 64, do_hi=fake, do_lo=fake + 64, ldq=64, ldk=64, ldv=64,
                 lddo=64, lse=fake, delta=fake, dq=fake, lddq=64, dk=fake, lddk=64, dv=fake, lddv=64, B=2, H=1, Nq=64, Nk=64, scale=32 ** -0.5)
        f.update(kw)
        return _lib.AttnBwdArgs(**f)

    def refused(name, rc, word):
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith(name + ":") and word in msg, (name, rc, msg)

    def fwd(blk, ln, word):
        refused("ns2_attention_train_fwd_hd", lib.ns2_attention_train_fwd_hd(None if blk is None else ctypes.byref(blk), ln, None), word)

    def bwd(blk, hd, ln, word):
        refused("ns2_attention_bwd_hd", lib.ns2_attention_bwd_hd(None if blk is None else ctypes.byref(blk), hd, ln, None), word)

    fwd(None, None, "null argument block")
    bwd(None, 32, None, "null argument block")
    for bad in (48, 16, 256, -1):
        fwd(fwd_block(head_dim=bad), None, "head_dim")
        bwd(bwd_block(), bad, None, "head_dim")
        refused("ns2_attention_delta_hd", lib.ns2_attention_delta_hd(fake, 64, fake, fake + 64, 64, 2, 1, 64, bad, fake, 3, None), "head_dim")
    fwd(fwd_block(lse=None), None, "lse is missing")
    bwd(bwd_block(lse=None), 32, None, "lse")
    fwd(fwd_block(precision=4), None, "precision 3")
    for ln in (lens,):
        fwd(fwd_block(Nk=32), ln, "Nq != Nk")
        fwd(fwd_block(key_mask=fake), ln, "key_mask")
        fwd(fwd_block(dropout_p=0.1, dropout_seed=fake), ln, "dropout")
        bwd(bwd_block(Nk=32), 128, ln, "Nq != Nk")
        bwd(bwd_block(key_mask=fake), 128, ln, "key_mask")
        bwd(bwd_block(dropout_p=0.1, dropout_seed=fake), 128, ln, "dropout")
    fwd(fwd_block(q_col0=16), None, "q_col0")
    fwd(fwd_block(k_col0=48), None, "k_col0")
    bwd(bwd_block(v_col0=16), 32, None, "v_col0")
    bwd(bwd_block(dq_col0=2), 32, None, "dq_col0")
    bwd(bwd_block(dv_col0=6), 128, None, "dv_col0")
    bwd(bwd_block(gp_hi=fake, gp_lo=fake + 64, gp_ld=192, gp_precision=3, gp_q=1, gp_kv=1, dk_col0=48), 32, None, "dk_col0")
    refused("ns2_attention_delta_hd", lib.ns2_attention_delta_hd(None, 64, fake, fake + 64, 64, 2, 1, 64, 32, fake, 3, None), "null pointer")
    refused("ns2_attention_delta_hd", lib.ns2_attention_delta_hd(fake, 64, fake, fake + 64, 64, 2, 1, 64, 32, fake, 2, None), "o_precision")
    # the entries of ns2hip.h keep their head dim of 64
    rc = lib.ns2_attention_fwd(fwd_block(), None)
    assert rc == _lib.NS2_ERR_ARG and "lse needs" in lib.ns2_last_error().decode()


# ---- the switch
def _modules(dim_head, **kw):
    return (Model(dim=64, depth=1, dim_head=dim_head, heads=2, **kw),
            [Transformer(dim=64, depth=1, dim_head=dim_head, heads=2, **kw),
             PhonemeEncoder(num_tokens=10, dim=64, dim_hidden=64, depth=1, dim_head=dim_head, heads=2, **kw),
             SpeechPromptEncoder(dim_codebook=32, dims=(64,), depth=1, dim_head=dim_head, heads=2, **kw)],
            DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=2, dim_head=dim_head, num_phoneme_tokens=10, **kw))


@pytest.mark.parametrize("dim_head", [32, 128])
def test_switch_off_is_todays_refusal_and_on_accepts_32_and_128(dim_head):
    m, encs, dp = _modules(dim_head)
    assert m.head_dim_training is False and dp.head_dim_training is False and encs[0].head_dim_training is False
    assert "dim_head" in training.unsupported_reason(m)
    assert all("dim_head" in training.encoder_unsupported_reason(e) for e in encs)
    assert "dim_head" in training.duration_pitch_unsupported_reason(dp)
    m, encs, dp = _modules(dim_head, head_dim_training=True)
    assert m.head_dim_training and dp.head_dim_training and all(getattr(e, "transformer", e).head_dim_training for e in encs)
    assert training.unsupported_reason(m) is None
    assert all(training.encoder_unsupported_reason(e) is None for e in encs)
    assert training.duration_pitch_unsupported_reason(dp) is None
    m.head_dim_training = False                             # a plain attribute, like ragged_training
    assert "dim_head" in training.unsupported_reason(m)


def test_switch_on_still_refuses_other_head_dims():
    m = Model(dim=64, depth=1, dim_head=48, heads=2, head_dim_training=True)
    assert "dim_head=48" in training.unsupported_reason(m)
    dp = DurationPitchPredictor(dim=64, dim_hidden=64, depth=1, heads=2, dim_head=32, num_phoneme_tokens=10, head_dim_training=True)
    dp.to_pitch_pred.dim_head = 48                          # (the constructors accept 32 / 64 / 128 only)
    assert "dim_head=48" in training.duration_pitch_unsupported_reason(dp)
    tr = Transformer(dim=64, depth=1, dim_head=32, heads=2, head_dim_training=True)
    tr.dim_head = 48
    assert "dim_head=48" in training.encoder_unsupported_reason(tr)
    assert training.unsupported_reason(Model(dim=64, depth=1, head_dim_training=True)) is None       # 64 stays what it was


# ---- the host logic of the HIP pass
@pytest.fixture()
def emu():
    bk = EmuBackendHeadDim()
    prev = training.set_backend(bk)
    yield bk
    training.set_backend(prev)


CASES = {"uncond_hd32": dict(dim=64, depth=1, dim_head=32, heads=2),
         "cond_hd128": dict(dim=64, depth=1, dim_head=128, heads=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_training_functions_at_head_dims_32_and_128_match_the_composite(emu, name):
    """functions.py / model_pass.py with `head_dim_training` on the emulated backend against torch autograd through the composite: the
    column offsets and the scale arrive right in AttnFn for self, cross and perceiver attention.  The tolerances of
    tests/test_ragged_training_cpu.py for the same comparison."""
    kw = CASES[name]
    m = Model(**kw, head_dim_training=True).train()
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    B, N = 2, 40
    x, t, cot = make_input("x", (B, N, 64), seed=2), make_input("times", (B,), seed=2, uniform=True), make_input("gw", (B, N, 64), seed=3)
    extra = {}
    if kw.get("condition_on_prompt"):
        extra = dict(prompt=make_input("prompt", (B, 7, 48), seed=2), cond=make_input("cond", (B, 48, N), seed=2), cond_drop_prob=0.)

    def run(fwd):
        for p in m.parameters():
            p.grad = None
        xr = x.clone().requires_grad_(True)
        y = fwd(m, xr, t, **extra)
        (y * cot).sum().backward()
        return y.detach(), xr.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}

    y0, dx0, g0 = run(model_forward_autograd)
    y1, dx1, g1 = run(training.model_forward_train)
    hd = kw["dim_head"]
    calls = [c for c in emu.calls if isinstance(c, tuple)]
    # uncond: 1 self attention; cond: 2 perceiver layers + (self + cross) -- every one of them got the head dim, forward, delta and backward
    want = 1 if not extra else 4
    assert [c[0] for c in calls].count("attention_hd") == want and [c[0] for c in calls].count("attention_bwd_hd") == want
    assert [c[0] for c in calls].count("attention_delta_hd") == want and all(c[1] == hd for c in calls)
    assert rel(y1, y0) < 1e-5 and rel(dx1, dx0) < 1e-4
    for k, ref in g0.items():
        if ref is None or ref.norm() == 0:
            assert g1[k] is None or g1[k].abs().max() == 0, k
            continue
        assert g1[k] is not None and g1[k].shape == ref.shape and rel(g1[k], ref) < 2e-4, (k, rel(g1[k], ref))


def test_head_dim_64_is_not_handed_to_the_backend():
    """tests/emu_backend.EmuBackend takes no head_dim keyword: a model of the default head dim with the switch on calls it as before"""
    from tests.emu_backend import EmuBackend
    prev = training.set_backend(EmuBackend())
    try:
        m = Model(dim=64, depth=1, heads=2, head_dim_training=True).train()
        x = make_input("x", (1, 16, 64), seed=2).requires_grad_(True)
        training.model_forward_train(m, x, make_input("times", (1,), seed=2, uniform=True)).sum().backward()
        assert torch.isfinite(x.grad).all()
    finally:
        training.set_backend(prev)
