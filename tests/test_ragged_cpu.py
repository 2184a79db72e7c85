"""Ragged batches on the CPU: the composite restatement of the rule the HIP kernels follow (include/ns2hip.h) -- utterance i
of a ragged batch equals utterance i alone at its own length --, its pin to the oracle, its two entries of the C ABI, and the host
logic of NaturalSpeech2.sample(length=<per-utterance counts> / None) with the model step substituted by the composite."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, Model, NaturalSpeech2
from naturalspeech2_pytorch_amd.autograd_path import model_forward_autograd
from oracle import ns2_oracle as O
from tests.golden.gen import make_weights, make_input

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LENS = [40, 17, 1]
CONFIGS = {"uncond": dict(dim=64, depth=2),
           "cond": dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16)}
# Batch against solo.  The yardstick is the same comparison with no lengths involved -- an equal-length batch [3, 40, 64] of the
# composite against each of its utterances alone, a pure reduction-order effect -- measured on the code before this feature: worst
# utterance 5.51e-7 (unconditioned), 5.60e-7 (conditioned) on one host, 5.66e-7 / 5.82e-7 on another (the CPU's own GEMM and SDPA
# routes decide).  The bound is twice the smaller conditioned figure; with lengths the composite measures 5.47e-7 / 5.57e-7 on the
# first host and 5.44e-7 / 5.56e-7 on the second (profiles/ragged_sampling.json, "composite_cpu": the second host).
BATCH_VS_SOLO = 2 * 5.60e-7


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def case(request):
    kw = CONFIGS[request.param]
    m = Model(**kw).eval()
    sd = make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)
    m.load_state_dict(sd)
    x = make_input("x", (3, 40, 64), seed=2)
    t = make_input("times", (3,), seed=2, uniform=True)
    prompt = cond = None
    if kw.get("condition_on_prompt"):
        prompt = make_input("prompt", (3, 7, 48), seed=2)
        cond = make_input("cond", (3, 48, 40), seed=2)

    def solo(i):
        n = LENS[i]
        return (x[i:i + 1, :n], t[i:i + 1], None if prompt is None else prompt[i:i + 1], None if cond is None else cond[i:i + 1, :, :n])

    with torch.no_grad():                                  # computed once, shared, left unchanged
        alone = [model_forward_autograd(m, xs, ts, prompt=ps, cond=cs, cond_drop_prob=0.) for xs, ts, ps, cs in map(solo, range(3))]
    return dict(m=m, sd=sd, x=x, t=t, prompt=prompt, cond=cond, solo=solo, alone=alone)


def test_composite_utterance_in_a_ragged_batch_equals_the_utterance_alone(case):
    c = case
    with torch.no_grad():
        y = model_forward_autograd(c["m"], c["x"], c["t"], prompt=c["prompt"], cond=c["cond"], cond_drop_prob=0., lens=torch.tensor(LENS))
        y_leaky = model_forward_autograd(c["m"], c["x"], c["t"], prompt=c["prompt"], cond=c["cond"], cond_drop_prob=0.)
    assert torch.isfinite(y).all()
    for i, n in enumerate(LENS):
        e = rel(y[i:i + 1, :n], c["alone"][i])
        print(f"utterance {i} ({n} frames): ragged batch vs alone {e:.3e}")
        assert e <= BATCH_VS_SOLO, (i, e)
    leak = rel(y_leaky[1:2, :LENS[1]], c["alone"][1])       # without lengths the frames behind the end are keys: the test sees the leak
    print(f"utterance 1 without lens vs alone {leak:.3e}")
    assert leak > 1e-2
    assert torch.equal(y[0], y_leaky[0]) or rel(y[0], y_leaky[0]) <= BATCH_VS_SOLO      # a full-length utterance: the mask hides nothing


def test_composite_lens_accepts_a_list_and_clamps(case):
    c = case
    with torch.no_grad():
        a = model_forward_autograd(c["m"], c["x"], c["t"], prompt=c["prompt"], cond=c["cond"], cond_drop_prob=0., lens=[40, 17, 1])
        b = model_forward_autograd(c["m"], c["x"], c["t"], prompt=c["prompt"], cond=c["cond"], cond_drop_prob=0., lens=torch.tensor([45, 17, 0]))
    assert torch.equal(a, b)                                # outside [1, n] is clamped into it, as the kernels do


def test_composite_alone_is_the_oracle(case):
    c = case
    for i in range(3):
        xs, ts, ps, cs = c["solo"](i)
        with torch.no_grad():
            ref = O.model_forward(c["sd"], xs, ts, ps, cs, drop=False)
        assert rel(c["alone"][i], ref) < 2e-5, i           # the tolerance of tests/test_oracle.py


def test_training_path_names_lens():
    m = Model(dim=64, depth=1).train()
    with pytest.raises(NotImplementedError, match="lens"):
        m(torch.zeros(2, 8, 64), torch.zeros(2), lens=torch.tensor([8, 3]))


# ---- the C ABI
def test_ragged_header_parses_and_the_library_exports_it():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert {"ns2_attention_fwd_lens", "ns2_model_forward_lens"} <= set(_lib.header_symbols("ns2hip.h"))     # beside their base entries
    S = _lib.ABI["ns2hip.h"].signatures
    assert S["ns2_attention_fwd_lens"] == (I, [ctypes.POINTER(_lib.AttnArgs), P, P])
    assert S["ns2_model_forward_lens"] == (I, [P, P, P, P, P, P, I, P, I, I, P, L, P])
    _lib.load()                                                                  # raises unless the library exports them


def test_c99_caller_includes_both_headers_and_links(tmp_path):     # (the two headers of its day are one now)
    if shutil.which("gcc") is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs gcc and the built library")
    src = tmp_path / "ragged_caller.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "ns2hip.h"
int main(void) {
  ns2_attn_args a;
  int lens[2] = {3, 1};
  memset(&a, 0, sizeof a);
  int r0 = ns2_attention_fwd_lens(0, lens, 0), r1;
  r1 = ns2_attention_fwd_lens(&a, 0, 0);
  printf("%d %d\n", r0, r1);
  printf("%s\n", ns2_last_error());
  return ns2_model_forward_lens(0, 0, 0, 0, lens, 0, 0, 0, 1, 8, 0, 0, 0) != NS2_ERR_ARG;   /* argument errors come back as codes */
}
''')
    exe = tmp_path / "ragged_caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lns2hip",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out                        # the model entry refused too
    lines = out.stdout.splitlines()
    assert lines[0].split() == [str(_lib.NS2_ERR_ARG)] * 2 and lines[1].startswith("ns2_attention_fwd_lens:"), lines


def test_attention_fwd_lens_refuses_before_any_device_call():
    """no GPU here: an entry that reached a device call would come back with a HIP error, not with the argument error"""
    lib = _lib.load()
    fake = 1 << 20                                          # addresses that are compared against null and never read
    lens = (ctypes.c_int * 2)(3, 1)

    def refused(block, key_lens, word):
        rc = lib.ns2_attention_fwd_lens(None if block is None else ctypes.byref(block), key_lens, None)
        msg = lib.ns2_last_error().decode()
        assert rc == _lib.NS2_ERR_ARG and msg.startswith("ns2_attention_fwd_lens:") and word in msg, (rc, msg)

    def block(precision=2, **kw):
        return _lib.AttnArgs(q_hi=fake, k_hi=fake, vt_hi=fake, o_hi=fake, ldq=128, ldk=128, vt_ld=64, ldo=64, B=2, H=1, Nq=64, Nk=64,
                             scale=0.125, head_dim=64, precision=precision, **kw)
    refused(None, lens, "null argument block")
    refused(block(), None, "key_lens is null")
    refused(block(key_mask=fake), lens, "key_mask")
    refused(block(lse=fake, precision=3), lens, "lse")
    refused(block(dropout_p=0.1), lens, "dropout")
    rc = lib.ns2_model_forward_lens(None, fake, fake, fake, lens, None, 0, fake, 2, 8, None, 0, None)
    assert rc == _lib.NS2_ERR_ARG and lib.ns2_last_error().decode().startswith("ns2_model_forward_lens: exactly one of")


# ---- NaturalSpeech2.sample, the model step substituted by the composite (the way tests/test_host_cpu.py runs the sampler without a GPU)
@pytest.fixture
def composite_step():
    seen = []

    def step(self, x, times, prompt=None, prompt_mask=None, cond=None, cond_drop_prob=None, out=None, cond_row=None, lens=None):
        seen.append(None if lens is None else lens.clone())
        return model_forward_autograd(self, x, times, prompt=prompt, cond=cond, cond_drop_prob=cond_drop_prob, lens=lens)

    Model._forward_hip_saved = Model._forward_hip
    Model._forward_hip = step
    try:
        yield seen
    finally:
        Model._forward_hip = Model._forward_hip_saved
        del Model._forward_hip_saved


UNFUSED = dict(schedule_kwargs=dict(start=-3.0, end=3.0, tau=1.0))     # the schedule on the host: no HIP update kernel in the loop


def test_sample_length_int_tensor_list(composite_step):
    m = Model(dim=64, depth=1).eval()
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2, **UNFUSED)
    noise = make_input("noise", (3, 12, 64), seed=3)
    lens = [12, 5, 1]
    full = d.sample(length=12, batch_size=3, noise=noise)
    assert full.shape == (3, 12, 64) and composite_step == [None, None]            # an int: today's call, no lengths anywhere
    a = d.sample(length=torch.tensor(lens), batch_size=3, noise=noise)
    b, got = d.sample(length=lens, batch_size=3, noise=noise, return_lens=True)
    assert torch.equal(a, b) and a.shape == (3, 12, 64) and got.tolist() == lens and not got.dtype.is_floating_point
    assert all(l is not None and l.tolist() == lens for l in composite_step[2:]) and len(composite_step) == 6
    for i, n in enumerate(lens):
        assert torch.count_nonzero(a[i, n:]) == 0 and torch.count_nonzero(a[i, :n]) == n * 64
        alone = d.sample(length=n, batch_size=1, noise=noise[i:i + 1, :n])
        assert rel(a[i:i + 1, :n], alone) < 1e-5                                    # (the tight bound is the forward's, above)
    assert torch.equal(a[0], full[0]) or rel(a[0], full[0]) < 1e-5
    _, same = d.sample(length=12, batch_size=3, noise=noise, return_lens=True)
    assert same.tolist() == [12, 12, 12]
    with pytest.raises(ValueError, match="length"):
        d.sample(length=None, batch_size=3)
    with pytest.raises(ValueError, match="frame counts for a batch"):
        d.sample(length=[4, 4], batch_size=3)
    with pytest.raises(ValueError, match="1-D integer"):
        d.sample(length=torch.tensor([[4, 4, 4]]), batch_size=3)


def test_sample_lengths_from_text_and_text_lens(composite_step):
    m = Model(dim=64, depth=1, dim_prompt=32, condition_on_prompt=True, num_latents_m=8).eval()
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2, build_duration_pitch=True, duration_pitch_dim=32,
                       pitch_emb_pp_hidden_dim=32, dim_codebook=32, **UNFUSED)
    g = torch.Generator().manual_seed(4)
    text = torch.randint(0, 100, (2, 6), generator=g)
    enc = torch.randn(2, 6, 32, generator=g)
    dur = torch.tensor([[2.2, 1.0, 0.4, 3.9, 1.0, 2.0], [1.0, 2.7, 1.1, 2.0, 5.0, 1.0]])
    pitch = torch.rand(2, 6, generator=g) * 400
    d.phoneme_enc.forward = lambda ids, mask=None: enc                              # the two HIP front-end modules, substituted
    d.duration_pitch.forward = lambda x, prompts, prompt_mask=None: (dur, pitch)
    p_enc = torch.randn(2, 5, 32, generator=g)
    with pytest.raises(ValueError, match="text="):
        d.sample(length=None, prompt_enc=p_enc, cond=torch.zeros(2, 32, 9))
    audio, lens = d.sample(length=None, prompt_enc=p_enc, text=text, return_lens=True)
    assert lens.tolist() == [9, 12] and audio.shape == (2, 12, 64)                  # the totals of int(duration)
    assert torch.count_nonzero(audio[0, 9:]) == 0 and torch.count_nonzero(audio[0, :9]) == 9 * 64
    cut, lens_cut = d.sample(length=None, prompt_enc=p_enc, text=text, text_lens=torch.tensor([6, 3]), return_lens=True)
    assert lens_cut.tolist() == [9, 4] and cut.shape == (2, 9, 64)                  # phonemes 3.. of utterance 1 give no frames
    assert torch.count_nonzero(cut[1, 4:]) == 0 and torch.count_nonzero(cut[1, :4]) == 4 * 64
    cond, totals = d.text_to_cond(text, p_enc, text_lens=torch.tensor([6, 3]), return_lens=True)
    assert totals.tolist() == [9, 4] and torch.count_nonzero(cond[1, :, 4:]) == 0 and torch.is_tensor(d.text_to_cond(text, p_enc))
    # with a codec the lengths come back in samples and the samples behind an utterance's end are 0
    class Codec(torch.nn.Module):
        target_sample_hz, seq_len_multiple_of, codebook_dim = 24000, 4, 64
        def decode(self, emb):
            return emb.mean(dim=-1).repeat_interleave(4, dim=-1)[:, None] + 1.
    d.codec, d.seq_len_multiple_of = Codec(), 4
    wav, n_samples = d.sample(length=None, prompt_enc=p_enc, text=text, return_lens=True)
    assert wav.shape == (2, 48) and n_samples.tolist() == [36, 48]
    assert torch.count_nonzero(wav[0, 36:]) == 0 and torch.count_nonzero(wav[0, :36]) == 36
