"""What per-utterance lengths (Model.forward(lens=), include/ns2hip.h) cost and save on one MI355X:

    python tools/bench_ragged_sampling.py [--out profiles/ragged_sampling.json] [--repeats 7] [--warmup 3]

1. The d512 / L12 hybrid denoising step (model forward + DDIM update, eager) at 32 x 1024 frames, three ways: `lens=None`, all lengths
   1024, lengths spread evenly over 256 ... 1024.  A repeat is one pair of device events around `inner` back-to-back steps (as many as
   fill about 200 ms), divided by `inner`; after `warmup` untimed repeats, `repeats` rounds visit the three variants in turn
   (alternating), and the median and the spread (min, max) of each are recorded.  The self-attention kernel time of a step comes from
   the library's own device events around the attention launches (ns2_model_profile_begin, category 5), in passes of their own.
   (`attention_launches_profiled` counts products; where a step runs as two utterance chains each product is two launches, which is
   what `attention_launches_on_attn_fast_kernel` counts.)
2. Batch against solo, the tolerance of the ragged tests: an utterance of a batch against the same utterance alone, as relative L2
   error.  `yardstick`: no lengths involved (an equal-length batch; a pure reduction-order effect, the same on the code before
   lengths existed); `ragged`: the batch carries lengths and the solo run has the utterance's own length.  For the 8-step sampler on
   the GPU (d64 / depth 2 at 4 x 256 frames, exact and hybrid) and for one forward of the composite on the CPU (3 x 40 frames).

This is a capability first: attention is about a tenth of the step and the GEMMs still multiply the padding rows, so no speed-up of
the step is claimed or aimed at.  Writes the JSON file and prints it as one line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, ops                     # noqa: E402
from naturalspeech2_pytorch_amd.autograd_path import model_forward_autograd              # noqa: E402
from tests.golden.gen import make_input, make_weights                                    # noqa: E402  (the seeded weights and inputs of the tests)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_sampling.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ragged_sampling.py times HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
lib = _lib.load()


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ---- 1. the step
B, N, DIM, DEPTH = 32, 1024, 512, 12
torch.manual_seed(1234)
model = Model(dim=DIM, depth=DEPTH, precision="hybrid").to(dev).eval()
g = torch.Generator().manual_seed(100)
x0 = torch.randn(B, N, DIM, generator=g).to(dev)
t_cur, t_nxt = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.49, device=dev)
variants = {"lens_none": None,
            "lens_all_1024": torch.full((B,), N, dtype=torch.int32, device=dev),
            "lens_256_to_1024": torch.linspace(256, N, B).round().to(device=dev, dtype=torch.int32)}
audio = x0.clone()


def step(lens):
    out = model(audio, t_cur, lens=lens)
    ops.ddim_step(audio, out, t_cur, t_nxt, "v", "sigmoid", 1., out=audio)


def window(lens, inner):
    audio.copy_(x0)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        step(lens)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def attention_ms(lens, steps=5):
    """the self-attention launches of `steps` steps: summed kernel time per step, launches per step"""
    h = model._ensure_native().handle
    ms, n = ctypes.c_double(0), ctypes.c_int64(0)
    audio.copy_(x0)
    torch.cuda.synchronize()
    _lib.check(lib.ns2_model_profile_begin(h, 1 << 5), "ns2_model_profile_begin")
    for _ in range(steps):
        step(lens)
    _lib.check(lib.ns2_model_profile_end(h, ctypes.byref(ms), ctypes.byref(n)), "ns2_model_profile_end")
    return ms.value / steps, n.value // steps


res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
           step=dict(model=f"Model(dim={DIM}, depth={DEPTH}, precision='hybrid')", batch=B, frames=N, what="model forward + DDIM update, eager",
                     lens_256_to_1024=[int(v) for v in variants["lens_256_to_1024"].tolist()], variants={}))
with torch.no_grad():
    for lens in variants.values():
        window(lens, 1)
    inner = max(1, min(200, int(200. / max(window(None, 2), 1e-3))))
    for _ in range(args.warmup):
        for lens in variants.values():
            window(lens, inner)
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):                          # alternating: every round visits the three variants
        for k, lens in variants.items():
            ms[k].append(window(lens, inner))
    fast0 = int(lib.ns2_debug_attention_fast_launches())
    for k, lens in variants.items():
        a_ms, a_n = attention_ms(lens)
        res["step"]["variants"][k] = dict(step_median_ms=round(statistics.median(ms[k]), 4), step_min_ms=round(min(ms[k]), 4),
                                          step_max_ms=round(max(ms[k]), 4), inner=inner, self_attention_ms_per_step=round(a_ms, 4),
                                          self_attention_launches_per_step=a_n)
    res["step"]["attention_launches_on_attn_fast_kernel"] = int(lib.ns2_debug_attention_fast_launches()) - fast0
    res["step"]["attention_launches_profiled"] = 3 * 5 * DEPTH
del model, audio, x0
torch.cuda.empty_cache()

# ---- 2. batch against solo
LENS = [256, 100, 30, 200]
noise = make_input("noise", (4, 256, 64), seed=5)


def seeded(**kw):
    m = Model(**kw)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m.eval()


res["sampler_batch_vs_solo"] = dict(model="Model(dim=64, depth=2)", batch=4, frames=256, timesteps=8, lens=LENS,
                                    metric="relative L2 error of an utterance of the batch against the utterance sampled alone")
for precision in ("exact", "hybrid"):
    m = seeded(dim=64, depth=2, precision=precision).to(dev)
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=8)
    full = d.sample(length=256, batch_size=4, noise=noise)
    yard = [rel(full[i:i + 1], d.sample(length=256, batch_size=1, noise=noise[i:i + 1])) for i in range(4)]
    rag = d.sample(length=LENS, batch_size=4, noise=noise)
    ragged = [rel(rag[i:i + 1, :n], d.sample(length=n, batch_size=1, noise=noise[i:i + 1, :n])) for i, n in enumerate(LENS)]
    res["sampler_batch_vs_solo"][precision] = dict(yardstick=yard, yardstick_worst=max(yard), ragged=ragged, ragged_worst=max(ragged),
                                                   stayed_in_precision=m.precision == precision)

CL = [40, 17, 1]
res["composite_cpu"] = dict(batch=3, frames=40, lens=CL, metric="relative L2 error, one forward of the PyTorch composite on the CPU")
for name, kw in (("uncond", dict(dim=64, depth=2)), ("cond", dict(dim=64, depth=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16))):
    m = seeded(**kw)
    x, t = make_input("x", (3, 40, 64), seed=2), make_input("times", (3,), seed=2, uniform=True)
    pr = cd = None
    if "dim_prompt" in kw:
        pr, cd = make_input("prompt", (3, 7, 48), seed=2), make_input("cond", (3, 48, 40), seed=2)
    one = lambda v, i: None if v is None else v[i:i + 1]                                  # noqa: E731
    with torch.no_grad():
        yb = model_forward_autograd(m, x, t, prompt=pr, cond=cd, cond_drop_prob=0.)
        yr = model_forward_autograd(m, x, t, prompt=pr, cond=cd, cond_drop_prob=0., lens=CL)
        yard = [rel(yb[i:i + 1], model_forward_autograd(m, x[i:i + 1], t[i:i + 1], prompt=one(pr, i), cond=one(cd, i), cond_drop_prob=0.))
                for i in range(3)]
        ragged = [rel(yr[i:i + 1, :n], model_forward_autograd(m, x[i:i + 1, :n], t[i:i + 1], prompt=one(pr, i),
                                                               cond=None if cd is None else cd[i:i + 1, :, :n], cond_drop_prob=0.))
                  for i, n in enumerate(CL)]
    res["composite_cpu"][name] = dict(yardstick=yard, yardstick_worst=max(yard), ragged=ragged, ragged_worst=max(ragged))

with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
