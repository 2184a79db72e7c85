#!/usr/bin/env python
"""The RVQ cross-entropy term of the training loss (`codec.rq(x_start, codes)`, NS2:1668-1684) at the headline shape -- 32 x 1024 frames,
8 quantizers of 1024 codes of 128 dims -- on the fused HIP kernel (`ResidualVQCrossEntropy(backend="hip")`, csrc/rvq_ce.hip) and on the
PyTorch composite, ALTERNATING in one process:

  rq     a warm forward + backward of `codec.rq` alone (x requires a gradient; the loss is backpropagated)
  step   a warm training step (loss + backward) of `NaturalSpeech2(Model(dim=128, depth=6), codec, rvq_cross_entropy_loss_weight=0.1)`: the
         codec's codebook dim fixes the denoiser's (NS2:1244), so this is the d128 / L6 configuration, on its HIP training path

A repeat = device events around `--iters` passes that end in a synchronise; warm-up passes first.  The composite is untouched by the HIP
path, so its time is the time without the feature.  `torch.cuda.max_memory_allocated` is reset before and read after every repeat.  Writes
profiles/rvq_ce_training.json with every repeat.

    python tools/bench_rvq_ce_training.py [--repeats 7] [--iters 3] [--warmup 2] [--only hip|composite] [--skip-step] [--out PATH]

`--only hip --repeats 1` is the run to put under `rocprofv3 --kernel-trace --stats` (a run of its own).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2                      # noqa: E402
from naturalspeech2_pytorch_amd.codec import EncodecWrapperHIP                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None, choices=("hip", "composite"))
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rvq_ce_training.json"))
args = ap.parse_args()
assert args.repeats >= 5 or args.only, "at least five repeats per path"

B, N, Q, C, D = 32, 1024, 8, 1024, 128
dev = torch.device("cuda:0")
torch.manual_seed(0)
codebooks = torch.randn(Q, C, D) * (0.5 ** torch.arange(Q, dtype=torch.float32))[:, None, None]
codec = EncodecWrapperHIP(codebooks).to(dev)
latents = torch.randn(B, N, D).to(dev)
_, codes, _ = codec(latents)                                                      # the codec's own codes of the clean latents
x = (latents + 0.5 * torch.randn(B, N, D, device=dev)).requires_grad_(True)
times, noise = torch.rand(B, device=dev), torch.randn(B, N, D, device=dev)
model = Model(dim=D, depth=6).to(dev).train()
diffusion = NaturalSpeech2(model, codec=codec, rvq_cross_entropy_loss_weight=0.1).to(dev)
backends = [args.only] if args.only else ["hip", "composite"]


def rq_pass(backend):
    codec.rq.backend = backend
    x.grad = None
    _, ce = codec.rq(x, codes)
    ce.backward()


def step_pass(backend):
    codec.rq.backend = backend
    for p in model.parameters():
        p.grad = None
    diffusion(latents, codes=codes, times=times, noise=noise).backward()


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters, torch.cuda.max_memory_allocated() / 2 ** 20


def summary(t, mem):
    return dict(ms=t, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), peak_allocated_mib=max(mem))


def measure(one_pass):
    times_, mem = {b: [] for b in backends}, {b: [] for b in backends}
    for b in backends:
        for _ in range(args.warmup):
            one_pass(b)
    for _ in range(args.repeats):
        for b in backends:                                                        # alternating: drift hits both paths alike
            t, m = timed(lambda: one_pass(b))
            times_[b].append(t)
            mem[b].append(m)
    case = {b: summary(times_[b], mem[b]) for b in backends}
    if len(backends) == 2:
        h, c = case["hip"], case["composite"]
        case["composite_over_hip_median"] = c["median_ms"] / h["median_ms"]
        # the HIP path counts as faster only when the gap exceeds the spread seen between repeats of the same path
        spread = max(h["max_ms"] - h["min_ms"], c["max_ms"] - c["min_ms"])
        case["gap_ms"], case["spread_ms"] = c["median_ms"] - h["median_ms"], spread
        case["hip_faster_beyond_spread"] = bool(c["median_ms"] - h["median_ms"] > spread)
    return case


result = dict(batch=B, frames=N, quantizers=Q, codes=C, dim=D, step_model=dict(dim=D, depth=6), loss_weight=0.1, iters_per_repeat=args.iters,
              warmup=args.warmup, device=torch.cuda.get_device_name(0))
for name, fn in (("rq", rq_pass),) + (() if args.skip_step else (("step", step_pass),)):
    result[name] = measure(fn)
    print(name, json.dumps({k: (v if not isinstance(v, dict) else {a: (round(b, 3) if isinstance(b, float) else [round(z, 3) for z in b])
                                                                  for a, b in v.items()}) for k, v in result[name].items()}), flush=True)

if not args.only:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)
