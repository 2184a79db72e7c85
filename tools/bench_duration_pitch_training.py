#!/usr/bin/env python
"""A warm training pass (forward + backward) of the DurationPitchPredictor at the reference's default sizes -- DurationPitchPredictor(dim=512):
two trunks of depth 10, attention dropout 0.2 -- at 32 x 256 phoneme encodings with 32 x 256 prompt rows, on the HIP training path
(`train_backend="hip"`) and on the PyTorch composite, ALTERNATING in one process.  A repeat = device events around `--iters`
passes that end in a synchronise; warm-up passes first.  The composite is untouched by the HIP path, so its time is the time
without the feature.  Writes profiles/duration_pitch_training.json with every repeat.

    python tools/bench_duration_pitch_training.py [--repeats 7] [--iters 3] [--warmup 2] [--only hip|composite] [--out PATH]

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

from naturalspeech2_pytorch_amd import DurationPitchPredictor                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None, choices=("hip", "composite"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duration_pitch_training.json"))
args = ap.parse_args()
assert args.repeats >= 5 or args.only, "at least five repeats per path"

B, N, NP = 32, 256, 256
dev = torch.device("cuda:0")


def build(which):
    torch.manual_seed(0)
    dp = DurationPitchPredictor(dim=512)
    inputs = (torch.randn(B, N, 512).to(dev).requires_grad_(True), torch.randn(B, NP, 512).to(dev).requires_grad_(True))
    proj = torch.randn(2, B, N).to(dev)
    return dp.to(dev).train(), inputs, proj


def set_backend(dp, backend):
    dp.train_backend = backend


def one_pass(dp, inputs, proj):
    for p in dp.parameters():
        p.grad = None
    for t in inputs:
        t.grad = None
    dur, pitch = dp(*inputs)
    ((dur * proj[0]).mean() + (pitch * proj[1]).mean()).backward()


def timed(enc, inputs, proj):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        one_pass(enc, inputs, proj)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


result = dict(batch=B, length=N, prompt_length=NP, iters_per_repeat=args.iters, warmup=args.warmup, device=torch.cuda.get_device_name(0), cases={})
backends = [args.only] if args.only else ["hip", "composite"]
for which in ("default_depth10",):
    enc, inputs, proj = build(which)
    times = {b: [] for b in backends}
    for b in backends:
        set_backend(enc, b)
        for _ in range(args.warmup):
            one_pass(enc, inputs, proj)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for b in backends:                                                        # alternating: drift hits both paths alike
            set_backend(enc, b)
            times[b].append(timed(enc, inputs, proj))
    case = {b: dict(ms_per_pass=t, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for b, t in times.items()}
    if len(backends) == 2:
        h, c = case["hip"], case["composite"]
        case["composite_over_hip_median"] = c["median_ms"] / h["median_ms"]
        # the HIP path counts as faster only when the gap exceeds the spread seen between repeats of the same path
        spread = max(h["max_ms"] - h["min_ms"], c["max_ms"] - c["min_ms"])
        case["gap_ms"], case["spread_ms"] = c["median_ms"] - h["median_ms"], spread
        case["hip_faster_beyond_spread"] = bool(c["median_ms"] - h["median_ms"] > spread)
    result["cases"][which] = case
    print(which, json.dumps({k: v for k, v in case.items() if not isinstance(v, dict)}),
          {b: [round(x, 2) for x in times[b]] for b in backends}, flush=True)
    del enc, inputs, proj
    torch.cuda.empty_cache()
if not args.only:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)
