#!/usr/bin/env python
"""DurationPitchPredictor (dim 512, depth 10) + the length regulator at B = 32, n_ph = 256, n_p = 225: the HIP path against the
PyTorch composite (autograd_path.py) on the same GPU.  Wall time per call with a synchronise at each end; kernel time and
launch counts come from a separate `rocprofv3 --kernel-trace --stats` run of the same script with --mode hip / composite.

    python tools/bench_duration_pitch.py [--mode both|hip|composite] [--iters N]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                          # noqa: E402

from naturalspeech2_pytorch_amd import DurationPitchPredictor, ops   # noqa: E402
from naturalspeech2_pytorch_amd import autograd_path as AP            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="both", choices=("both", "hip", "composite"))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

B, N_PH, N_P, D = 32, 256, 225, 512
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = DurationPitchPredictor(dim=D).eval().to(dev)
with torch.no_grad():                    # heads biased to 1-6 frames and 80-400 Hz, as the golden fixtures
    for tr, bias in ((m.to_duration_pred, 3.5), (m.to_pitch_pred, 240.)):
        tr.to_pred[0].weight.mul_(0.01)
        tr.to_pred[0].bias.fill_(bias)
g = torch.Generator().manual_seed(1)
x = torch.randn(B, N_PH, D, generator=g).to(dev)
p = torch.randn(B, N_P, D, generator=g).to(dev)
table = torch.randn(256, D, generator=g).to(dev)


def hip():
    dur, pitch = m(x, p)
    return ops.length_regulate(dur, pitch, x, table)


def composite():
    dur, pitch = AP.duration_pitch_autograd(m, x, p)
    return AP.length_regulate(dur, pitch, x, table)


def timed(fn):
    with torch.no_grad():
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            out = fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.iters, out


res = dict(B=B, n_ph=N_PH, n_p=N_P, dim=D, depth=10, iters=args.iters)
outs = {}
for name, fn in (("hip", hip), ("composite", composite)):
    if args.mode in ("both", name):
        ms, outs[name] = timed(fn)
        res[f"{name}_wall_ms"] = round(ms, 3)
if args.mode == "both":
    res["wall_ratio_composite_over_hip"] = round(res["composite_wall_ms"] / res["hip_wall_ms"], 3)
    a, b = outs["hip"], outs["composite"]
    res["n_frames"] = [a.shape[-1], b.shape[-1]]
    if a.shape == b.shape:
        res["cond_max_abs_diff"] = float((a - b).abs().max())
print(json.dumps(res))
