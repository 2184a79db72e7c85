"""Wall time of AudioToMel on one MI355X, the HIP kernel against the GPU composite (torch.stft + matmul + log10), profiles/r09_*:

    python tools/bench_audio_to_mel.py [--iters 20] [--warmup 3] [--mode both|hip|composite] [--B 32] [--L 327680]

B x L fp32 samples (default: BASELINE config 4's batch, 32 x 327 680), the reference's defaults (n_mels 100, n_fft 1024,
win_length 640, hop_length 160, log).  Times are device events around `iters` calls.  `bytes` = 4 B L + 4 B n_mels T, what one
pass must move; `bytes_per_s_wall` divides it by the HIP wall time.  For the kernel's own time and rate, run this under
`rocprofv3 --kernel-trace --stats` (a separate run) and divide `bytes` by the kernel's average duration.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naturalspeech2_pytorch_amd import AudioToMel                                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--mode", default="both", choices=("both", "hip", "composite"))
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--L", type=int, default=327680)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
audio = torch.randn(args.B, args.L, generator=g, device=dev)
m = AudioToMel()
T = 1 + args.L // m.hop_length
runs = {"hip": lambda: m(audio), "composite": lambda: m._forward_composite(audio)}


def timed(fn):
    with torch.no_grad():
        for _ in range(args.warmup):
            out = fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            out = fn()
        end.record()
        end.synchronize()
    return start.elapsed_time(end) / args.iters, out


res = dict(B=args.B, L=args.L, n_mels=m.n_mels, n_fft=m.n_fft, hop_length=m.hop_length, frames=args.B * T, iters=args.iters,
           bytes=4 * args.B * args.L + 4 * args.B * m.n_mels * T)
outs = {}
for name, fn in runs.items():
    if args.mode in ("both", name):
        ms, outs[name] = timed(fn)
        res[f"{name}_wall_ms"] = round(ms, 4)
if "hip" in outs:
    res["bytes_per_s_wall_hip"] = round(res["bytes"] / (res["hip_wall_ms"] * 1e-3), 1)
if len(outs) == 2:
    res["ratio_composite_over_hip"] = round(res["composite_wall_ms"] / res["hip_wall_ms"], 2)
    res["max_abs_db_diff"] = float((outs["hip"] - outs["composite"]).abs().max())
print(json.dumps(res))
