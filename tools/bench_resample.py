"""Time of Resample's HIP kernel (csrc/resample.hip) on one MI355X against the PyTorch composite (pad, conv1d, transpose, crop) on the same
GPU and the same audio:

    python tools/bench_resample.py [--out profiles/resample.json] [--repeats 9] [--warmup 3]

Two pairs, 48 kHz -> 24 kHz (up 1, down 2, 28 taps per phase) and 44.1 kHz -> 24 kHz (up 80, down 147, 171 taps per phase), each on
32 x 327 680 samples of seeded white noise (BASELINE config 4's batch and length).  A window is one pair of device events around `inner`
back-to-back calls (as many as fill about 20 ms), divided by `inner`.  After `warmup` untimed windows of each, `repeats` windows of the
kernel and of the composite ALTERNATE (kernel, composite, kernel, ...), so that what else runs on the machine falls on both alike; the
median and the spread (min, max) of each are recorded, with the ratio of the medians.  `bytes` = the input read once and the output
written once (the tap table stays in cache), so bytes / time is the share of the memory rate the call reaches, allocation of the output
included.  `max_abs_diff` compares the two results on the timed input.  For the record: there is no bar to clear, nothing before this
module did the work on the GPU.  Writes the JSON file and prints it as one line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import Resample                                      # noqa: E402
from naturalspeech2_pytorch_amd.resample import resample_composite                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_resample.py times the HIP kernel: it needs the GPU"
dev = torch.device("cuda:0")
B, L = 32, 327680


def window(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def alternate(fns):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms, inner)}: warm-up of each, then the timed windows in turn"""
    with torch.no_grad():
        inner = {}
        for k, fn in fns.items():
            window(fn, 1)
            inner[k] = max(1, min(1000, int(20. / max(window(fn, 2), 1e-3))))
            for _ in range(args.warmup):
                window(fn, inner[k])
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(window(fn, inner[k]))
    return {k: dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), inner=inner[k])
            for k, v in ms.items()}


res = dict(B=B, L=L, repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0), pairs=[])
for orig, new in ((48000, 24000), (44100, 24000)):
    mod = Resample(orig, new)
    assert mod.hip_supported()
    audio = torch.rand(B, L, device=dev, generator=torch.Generator(device=dev).manual_seed(orig)) * 2 - 1
    got, ref = mod(audio), resample_composite(audio, orig, new)
    row = dict(orig_hz=orig, new_hz=new, up=mod.up, down=mod.down, taps_per_phase=2 * mod.width + mod.down, L_out=got.shape[-1],
               bytes=4 * B * (L + got.shape[-1]), fma=B * got.shape[-1] * (2 * mod.width + mod.down),
               max_abs_diff=float((got - ref).abs().max()))
    row.update(alternate(dict(kernel=lambda: mod(audio), composite=lambda: resample_composite(audio, orig, new))))
    row["composite_over_kernel"] = round(row["composite"]["median_ms"] / row["kernel"]["median_ms"], 2)
    row["kernel_bytes_per_s"] = round(row["bytes"] / (row["kernel"]["median_ms"] * 1e-3), 1)
    res["pairs"].append(row)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
