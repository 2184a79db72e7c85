"""What per-utterance lengths cost and save in the three kernels of include/ns2hip_audio.h on one MI355X:

    python tools/bench_ragged_audio.py [--out profiles/ragged_audio.json] [--repeats 7] [--warmup 3]

Shapes: 32 x 327 680 samples for AudioToMel and PitchExtractor (the defaults: 24 kHz, n_fft 1024, hop 160, lags 37 .. 339), and
32 x 1024 frames x 8 quantizers x 1024 codes of 128 dims for the RVQ cross-entropy term, forward plus gradient in its one launch
(`ops.rvq_cross_entropy(..., need_grad=True)`).  Three arms each:
    plain    the existing entry, no lengths (ns2_audio_to_mel / ns2_pitch_yin / ns2_rvq_ce)
    full     the new entry with every length full
    ragged   the new entry with the lengths spread evenly over a quarter to the whole
A repeat is one pair of device events around `inner` back-to-back calls (as many as fill about 20 ms), divided by `inner`.  After
`warmup` untimed rounds the arms ALTERNATE -- plain, full, ragged, plain, ... -- for `repeats` rounds, so that a drift of the device hits
the three alike; median and range (min, max) per arm are recorded with every repeat.  No bar is fixed: nobody had measured these.
Writes the JSON file and prints it as one line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import AudioToMel, PitchExtractor, ops              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_audio.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ragged_audio.py times the HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
B, L, N, Q, C, D = 32, 327680, 1024, 8, 1024, 128
pe, mel = PitchExtractor(), AudioToMel()
assert pe.hip_supported() and mel.hip_supported()


def spread(whole, multiple=1):
    """B lengths spread evenly over a quarter of `whole` to the whole, multiples of `multiple`"""
    return [max(multiple, int(whole * (0.25 + 0.75 * i / (B - 1))) // multiple * multiple) for i in range(B)]


def window(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def alternate(arms):
    """arms: {name: callable} -> {name: dict(median_ms, min_ms, max_ms, inner, repeats_ms)}"""
    with torch.no_grad():
        inner = {}
        for name, fn in arms.items():
            window(fn, 1)
            inner[name] = max(1, min(1000, int(20. / max(window(fn, 2), 1e-3))))
        for _ in range(args.warmup):
            for name, fn in arms.items():
                window(fn, inner[name])
        ms = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                ms[name].append(window(fn, inner[name]))
    return {name: dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), inner=inner[name],
                       repeats_ms=[round(x, 5) for x in v]) for name, v in ms.items()}


def verdict(r):
    """the full-length arm against the existing entry, in the terms the README uses"""
    d = r["full"]["median_ms"] - r["plain"]["median_ms"]
    noise = max(r[a]["max_ms"] - r[a]["min_ms"] for a in ("plain", "full"))
    return dict(full_minus_plain_ms=round(d, 5), full_over_plain=round(r["full"]["median_ms"] / r["plain"]["median_ms"], 4),
                spread_between_repeats_ms=round(noise, 5), beyond_the_spread=bool(abs(d) > noise),
                ragged_over_plain=round(r["ragged"]["median_ms"] / r["plain"]["median_ms"], 4))


# ---- audio: a seeded harmonic tone with noise per utterance, as tools/bench_pitch.py makes it
g = torch.Generator(device=dev).manual_seed(B * 1000003 + L)
f = torch.linspace(90., 400., B, device=dev)[:, None]
phi = 2 * math.pi * f * torch.arange(L, device=dev)[None] / pe.sample_rate
audio = sum(a * torch.sin((k + 1) * phi + 0.7 * k) for k, a in enumerate((1., .5, .3, .2)))
audio = (0.3 * (audio + 0.05 * torch.randn(B, L, generator=g, device=dev))).contiguous()
del phi
s_full = torch.full((B,), L, dtype=torch.int32, device=dev)
s_ragged = torch.tensor(spread(L, 320), dtype=torch.int32, device=dev)

res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, B=B,
           ragged_share_of_padded=round(float(s_ragged.float().mean()) / L, 4))
res["audio_to_mel"] = alternate(dict(plain=lambda: mel(audio), full=lambda: mel(audio, lens=s_full), ragged=lambda: mel(audio, lens=s_ragged)))
res["audio_to_mel"].update(shape=[B, L], verdict=verdict(res["audio_to_mel"]))
res["pitch_yin"] = alternate(dict(plain=lambda: pe(audio), full=lambda: pe(audio, lens=s_full), ragged=lambda: pe(audio, lens=s_ragged)))
res["pitch_yin"].update(shape=[B, L], verdict=verdict(res["pitch_yin"]))
del audio

# ---- the RVQ term: latents near codes of a halving codebook stack, targets = the codes of the clean latents (ns2_rvq_encode)
g = torch.Generator(device=dev).manual_seed(7)
cb = (torch.randn(Q, C, D, generator=g, device=dev) * (0.5 ** torch.arange(Q, device=dev))[:, None, None]).contiguous()
norm = ops.rvq_prepare(cb)
lat = torch.randn(B * N, D, generator=g, device=dev)
idx, _ = ops.rvq_encode(lat, cb, norm)
x = (lat + 0.5 * torch.randn(B * N, D, generator=g, device=dev)).contiguous()
n_full = torch.full((B,), N, dtype=torch.int32, device=dev)
n_ragged = torch.tensor(spread(N), dtype=torch.int32, device=dev)
res["rvq_ce_fwd_grad"] = alternate(dict(plain=lambda: ops.rvq_cross_entropy(x, cb, norm, idx, True),
                                        full=lambda: ops.rvq_cross_entropy(x, cb, norm, idx, True, lens=n_full),
                                        ragged=lambda: ops.rvq_cross_entropy(x, cb, norm, idx, True, lens=n_ragged)))
res["rvq_ce_fwd_grad"].update(shape=[B, N, Q, C, D], verdict=verdict(res["rvq_ce_fwd_grad"]))

with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
