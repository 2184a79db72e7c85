"""Time of PitchExtractor's HIP kernel (csrc/pitch.hip) on one MI355X, AudioToMel's on the same audio beside it for scale:

    python tools/bench_pitch.py [--out profiles/pitch_extract.json] [--repeats 7] [--warmup 3]

Two shapes: 32 x 327 680 samples (BASELINE config 4's audio) and 1 x 24 000, at the defaults (24 kHz, hop 160, lags 37 .. 339).
The audio is a seeded harmonic tone with noise per utterance (F0 from 90 to 400 Hz), so that the searches run as they do on voiced
speech.  A repeat is one pair of device events around `inner` back-to-back calls (as many as fill about 20 ms), divided by
`inner`; after `warmup` untimed repeats, `repeats` of them give the median and the spread (min, max) recorded per shape.
`pairs` = frames x tau_max x 2 tau_max, the subtract-multiply-add pairs of the difference function, the kernel's work.
There is no bar to clear: nothing before this module did the work on the GPU.  Writes the JSON file and prints it as one line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import AudioToMel, PitchExtractor                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_extract.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_pitch.py times the HIP kernel: it needs the GPU"
dev = torch.device("cuda:0")
pe, mel = PitchExtractor(), AudioToMel()
assert pe.hip_supported() and mel.hip_supported()


def make_audio(B, L):
    g = torch.Generator(device=dev).manual_seed(B * 1000003 + L)
    f = torch.linspace(90., 400., B, device=dev)[:, None] if B > 1 else torch.full((1, 1), 220., device=dev)
    phi = 2 * math.pi * f * torch.arange(L, device=dev)[None] / pe.sample_rate
    x = sum(a * torch.sin((k + 1) * phi + 0.7 * k) for k, a in enumerate((1., .5, .3, .2)))
    return (0.3 * (x + 0.05 * torch.randn(B, L, generator=g, device=dev))).contiguous()


def timed(fn):
    def window(inner):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / inner
    with torch.no_grad():
        window(1)
        inner = max(1, min(1000, int(20. / max(window(2), 1e-3))))
        for _ in range(args.warmup):
            window(inner)
        ms = [window(inner) for _ in range(args.repeats)]
    return dict(median_ms=round(statistics.median(ms), 5), min_ms=round(min(ms), 5), max_ms=round(max(ms), 5), inner=inner)


res = dict(sample_rate=pe.sample_rate, hop_length=pe.hop_length, tau_min=pe.tau_min, tau_max=pe.tau_max, repeats=args.repeats,
           warmup=args.warmup, device=torch.cuda.get_device_name(0), shapes=[])
for B, L in ((32, 327680), (1, 24000)):
    audio = make_audio(B, L)
    T = 1 + L // pe.hop_length
    f0 = pe(audio)
    row = dict(B=B, L=L, frames=B * T, voiced_share=round(float((f0 > 0).float().mean()), 4), pairs=B * T * pe.tau_max * 2 * pe.tau_max,
               pitch_yin=timed(lambda: pe(audio)), audio_to_mel=timed(lambda: mel(audio)))
    row["pairs_per_s"] = round(row["pairs"] / (row["pitch_yin"]["median_ms"] * 1e-3), 1)
    res["shapes"].append(row)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
