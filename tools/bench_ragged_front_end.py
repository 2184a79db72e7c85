"""What per-utterance prompt and text lengths (include/ns2hip_frontend.h) cost in the conditioning front-end on one MI355X:

    python tools/bench_ragged_front_end.py [--out profiles/ragged_front_end.json] [--repeats 7] [--warmup 2]

The front-end of one sample() call at the default sizes -- 32 utterances x 256 phonemes x 256 prompt frames through the default
SpeechPromptEncoder, PhonemeEncoder, DurationPitchPredictor and the conditioning of the d512 / L12 hybrid denoiser:
`prompt_enc` + `text_to_cond` (phoneme encoder, predictor, length regulator, its one host read included) + the model's prepare_cond --
three ways: no lengths, all lengths full, lengths spread evenly over 64 ... 256 (prompt and text alike).  A repeat is one pair of device
events around one front-end pass; after `warmup` untimed rounds, `repeats` rounds visit the three variants in turn (alternating), and the
median and the spread (min, max) of each are recorded.  The length path adds launches (row zeroing behind every "same" convolution, the
key mask) and saves nothing but attention tiles: a capability, no speed-up is claimed.  Writes the JSON file and prints it as one line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import Model, NaturalSpeech2                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_front_end.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ragged_front_end.py times HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
B, N_TEXT, N_PROMPT, DIM, DEPTH = 32, 256, 256, 512, 12
torch.manual_seed(1234)
model = Model(dim=DIM, depth=DEPTH, dim_prompt=512, condition_on_prompt=True, precision="hybrid")
d = NaturalSpeech2(model, codec=None, target_sample_hz=24000, build_duration_pitch=True).to(dev).eval()
with torch.no_grad():
    d.duration_pitch.to_duration_pred.to_pred[0].bias.fill_(2.5)       # a few frames per phoneme instead of an untrained head's zeros
    d.duration_pitch.to_pitch_pred.to_pred[0].bias.fill_(150.)
g = torch.Generator().manual_seed(100)
text = torch.randint(0, 150, (B, N_TEXT), generator=g).to(dev)
latents = torch.randn(B, N_PROMPT, 128, generator=g).to(dev)
spread = torch.linspace(64, 256, B).round().to(device=dev, dtype=torch.int32)
variants = {"lens_none": None, "lens_all_full": (torch.full((B,), N_PROMPT, dtype=torch.int32, device=dev),
                                                 torch.full((B,), N_TEXT, dtype=torch.int32, device=dev)),
            "lens_64_to_256": (spread, spread.clone())}


def front(lens):
    if lens is None:
        p_enc = d.prompt_enc(latents)
        cond = d.text_to_cond(text, p_enc)
        pl = None
    else:
        pl, tl = lens
        p_enc = d.prompt_enc(latents, lens=pl)
        cond = d.text_to_cond(text, p_enc, text_lens=tl, prompt_lens=pl)
    model.clear_cond_cache()
    model._cond_state(model._ensure_native(), p_enc, cond, False, B, cond.shape[2], pl)
    return cond.shape[2]


def window(lens):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    frames = front(lens)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), frames


res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, batch=B, phonemes=N_TEXT, prompt_frames=N_PROMPT,
           model=f"Model(dim={DIM}, depth={DEPTH}, dim_prompt=512, condition_on_prompt=True, precision='hybrid')",
           what="prompt_enc + text_to_cond + the model's prepare_cond, one pass, device events (the length regulator's host read included)",
           lens_64_to_256=[int(v) for v in spread.tolist()], variants={})
with torch.no_grad():
    for _ in range(args.warmup):
        for lens in variants.values():
            window(lens)
    ms, frames = {k: [] for k in variants}, {}
    for _ in range(args.repeats):                          # alternating: every round visits the three variants
        for k, lens in variants.items():
            t, frames[k] = window(lens)
            ms[k].append(t)
for k in variants:
    res["variants"][k] = dict(median_ms=round(statistics.median(ms[k]), 4), min_ms=round(min(ms[k]), 4), max_ms=round(max(ms[k]), 4),
                              cond_frames=int(frames[k]))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
