"""What per-utterance text and prompt lengths cost in the TRAINING pass of the conditioning (include/ns2hip_train.h) on one MI355X:

    python tools/bench_ragged_conditioning.py [--out profiles/ragged_conditioning.json] [--repeats 7] [--warmup 2]

One warm forward + backward of the default SpeechPromptEncoder, PhonemeEncoder and DurationPitchPredictor (`train_backend="hip"`,
`ragged_conditioning=True`, dropouts as built) at 32 utterances x 256 phonemes x 256 prompt rows, three ways: no lengths, all lengths full
(device tensors: the length path runs), lengths spread evenly over a quarter to the whole (prompt and text alike).  A repeat is one pair
of device events around one forward + backward; after `warmup` untimed rounds, `repeats` rounds visit the three arms in turn
(alternating), and the median and the spread (min, max) of each are recorded.  The length path adds launches (the row selects behind
every "same" convolution and their backward, the byte masks) and runs the key-mask attention kernels, while the GEMMs still multiply
the padding: a capability, no speed-up is claimed.  The "timing" key of the JSON file is replaced, its other keys (the tests' recorded
figures) are kept; the result is printed as one line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import DurationPitchPredictor, PhonemeEncoder, SpeechPromptEncoder      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_conditioning.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ragged_conditioning.py times HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
B, N_TEXT, N_PROMPT = 32, 256, 256
torch.manual_seed(1234)
kw = dict(train_backend="hip", ragged_conditioning=True)
prompt_enc = SpeechPromptEncoder(dim_codebook=128, **kw).to(dev).train()
phoneme_enc = PhonemeEncoder(num_tokens=150, train_backend="hip").to(dev).train()
predictor = DurationPitchPredictor(dim=512, **kw).to(dev).train()
params = [p for m in (prompt_enc, phoneme_enc, predictor) for p in m.parameters()]
g = torch.Generator().manual_seed(100)
text = torch.randint(0, 150, (B, N_TEXT), generator=g).to(dev)
latents = torch.randn(B, N_PROMPT, 128, generator=g).to(dev)
spread = torch.linspace(N_TEXT // 4, N_TEXT, B).round().to(device=dev, dtype=torch.int32)
full = torch.full((B,), N_TEXT, dtype=torch.int32, device=dev)
arms = {"lens_none": None, "lens_all_full": (full, full.clone()), "lens_quarter_to_whole": (spread, spread.clone())}


def step(lens):
    for p in params:
        p.grad = None
    if lens is None:
        p_enc = prompt_enc(latents)
        ph = phoneme_enc(text)
        dur, pitch = predictor(ph, p_enc)
    else:
        pl, tl = lens
        p_enc = prompt_enc(latents, lens=pl)
        ph = phoneme_enc(text, lens=tl)
        dur, pitch = predictor(ph, p_enc, text_lens=tl, prompt_lens=pl)
    (dur.sum() + pitch.sum() + p_enc.sum() * 1e-3).backward()


def window(lens):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    step(lens)
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


timing = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, batch=B, phonemes=N_TEXT, prompt_rows=N_PROMPT,
              what="forward + backward of the default SpeechPromptEncoder, PhonemeEncoder and DurationPitchPredictor (train_backend='hip'), device events",
              lens_quarter_to_whole=[int(v) for v in spread.tolist()], arms={})
for _ in range(args.warmup):
    for lens in arms.values():
        window(lens)
ms = {k: [] for k in arms}
for _ in range(args.repeats):                              # alternating: every round visits the three arms
    for k, lens in arms.items():
        ms[k].append(window(lens))
for k in arms:
    timing["arms"][k] = dict(median_ms=round(statistics.median(ms[k]), 4), min_ms=round(min(ms[k]), 4), max_ms=round(max(ms[k]), 4))
res = {}
try:
    with open(args.out) as f:
        res = json.load(f)
except Exception:
    pass
res["timing"] = timing
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(timing))
