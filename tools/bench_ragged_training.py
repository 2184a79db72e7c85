"""What per-utterance lengths in the TRAINING pass (Model(ragged_training=True), NaturalSpeech2.forward(audio_lens=),
include/ns2hip_train.h) cost and save on one MI355X:

    python tools/bench_ragged_training.py [--out profiles/ragged_training.json] [--repeats 7] [--warmup 3]

1. `step`: the d512 / L12 model at 32 x 1024 frames, train_precision="mixed", one loss + backward (NaturalSpeech2.forward + loss.backward(),
   eager), three arms: `lens_none` (no audio_lens: today's pass), `lens_all_1024`, `lens_256_to_1024` (lengths spread evenly).  A repeat is
   one pair of device events around `inner` back-to-back steps, divided by `inner`; after `warmup` untimed repeats, `repeats` rounds visit
   the three arms in turn (alternating), and the median and the spread (min, max) of each are recorded.
2. `kernels`: the twelve self-attention forward + backward pairs of such a step alone (HipBackend.attention / attention_bwd on operand
   planes of 32 x 8 heads x 1024 frames, the gradients leaving as operand planes), the same three arms, the same protocol.

This is a capability first: attention is about a tenth of the step and the GEMMs still multiply the padding rows, so no speed-up of the
step is claimed or aimed at.  Keys of the output file other than `device`, `step` and `kernels` (the tolerances the tests quote) are kept.
Prints the result as one line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, ops                          # noqa: E402
from naturalspeech2_pytorch_amd.training import HipBackend                                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_training.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_ragged_training.py times HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
B, N, DIM, DEPTH, HEADS = 32, 1024, 512, 12, 8
arms = {"lens_none": None,
        "lens_all_1024": torch.full((B,), N, dtype=torch.int32, device=dev),
        "lens_256_to_1024": torch.linspace(256, N, B).round().to(device=dev, dtype=torch.int32)}


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def measure(run, target_ms=200.):
    """run(lens) -> {arm: dict(median, min, max, inner)} by the protocol of the module docstring"""
    for lens in arms.values():
        timed(lambda: run(lens), 1)
    inner = max(1, min(200, int(target_ms / max(timed(lambda: run(None), 2), 1e-3))))
    for _ in range(args.warmup):
        for lens in arms.values():
            timed(lambda: run(lens), inner)
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):                          # alternating: every round visits the three arms
        for k, lens in arms.items():
            ms[k].append(timed(lambda: run(lens), inner))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), inner=inner) for k, v in ms.items()}


res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup)

# ---- 1. the step
torch.manual_seed(1234)
model = Model(dim=DIM, depth=DEPTH, heads=HEADS, ragged_training=True).to(dev).train()
model.train_backend, model.train_precision = "hip", "mixed"
diffusion = NaturalSpeech2(model, codec=None, target_sample_hz=24000).to(dev)
g = torch.Generator().manual_seed(100)
latents, noise = torch.randn(B, N, DIM, generator=g).to(dev), torch.randn(B, N, DIM, generator=g).to(dev)
times = torch.rand(B, generator=g).to(dev)


def train_step(lens):
    for p in model.parameters():
        p.grad = None
    kw = {} if lens is None else dict(audio_lens=lens)
    diffusion(latents, times=times, noise=noise, **kw).backward()


res["step"] = dict(model=f"Model(dim={DIM}, depth={DEPTH}), train_precision='mixed'", batch=B, frames=N,
                   what="NaturalSpeech2.forward (+ audio_lens) and loss.backward(), eager",
                   lens_256_to_1024=[int(v) for v in arms["lens_256_to_1024"].tolist()], arms=measure(train_step, target_ms=300.))
del model, diffusion, latents, noise
torch.cuda.empty_cache()

# ---- 2. the twelve self-attention forward + backward pairs alone
bk = HipBackend(4)
A = HEADS * 64
M = B * N
qkv = ops.split(torch.randn(M, 3 * A, generator=g).to(dev), precision=3)            # q | k | v as the QKV GEMM leaves them (bf16 hi / lo)
do_row = ops.split(torch.randn(M, A, generator=g).to(dev), precision=3)
d_o = torch.randn(M, A, generator=g).to(dev)
vt = bk.transpose(qkv, 2 * A, A, N, per_batch=True)
g_row = bk.new_planes(M, 3 * A)


def attention_pairs(lens):
    kw = {} if lens is None else dict(lens=lens)
    for _ in range(DEPTH):
        o, lse = bk.attention(qkv, 0, qkv, A, vt, B, HEADS, N, N, **kw)
        delta = bk.attention_delta(d_o, o, B, HEADS, N)
        bk.attention_bwd(qkv, 0, qkv, A, qkv, 2 * A, do_row, lse, delta, B, HEADS, N, N, planes=(g_row, 0, A, 2 * A), **kw)


res["kernels"] = dict(what=f"{DEPTH} x (training forward + delta + backward, gradients as operand planes) of the self-attention, "
                           f"{B} x {HEADS} heads x {N} frames", arms=measure(attention_pairs, target_ms=100.))

out = {}
try:
    with open(args.out) as f:
        out = json.load(f)
except Exception:
    pass
out.update(res)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(res))
