"""Wall time of the Aligner pieces of forward(text=...) on one MI355X, HIP against the PyTorch composite (profiles/r08_*):

    python tools/bench_alignment.py [--iters 10] [--mode both|hip|composite] [--T 1024]

B = 32 utterances, 256 phonemes, T mel frames.  `search`: the alignment search alone on one soft alignment [B, 256, T]
(ns2_maximum_path against autograd_path.maximum_path_composite); `front_end`: the Aligner forward from phoneme encodings and
mel to the hard path (HIP path against the composite Aligner with the composite search) plus average_over_durations and the
expansion into cond; `train_step`: a d512 / L12 text-conditioned forward + backward at B x T (HIP front end; the composite
front end for the other side).  Run under `rocprofv3 --kernel-trace --stats` for kernel times.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, ops                   # noqa: E402
from naturalspeech2_pytorch_amd import autograd_path as AP                            # noqa: E402
from naturalspeech2_pytorch_amd.aligner import Aligner, average_over_durations, create_mask, expand_encodings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--mode", default="both", choices=("both", "hip", "composite"))
ap.add_argument("--T", type=int, default=1024)
ap.add_argument("--no-train", action="store_true")
args = ap.parse_args()

B, N_PH, T = 32, 256, args.T
dev = torch.device("cuda:0")
torch.manual_seed(0)
g = torch.Generator().manual_seed(1)
tl = torch.randint(N_PH // 2, N_PH + 1, (B,), generator=g).to(dev)
ml = torch.randint(T // 2, T + 1, (B,), generator=g).to(dev)
tl[0], ml[0] = N_PH, T
mask = (create_mask(tl, N_PH)[:, :, None] & create_mask(ml, T)[:, None]).float()
soft = torch.rand(B, N_PH, T, generator=g).softmax(1).to(dev)
al = Aligner(dim_in=80, dim_hidden=512).to(dev).eval()
x = torch.randn(B, N_PH, 512, generator=g).to(dev)
mel = torch.randn(B, 80, T, generator=g).to(dev)
pitch = (80 + 300 * torch.rand(B, 1, T, generator=g)).to(dev)
table = torch.randn(256, 512, generator=g).to(dev)


def front(hip):
    if hip:
        hard, _, _, path = al.forward_lengths(x, tl, mel, ml)
    else:
        hard, _, _, path = al._forward_composite(x, create_mask(tl, N_PH)[:, None], mel, create_mask(ml, T)[:, None])
        # the composite search on the GPU is the same PyTorch loop as on the CPU
    p = average_over_durations(pitch, hard) if hip else AP.average_over_durations_composite(pitch, hard)
    return expand_encodings(x, hard, path, p[:, 0], table) if hip else AP.expand_with_path(x, path, p[:, 0], table)


def timed(fn, iters):
    with torch.no_grad():
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, out


# the composite front end must not reach ns2_maximum_path: patch the public search to the loop for that side
import naturalspeech2_pytorch_amd.aligner as AL                                      # noqa: E402
hip_search = AL.maximum_path
res = dict(B=B, n_ph=N_PH, T=T, iters=args.iters)
outs = {}
for name in ("hip", "composite"):
    if args.mode not in ("both", name):
        continue
    it = args.iters if name == "hip" else max(1, args.iters // 5)
    if name == "hip":
        ms, outs["search_hip"] = timed(lambda: ops.maximum_path(soft, tl, ml)[0], it)
        res["search_hip_wall_ms"] = round(ms, 3)
        AL.maximum_path = hip_search
    else:
        ms, outs["search_composite"] = timed(lambda: AP.maximum_path_composite(soft, mask), it)
        res["search_composite_wall_ms"] = round(ms, 3)
        AL.maximum_path = lambda v, m, const=None: AP.maximum_path_composite(v, m, const)
    ms, outs[f"front_{name}"] = timed(lambda: front(name == "hip"), it)
    res[f"front_end_{name}_wall_ms"] = round(ms, 3)
AL.maximum_path = hip_search
if args.mode == "both":
    res["search_paths_equal"] = bool(torch.equal(outs["search_hip"], outs["search_composite"]))
    res["search_ratio_composite_over_hip"] = round(res["search_composite_wall_ms"] / res["search_hip_wall_ms"], 1)
    res["front_end_ratio_composite_over_hip"] = round(res["front_end_composite_wall_ms"] / res["front_end_hip_wall_ms"], 2)
    res["front_end_cond_max_abs_diff"] = float((outs["front_hip"] - outs["front_composite"]).abs().max())

if not args.no_train:
    d = NaturalSpeech2(Model(dim=512, depth=12, dim_prompt=512, condition_on_prompt=True, cond_drop_prob=0.), codec=None,
                       target_sample_hz=24000, build_aligner=True).to(dev).train()
    d.phoneme_enc.eval()
    text = torch.randint(0, 150, (B, N_PH), generator=g).to(dev)
    audio = torch.randn(B, T, 512, generator=g).to(dev)
    p_enc = torch.randn(B, 64, 512, generator=g).to(dev)

    def step():
        d.zero_grad(set_to_none=True)
        d(audio, text=text, text_lens=tl, mel=mel, mel_lens=ml, pitch=pitch, prompt_enc=p_enc).backward()

    for name in ("hip", "composite"):
        if args.mode not in ("both", name):
            continue
        AL.maximum_path = hip_search if name == "hip" else (lambda v, m, const=None: AP.maximum_path_composite(v, m, const))
        orig = d.aligner.forward_lengths
        if name == "composite":
            d.aligner.forward_lengths = lambda x_, tl_, y_, ml_: d.aligner._forward_composite(
                x_, create_mask(tl_, x_.shape[1])[:, None], y_, create_mask(ml_, y_.shape[-1])[:, None])
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_it = max(1, args.iters // 2)
        for _ in range(n_it):
            step()
        torch.cuda.synchronize()
        res[f"train_step_{name}_wall_ms"] = round((time.perf_counter() - t0) * 1e3 / n_it, 3)
        d.aligner.forward_lengths = orig
    AL.maximum_path = hip_search
print(json.dumps(res))
