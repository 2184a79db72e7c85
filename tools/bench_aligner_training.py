#!/usr/bin/env python
"""A warm training pass (forward + backward) of the Aligner with its forward-sum and bin losses at the reference's default sizes --
Aligner(dim_in=80, dim_hidden=512, attn_channels=80) -- on 32 utterances of 256 phonemes and 1024 mel frames (ragged lengths), on the HIP
training path (`train_backend="hip"`, both losses `backend="hip"`, lengths on the device) and on the PyTorch composite (masks, torch's
CTCLoss), ALTERNATING in one process.  A repeat = device events around `--iters` passes that end in a synchronise; warm-up passes first.
The composite is untouched by the HIP path, so its time is the time without the feature.  Also timed on their own: the two new kernels
groups, ns2_align_attn_bwd and ns2_align_losses_fwd + _bwd (both losses), at the same sizes.  Writes profiles/aligner_training.json with
every repeat.

    python tools/bench_aligner_training.py [--repeats 7] [--iters 3] [--warmup 2] [--only hip|composite] [--out PATH]

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

from naturalspeech2_pytorch_amd import training                                   # noqa: E402
from naturalspeech2_pytorch_amd.aligner import Aligner, BinLoss, ForwardSumLoss, create_mask   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None, choices=("hip", "composite"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_training.json"))
args = ap.parse_args()
assert args.repeats >= 5 or args.only, "at least five repeats per path"

B, N, T = 32, 256, 1024
dev = torch.device("cuda:0")
torch.manual_seed(0)
aligner = Aligner(dim_in=80, dim_hidden=512, attn_channels=80).to(dev).train()
x = torch.randn(B, N, 512).to(dev).requires_grad_(True)
mel = torch.randn(B, 80, T).to(dev)
g = torch.Generator().manual_seed(1)
text_lens = torch.randint(N // 2, N + 1, (B,), generator=g)
mel_lens = torch.randint(T // 2, T + 1, (B,), generator=g)
text_lens[0], mel_lens[0] = N, T
text_lens, mel_lens = text_lens.to(dev), mel_lens.to(dev)
x_mask, y_mask = create_mask(text_lens, N)[:, None], create_mask(mel_lens, T)[:, None]
losses = {b: (ForwardSumLoss(backend=b), BinLoss(backend=b)) for b in ("hip", "composite")}


def one_pass(backend):
    aligner.train_backend = backend
    for p in aligner.parameters():
        p.grad = None
    x.grad = None
    if backend == "hip":                                                          # lengths straight through: no masks, no host read
        hard, soft, logp, path = aligner.forward_lengths_train(x, text_lens, mel, mel_lens)
    else:
        hard, soft, logp, path = aligner(x, x_mask, mel, y_mask)
    fs, bn = losses[backend]
    (fs(logp, text_lens, mel_lens) + bn(path, logp, text_lens)).backward()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


def summary(t):
    return dict(ms=t, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


result = dict(batch=B, phonemes=N, frames=T, dims=dict(dim_in=80, dim_hidden=512, attn_channels=80), iters_per_repeat=args.iters,
              warmup=args.warmup, device=torch.cuda.get_device_name(0))
backends = [args.only] if args.only else ["hip", "composite"]
times = {b: [] for b in backends}
for b in backends:
    for _ in range(args.warmup):
        one_pass(b)
torch.cuda.synchronize()
for _ in range(args.repeats):
    for b in backends:                                                            # alternating: drift hits both paths alike
        times[b].append(timed(lambda: one_pass(b)))
case = {b: summary(t) for b, t in times.items()}
if len(backends) == 2:
    h, c = case["hip"], case["composite"]
    case["composite_over_hip_median"] = c["median_ms"] / h["median_ms"]
    # the HIP path counts as faster only when the gap exceeds the spread seen between repeats of the same path
    spread = max(h["max_ms"] - h["min_ms"], c["max_ms"] - c["min_ms"])
    case["gap_ms"], case["spread_ms"] = c["median_ms"] - h["median_ms"], spread
    case["hip_faster_beyond_spread"] = bool(c["median_ms"] - h["median_ms"] > spread)
result["pass"] = case
print("pass", json.dumps({k: v for k, v in case.items() if not isinstance(v, dict)}), {b: [round(v, 2) for v in times[b]] for b in backends}, flush=True)

if args.only != "composite":                                                      # the two new kernel groups on their own
    bk = training.HipBackend(3)
    tl, ml = text_lens.int(), mel_lens.int()
    with torch.no_grad():
        hard, soft, logp, path = aligner.forward_lengths(x.detach(), tl, mel, ml)
    q, k = torch.randn(B * T, 80, device=dev), torch.randn(B * N, 80, device=dev)
    log2, soft2 = bk.align_attn(q, k, tl, B)
    g_log, g_soft = torch.randn_like(log2), torch.randn_like(soft2)
    one = torch.ones(1, device=dev)

    def losses_pair():
        fs, bn, ws = bk.align_losses_fwd(logp, tl, ml, -1., hard=path, want_fs=True, want_bin=True)
        bk.align_losses_bwd(logp, tl, ml, -1., ws, hard=path, g_fs=one, g_bin=one)

    kern = {"ns2_align_attn_bwd": lambda: bk.align_attn_bwd(q, k, log2, soft2, g_log, g_soft, tl),
            "ns2_align_losses_fwd": lambda: bk.align_losses_fwd(logp, tl, ml, -1., hard=path, want_fs=True, want_bin=True),
            "ns2_align_losses_fwd+bwd": losses_pair}
    result["kernels"] = {}
    for name, fn in kern.items():
        for _ in range(args.warmup):
            fn()
        result["kernels"][name] = summary([timed(fn) for _ in range(max(args.repeats, 5))])
        print(name, round(result["kernels"][name]["median_ms"], 3), "ms", flush=True)

if not args.only:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)
