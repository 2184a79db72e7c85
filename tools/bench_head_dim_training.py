"""What training at head dims 32 and 128 on the HIP kernels (`head_dim_training=True`, include/ns2hip_train.h) costs and saves on
one MI355X, and whether the head-dim-64 backward kept its speed:

    python tools/bench_head_dim_training.py [--out profiles/head_dim_training.json] [--repeats 7] [--warmup 2] [--parent-lib PATH]

1. `step`: warm forward + backward of Model(dim=512, depth=12) at 32 x 1024 frames with (dim_head, heads) = (32, 16), (64, 8), (128, 4) --
   the same inner width of 512 --, three arms: `hip_exact`, `hip_mixed` (train_precision) and `composite`, the PyTorch composite such a model
   trains on without the switch.  A repeat is one pair of device events around one forward + backward; after `warmup` untimed rounds,
   `repeats` rounds visit the three arms in turn (alternating); median and spread (min, max) of each are recorded.
2. `attention`: the attention forward (with lse) + delta + backward of ONE layer alone at 32 x heads x 1024 for the three head dims
   (gradients leaving as operand planes), same protocol, with the algorithmic TFLOP/s (14 B H N^2 D per pair).
3. `d64_vs_parent` (with --parent-lib: a libns2hip.so built from the parent commit): the attention backward of one layer at
   32 x 8 x 1024 x 64 on this library and on the parent's, one fresh process per repeat, alternating; the difference of the medians
   against the spread between repeats.

Keys of the output file other than those written here are kept.  Prints the result as one line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_dim_training.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--child-bwd64", action="store_true", help="internal: time the head-dim-64 backward on $NS2_LIB and print the median")
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()

from naturalspeech2_pytorch_amd import _lib                                                # noqa: E402
from naturalspeech2_pytorch_amd import Model, ops, autograd_path                           # noqa: E402
from naturalspeech2_pytorch_amd.training import HipBackend, model_forward_train           # noqa: E402

assert torch.cuda.is_available(), "bench_head_dim_training.py times HIP kernels: it needs the GPU"
dev = torch.device("cuda:0")
B, N, DIM, DEPTH = 32, 1024, 512, 12
SHAPES = ((32, 16), (64, 8), (128, 4))


def timed(fn, inner=1):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def stats(v, **kw):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), **kw)


def measure(arms, inner):
    """arms: {name: fn} -> {name: stats}; warm-up, then alternating rounds"""
    for _ in range(args.warmup):
        for fn in arms.values():
            timed(fn, inner)
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(timed(fn, inner))
    return {k: stats(v, inner=inner) for k, v in ms.items()}


def attention_operands(H, D, gen):
    A, M = H * D, B * N
    bk = HipBackend(4)
    qkv = ops.split(torch.randn(M, 3 * A, generator=gen).to(dev), precision=3)
    do_row = ops.split(torch.randn(M, A, generator=gen).to(dev), precision=3)
    d_o = torch.randn(M, A, generator=gen).to(dev)
    vt = bk.transpose(qkv, 2 * A, A, N, per_batch=True)
    return bk, A, qkv, do_row, d_o, vt, bk.new_planes(M, 3 * A)


if args.child_bwd64:
    bk, A, qkv, do_row, d_o, vt, g_row = attention_operands(8, 64, torch.Generator().manual_seed(100))
    o, lse = bk.attention(qkv, 0, qkv, A, vt, B, 8, N, N)
    delta = bk.attention_delta(d_o, o, B, 8, N)
    run = lambda: bk.attention_bwd(qkv, 0, qkv, A, qkv, 2 * A, do_row, lse, delta, B, 8, N, N, planes=(g_row, 0, A, 2 * A))      # noqa: E731
    for _ in range(3):
        timed(run, 20)
    print(json.dumps(dict(bwd64_ms=statistics.median(timed(run, 50) for _ in range(5)))))
    sys.exit(0)

res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup)
gen = torch.Generator().manual_seed(100)

# ---- 1. forward + backward of the model
if not args.skip_step:
    x = torch.randn(B, N, DIM, generator=gen).to(dev)
    cot = torch.randn(B, N, DIM, generator=gen).to(dev)
    times = torch.rand(B, generator=gen).to(dev)
    res["step"] = dict(model=f"Model(dim={DIM}, depth={DEPTH}, dim_head=D, heads=512 / D, head_dim_training=True)", batch=B, frames=N,
                       what="forward + backward of sum(pred * w), eager, warm", by_head_dim={})
    for D, H in SHAPES:
        torch.manual_seed(1234)
        model = Model(dim=DIM, depth=DEPTH, dim_head=D, heads=H, head_dim_training=True).to(dev).train()

        def step(fwd, tprec="exact"):
            model.train_precision = tprec
            for p in model.parameters():
                p.grad = None
            (fwd(model, x, times) * cot).sum().backward()

        arms = {"hip_exact": lambda: step(model_forward_train, "exact"), "hip_mixed": lambda: step(model_forward_train, "mixed"),
                "composite": lambda: step(autograd_path.model_forward_autograd)}
        r = measure(arms, 1)
        r["composite_over_hip_exact"] = round(r["composite"]["median_ms"] / r["hip_exact"]["median_ms"], 3)
        r["composite_over_hip_mixed"] = round(r["composite"]["median_ms"] / r["hip_mixed"]["median_ms"], 3)
        res["step"]["by_head_dim"][str(D)] = dict(heads=H, **r)
        del model
        torch.cuda.empty_cache()
    del x, cot

# ---- 2. the attention of one layer alone
res["attention"] = dict(what=f"one layer: training forward + delta + backward (gradients as operand planes), {B} x heads x {N}", by_head_dim={})
for D, H in SHAPES:
    bk, A, qkv, do_row, d_o, vt, g_row = attention_operands(H, D, gen)
    hd = {} if D == 64 else dict(head_dim=D)
    o, lse = bk.attention(qkv, 0, qkv, A, vt, B, H, N, N, **hd)
    delta = bk.attention_delta(d_o, o, B, H, N, **hd)
    arms = {"forward": lambda: bk.attention(qkv, 0, qkv, A, vt, B, H, N, N, **hd),
            "delta": lambda: bk.attention_delta(d_o, o, B, H, N, **hd),
            "backward": lambda: bk.attention_bwd(qkv, 0, qkv, A, qkv, 2 * A, do_row, lse, delta, B, H, N, N, planes=(g_row, 0, A, 2 * A), **hd)}
    r = measure(arms, 20)
    flop = B * H * N * N * float(D)
    r["forward_tflops"] = round(4 * flop / r["forward"]["median_ms"] / 1e9, 1)
    r["backward_tflops"] = round(10 * flop / r["backward"]["median_ms"] / 1e9, 1)
    res["attention"]["by_head_dim"][str(D)] = dict(heads=H, **r)
    del bk, qkv, do_row, d_o, vt, g_row, o, lse, delta
    torch.cuda.empty_cache()

# ---- 3. head dim 64 against the parent commit's library
if args.parent_lib:
    libs = {"this": _lib.LIB_PATH, "parent": os.path.abspath(args.parent_lib)}
    ms = {k: [] for k in libs}
    for _ in range(args.repeats):                           # alternating: a fresh process per library and repeat
        for k, path in libs.items():
            env = dict(os.environ, NS2_LIB=path)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bwd64"], env=env, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr[-2000:]
            ms[k].append(json.loads(out.stdout.strip().splitlines()[-1])["bwd64_ms"])
    r = {k: stats(v) for k, v in ms.items()}
    diff = r["this"]["median_ms"] - r["parent"]["median_ms"]
    spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in r)
    res["d64_vs_parent"] = dict(what="attention backward of one layer, 32 x 8 x 1024 x 64, gradients as operand planes; per repeat the median of "
                                     "5 x 50 launches in a fresh process", **r, difference_ms=round(diff, 4), spread_ms=round(spread, 4),
                                inside_spread=bool(abs(diff) <= spread))

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
