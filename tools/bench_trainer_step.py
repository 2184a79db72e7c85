#!/usr/bin/env python
"""The optimizer step of the training loop (clip, Adam, EMA: NS2:1888-1901) on the HIP kernels of csrc/optim.hip (`training.HipAdam`) and on
PyTorch's kernels, ALTERNATING in one process.  A record, not a gate.

  chain  the chain alone over the parameters of the headline model, Model(dim=512, depth=12): 373 tensors, 260 425 464 values.
           hip / hip_ema      HipAdam.step(): norm + finish + update (32 bytes per value; + 8 on an EMA step)
           torch / torch_ema  clip_grad_norm_ + Adam(fused=True).step() (40 bytes per value: the norm reads g, the scaling reads and writes
                              it, fused Adam reads g, p, m, v and writes p, m, v) + torch._foreach_lerp_ on an EMA step (+ 12)
         achieved bytes per second by those counts, against 6.29 TB/s, a measured device-to-device copy rate of the MI355X (read + write bytes).
  step   the d512 / L12, 32 x 1024 frames, mixed-arithmetic training step: ONE graph with the optimizer inside
         (`GraphedTrainStep(optimizer=HipAdam)`) against the graph of loss + backward with clip_grad_norm_ + Adam(fused=True) + a foreach
         lerp every 10th step behind it (no overflow check on that path: it would add a host round trip).  EMA every 10th step on both.

A repeat = device events around `--iters` steps that end in a synchronise; warm-up steps first.  Writes profiles/trainer_step.json with every
repeat (the `tests` entry of an existing file, written by tests/test_trainer_step_gpu.py, is kept).

    python tools/bench_trainer_step.py [--repeats 7] [--iters 10] [--warmup 2] [--skip-step] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, training            # noqa: E402
from naturalspeech2_pytorch_amd.training import HipAdam                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_step.json"))
args = ap.parse_args()
assert args.repeats >= 5, "at least five repeats per path"

COPY_RATE = 6.29e12
DECAY = 0.995
dev = torch.device("cuda:0")


def timed(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(paths, iters):
    """paths: {name: fn}; alternating repeats, so drift hits every path alike"""
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            ms[k].append(timed(fn, iters))
    return {k: dict(ms=t, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for k, t in ms.items()}


def compare(case, ours, theirs):
    """our path counts as faster only when the gap exceeds the spread seen between repeats of the same path"""
    a, b = case[ours], case[theirs]
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return dict(gap_ms=b["median_ms"] - a["median_ms"], spread_ms=spread, hip_faster_beyond_spread=bool(b["median_ms"] - a["median_ms"] > spread),
                torch_over_hip_median=b["median_ms"] / a["median_ms"])


result = dict(device=torch.cuda.get_device_name(0), iters_per_repeat=args.iters, warmup=args.warmup, copy_rate_bytes_per_s=COPY_RATE)

# ------------------------------------------------------------------------------------------------------------------ the chain alone
torch.manual_seed(0)
shapes = [tuple(p.shape) for p in Model(dim=512, depth=12).parameters()]
values = sum(torch.Size(s).numel() for s in shapes)
grads = [1e-3 * torch.randn(s, device=dev) for s in shapes]                       # norm ~16: clipping is active


def make_params():
    torch.manual_seed(1)
    return [(0.1 * torch.randn(s, device=dev)).requires_grad_(True) for s in shapes]


p_hip, p_torch = make_params(), make_params()
hip = HipAdam(p_hip, lr=1e-4, max_grad_norm=1.0, ema=True, ema_decay=DECAY, ema_update_every=1)
hip.bind(p_hip, grads)
adam = torch.optim.Adam(p_torch, lr=1e-4, betas=(0.9, 0.99), fused=True)
ema_torch = [p.detach().clone() for p in p_torch]
g_torch = [g.clone() for g in grads]                                              # clip_grad_norm_ scales its gradients in place
for p, g in zip(p_torch, g_torch):
    p.grad = g


def hip_step(every):
    hip.ema_update_every = every
    hip.step()


def torch_step(ema):
    torch.nn.utils.clip_grad_norm_(p_torch, 1.0)
    adam.step()
    if ema:
        with torch.no_grad():
            torch._foreach_lerp_(ema_torch, [p.detach() for p in p_torch], 1.0 - DECAY)


chain = measure({"hip": lambda: hip_step(1 << 30), "torch": lambda: torch_step(False), "hip_ema": lambda: hip_step(1), "torch_ema": lambda: torch_step(True)},
                args.iters)
for k, nbytes in (("hip", 32), ("hip_ema", 40), ("torch", 40), ("torch_ema", 52)):
    rate = nbytes * values / (chain[k]["median_ms"] * 1e-3)
    chain[k].update(bytes_per_value=nbytes, bytes_per_s=rate, frac_of_copy_rate=rate / COPY_RATE)
chain.update(tensors=len(shapes), values=values, ordinary=compare(chain, "hip", "torch"), ema_step=compare(chain, "hip_ema", "torch_ema"))
assert int(hip.skipped) == 0
result["chain"] = chain
print("chain", json.dumps({k: (round(v["median_ms"], 3), round(v["frac_of_copy_rate"], 3)) for k, v in chain.items() if isinstance(v, dict) and "ms" in v}),
      json.dumps(dict(ordinary=chain["ordinary"], ema_step=chain["ema_step"])), flush=True)
del p_hip, p_torch, hip, adam, ema_torch, g_torch, grads
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------------------------ the whole step
if not args.skip_step:
    B, N, D = 32, 1024, 512
    g = torch.Generator().manual_seed(1)
    audio, times, noise = torch.randn(B, N, D, generator=g).to(dev), torch.rand(B, generator=g).to(dev), torch.randn(B, N, D, generator=g).to(dev)

    def build(with_opt):
        torch.manual_seed(0)
        m = Model(dim=D, depth=12).to(dev).train()
        m.train_backend, m.train_precision = "hip", "mixed"
        d = NaturalSpeech2(m, codec=None, target_sample_hz=24000).to(dev)
        opt = HipAdam(m.parameters(), lr=1e-4, max_grad_norm=1.0, ema=True, ema_decay=DECAY, ema_update_every=10) if with_opt else None
        gs = training.GraphedTrainStep(lambda a, t, z: d(a, times=t, noise=z), (audio, times, noise), m, optimizer=opt)
        return m, d, opt, gs

    m1, d1, opt1, gs1 = build(True)
    m2, d2, _, gs2 = build(False)
    adam2 = torch.optim.Adam(m2.parameters(), lr=1e-4, betas=(0.9, 0.99), fused=True)
    ema2 = [p.detach().clone() for p in m2.parameters()]
    count = [0]

    def torch_path():
        gs2(audio, times, noise)
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
        adam2.step()
        count[0] += 1
        if count[0] % 10 == 0:
            with torch.no_grad():
                torch._foreach_lerp_(ema2, [p.detach() for p in m2.parameters()], 1.0 - DECAY)

    step = measure({"hip_one_graph": lambda: gs1(audio, times, noise), "graph_then_torch_chain": torch_path}, 10)
    step.update(compare(step, "hip_one_graph", "graph_then_torch_chain"), batch=B, frames=N, dim=D, depth=12, train_precision="mixed",
                hip_steps_taken=int(opt1.steps_taken), hip_last_skipped=int(opt1.skipped), hip_loss=float(gs1.loss), torch_chain_loss=float(gs2.loss))
    result["step"] = step
    print("step", json.dumps({k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in step.items()}), flush=True)

for path in (os.path.join(ROOT, "profiles", "trainer_step.json"), args.out):      # keep what the GPU tests recorded
    try:
        with open(path) as f:
            old = json.load(f)
        if "tests" in old:
            result.setdefault("tests", {}).update(old["tests"])
    except Exception:
        pass
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
print("wrote", args.out)
