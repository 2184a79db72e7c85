"""What skipping the hidden row tiles of a ragged TRAINING batch (Model(ragged_skip_training=True), include/ns2hip_train.h)
costs and saves on one MI355X:

    python tools/bench_ragged_skip_training.py [--out profiles/ragged_skip_training.json] [--repeats 7] [--warmup 2]

1. `step`: the d512 / L12 model at 32 x 1024 frames, train_precision="mixed", one eager loss + backward (NaturalSpeech2.forward with
   audio_lens and loss.backward()), in the manner of tools/bench_ragged_training.py: a repeat is one pair of device events around `inner`
   back-to-back steps, divided by `inner`; after `warmup` untimed repeats, `repeats` rounds visit the arms in turn (alternating), and the
   median and the spread (min, max) of each are recorded.  Arms: `lens_none`; `lens_spread_switch_off` -- lengths spread evenly over
   256 ... 1024, the switch off: the baseline of every comparison; the switch on with that spread ascending, with it shuffled, and with
   all lengths full.  `hidden_share` is COMPUTED, not measured: the share of 256-row tiles at or behind the computed extents
   H_i = min(N, 256 ceil(lens_i / 256)) -- what the products can save at most.  `saving_counts` says whether the median saving against
   the baseline exceeds the spread between the repeats of either arm.
2. `categories`: per-category sums of kernel time for the baseline and the ascending arm, from one pass each in which every backend
   call sits between a pair of device events (a pass of its own: the events serialise nothing, but they are not in the timed arms):
   forward products, dgrads, weight gradients, attention, and the row-local kernels that do not skip.

`hidden_share` is importable without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GRANULE = 256


def computed_extent(length, n):
    length = min(max(int(length), 1), n)
    return min(n, -(-length // GRANULE) * GRANULE)


def hidden_share(lens, n):
    """the share of the batch's 256-row tiles at or behind their utterance's computed extent (n % 256 == 0)"""
    assert n % GRANULE == 0 and len(lens) > 0
    return sum(n - computed_extent(l, n) for l in lens) / float(n * len(lens))


class TimedBackend:
    """every call of the wrapped HipBackend between two device events, filed under forward products / dgrads / weight gradients / attention /
    row-local by the call and, for a product, by the pack it multiplies (the forward packs are keyed "f" and "qkv", the dgrad packs "b" and
    "qkv_b": functions.py)"""
    PRODUCTS = ("gemm_f32", "gemm_split")

    def __init__(self, inner, torch):
        self._bk, self._torch, self._pairs, self._kind = inner, torch, [], {}
        self.packs = inner.packs

    def pack(self, key, *a, **kw):
        pw = self._bk.pack(key, *a, **kw)
        self._kind[id(pw)] = "dgrad" if str(key[0]).endswith("b") else "forward_products"
        return pw

    def __getattr__(self, name):
        fn = getattr(self._bk, name)
        if not callable(fn):
            return fn

        def timed(*a, **kw):
            if name in self.PRODUCTS:
                cat = self._kind.get(id(a[0]), "forward_products")
            elif name.startswith("wgrad") and name != "wgrad_rows_ok":
                cat = "weight_gradients"
            elif name.startswith("attention"):
                cat = "attention"
            elif name in ("wgrad_rows_ok",):
                return fn(*a, **kw)
            else:
                cat = "row_local"
            s, e = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **kw)
            e.record()
            self._pairs.append((cat, s, e))
            return out
        return timed

    def sums(self):
        self._torch.cuda.synchronize()
        out = {}
        for cat, s, e in self._pairs:
            d = out.setdefault(cat, dict(ms=0.0, calls=0))
            d["ms"] += s.elapsed_time(e)
            d["calls"] += 1
        self._pairs = []
        return {k: dict(ms=round(v["ms"], 3), calls=v["calls"]) for k, v in sorted(out.items())}


def main():
    import torch
    sys.path.insert(0, ROOT)
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, _lib, training
    from naturalspeech2_pytorch_amd.training import HipBackend

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_skip_training.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--depth", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ragged_skip_training.py times HIP kernels: it needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, N, DIM, DEPTH = 32, 1024, args.dim, args.depth
    spread = torch.linspace(256, N, B).round().to(torch.int32)
    shuffled = spread[torch.randperm(B, generator=torch.Generator().manual_seed(7))]
    full = torch.full((B,), N, dtype=torch.int32)
    arms = {"lens_none": (None, False), "lens_spread_switch_off": (spread, False), "lens_spread_ascending_switch_on": (spread, True),
            "lens_spread_shuffled_switch_on": (shuffled, True), "lens_full_switch_on": (full, True)}
    on_dev = {k: (None if l is None else l.to(dev), sw) for k, (l, sw) in arms.items()}

    torch.manual_seed(1234)
    model = Model(dim=DIM, depth=DEPTH, ragged_training=True).to(dev).train()
    model.train_backend, model.train_precision = "hip", "mixed"
    diffusion = NaturalSpeech2(model, codec=None, target_sample_hz=24000).to(dev)
    g = torch.Generator().manual_seed(100)
    latents, noise = torch.randn(B, N, DIM, generator=g).to(dev), torch.randn(B, N, DIM, generator=g).to(dev)
    times = torch.rand(B, generator=g).to(dev)

    def step(lens, switch):
        model.ragged_skip_training = switch
        for p in model.parameters():
            p.grad = None
        kw = {} if lens is None else dict(audio_lens=lens)
        diffusion(latents, times=times, noise=noise, **kw).backward()

    def window(arm, inner):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            step(*on_dev[arm])
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / inner

    for arm in arms:
        window(arm, 1)
    inner = max(1, min(50, int(300. / max(window("lens_none", 2), 1e-3))))
    for _ in range(args.warmup):
        for arm in arms:
            window(arm, inner)
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):                              # alternating: every round visits every arm
        for arm in arms:
            ms[arm].append(window(arm, inner))
    res_arms = {}
    for arm, (lens, switch) in arms.items():
        n0 = int(lib.ns2_debug_train_skip_launches())
        step(*on_dev[arm])
        res_arms[arm] = dict(median_ms=round(statistics.median(ms[arm]), 4), min_ms=round(min(ms[arm]), 4), max_ms=round(max(ms[arm]), 4),
                             inner=inner, ragged_skip_training=switch, launches_with_lengths=int(lib.ns2_debug_train_skip_launches()) - n0,
                             hidden_share=0.0 if lens is None or not switch else round(hidden_share(lens.tolist(), N), 4),
                             lens=None if lens is None else [int(v) for v in lens.tolist()])
    base = res_arms["lens_spread_switch_off"]
    for arm, r in res_arms.items():
        ref = res_arms["lens_none"] if arm == "lens_full_switch_on" else base
        r["against"] = "lens_none" if arm == "lens_full_switch_on" else "lens_spread_switch_off"
        r["saving_ms"] = round(ref["median_ms"] - r["median_ms"], 4)
        r["saving_percent"] = round(100. * (ref["median_ms"] - r["median_ms"]) / ref["median_ms"], 2)
        spread_ms = max(ref["max_ms"] - ref["min_ms"], r["max_ms"] - r["min_ms"])
        r["saving_counts"] = bool(abs(r["saving_ms"]) > spread_ms)

    # ---- per-category kernel-time sums, in passes of their own
    cats = {}
    for arm in ("lens_spread_switch_off", "lens_spread_ascending_switch_on"):
        tb = TimedBackend(HipBackend(4), torch)
        prev = training.set_backend(tb)
        try:
            step(*on_dev[arm])                                 # (packs its weights)
            tb.sums()
            step(*on_dev[arm])
            cats[arm] = tb.sums()
        finally:
            training.set_backend(prev)
    model.ragged_skip_training = False
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, batch=B, frames=N,
               model=f"Model(dim={DIM}, depth={DEPTH}), train_precision='mixed'",
               what="NaturalSpeech2.forward (+ audio_lens) and loss.backward(), eager", baseline="lens_spread_switch_off",
               hidden_share_bound=round(hidden_share(spread.tolist(), N), 4), step=res_arms, categories=cats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
