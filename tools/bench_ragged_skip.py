"""What skipping the hidden row tiles of a ragged sampling batch (Model(ragged_skip=True), include/ns2hip.h) costs and saves
on one MI355X:

    python tools/bench_ragged_skip.py [--out profiles/ragged_skip.json] [--repeats 7] [--warmup 3]

The d512 / L12 hybrid denoising step (model forward + DDIM update, eager) at 32 x 1024 frames, in the manner of
tools/bench_ragged_sampling.py: a repeat is one pair of device events around `inner` back-to-back steps (as many as fill about 200 ms),
divided by `inner`; after `warmup` untimed repeats, `repeats` rounds visit the arms in turn (alternating), and the median and the spread
(min, max) of each are recorded.  Arms: `lens=None`; lengths, switch off (the baseline of every comparison); switch on with all lengths
full; switch on with the lengths spread evenly over 256 ... 1024, once ascending and once shuffled; and the dim-128 model at 32 x 1024 with
the same spread, switch off and on.  `hidden_share` of an arm is COMPUTED, not measured: the share of 256-row tiles at or behind the
computed extents H_i = min(N, 256 ceil(lens_i / 256)) -- what the step can save at most.  The library's per-category kernel times
(ns2_model_profile_begin / _end) are taken with the switch off and on, in passes of their own.

`computed_extent` and `hidden_share` are importable without a GPU (tests/test_ragged_skip_cpu.py checks them against a restatement)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GRANULE = 256


def computed_extent(length, n):
    """H = min(n, 256 ceil(clamp(length, 1, n) / 256)): the rows of an utterance a skipping step computes"""
    length = min(max(int(length), 1), n)
    return min(n, -(-length // GRANULE) * GRANULE)


def hidden_share(lens, n):
    """the share of the batch's 256-row tiles that lie at or behind their utterance's computed extent (n % 256 == 0)"""
    assert n % GRANULE == 0 and len(lens) > 0
    return sum(n - computed_extent(l, n) for l in lens) / float(n * len(lens))


CATEGORIES = ["gemm_f32", "gemm_split", "gemm_qkv", "gemm_geglu", "gemm_wavenet", "attention", "rmsnorm", "gemm_ffconv"]


def main():
    import torch
    sys.path.insert(0, ROOT)
    from naturalspeech2_pytorch_amd import Model, _lib, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_skip.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ragged_skip.py times HIP kernels: it needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, N = 32, 1024
    spread = torch.linspace(256, N, B).round().to(torch.int32)
    shuffled = spread[torch.randperm(B, generator=torch.Generator().manual_seed(7))]
    t_cur, t_nxt = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.49, device=dev)

    def bench(dim, depth, arms):
        """arms: {name: (lens on the host or None, switch)} -> {name: figures}"""
        torch.manual_seed(1234)
        model = Model(dim=dim, depth=depth, precision="hybrid").to(dev).eval()
        x0 = torch.randn(B, N, dim, generator=torch.Generator().manual_seed(100)).to(dev)
        audio = x0.clone()
        on_dev = {k: (None if l is None else l.to(dev), sw) for k, (l, sw) in arms.items()}

        def step(lens, switch):
            model.ragged_skip = switch
            out = model(audio, t_cur, lens=lens)
            ops.ddim_step(audio, out, t_cur, t_nxt, "v", "sigmoid", 1., out=audio)

        def window(arm, inner):
            audio.copy_(x0)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                step(*on_dev[arm])
            end.record()
            end.synchronize()
            return start.elapsed_time(end) / inner

        def categories(arm, steps=3):
            h = model._ensure_native().handle
            out = {}
            for c, name in enumerate(CATEGORIES):
                ms, n = ctypes.c_double(0), ctypes.c_int64(0)
                audio.copy_(x0)
                torch.cuda.synchronize()
                _lib.check(lib.ns2_model_profile_begin(h, 1 << c), "ns2_model_profile_begin")
                for _ in range(steps):
                    step(*on_dev[arm])
                _lib.check(lib.ns2_model_profile_end(h, ctypes.byref(ms), ctypes.byref(n)), "ns2_model_profile_end")
                out[name] = dict(ms_per_step=round(ms.value / steps, 4), products_per_step=n.value // steps)
            return out

        res = {}
        with torch.no_grad():
            for arm in arms:
                window(arm, 1)
            inner = max(1, min(200, int(200. / max(window(next(iter(arms)), 2), 1e-3))))
            for _ in range(args.warmup):
                for arm in arms:
                    window(arm, inner)
            ms = {k: [] for k in arms}
            for _ in range(args.repeats):                      # alternating: every round visits every arm
                for arm in arms:
                    ms[arm].append(window(arm, inner))
            for arm, (lens, switch) in arms.items():
                res[arm] = dict(step_median_ms=round(statistics.median(ms[arm]), 4), step_min_ms=round(min(ms[arm]), 4),
                                step_max_ms=round(max(ms[arm]), 4), inner=inner, ragged_skip=switch,
                                skipping_step_ran=bool(lens is not None and switch and _ran(step, on_dev[arm], lib)),
                                hidden_share=0.0 if lens is None or not switch else round(hidden_share(lens.tolist(), N), 4),
                                lens=None if lens is None else [int(v) for v in lens.tolist()])
            prof = {arm: categories(arm) for arm in arms if arm in ("lens_spread_switch_off", "lens_spread_ascending_switch_on")}
        model.ragged_skip = False
        return res, prof

    def _ran(step, arm, lib):
        step(*arm)
        return int(lib.ns2_debug_skip_last()) == 1

    full = torch.full((B,), N, dtype=torch.int32)
    arms512 = {"lens_none": (None, False), "lens_spread_switch_off": (spread, False), "lens_full_switch_on": (full, True),
               "lens_spread_ascending_switch_on": (spread, True), "lens_spread_shuffled_switch_on": (shuffled, True)}
    arms128 = {"lens_spread_switch_off": (spread, False), "lens_spread_ascending_switch_on": (spread, True)}
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, batch=B, frames=N,
               what="model forward + DDIM update, eager; hybrid precision", baseline="lens_spread_switch_off")
    res["d512_L12"], res["d512_L12_categories"] = bench(512, 12, arms512)
    torch.cuda.empty_cache()
    res["d128_L12"], res["d128_L12_categories"] = bench(128, 12, arms128)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
