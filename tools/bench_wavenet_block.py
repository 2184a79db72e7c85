"""The lean Wavenet block kernel (csrc/wavenet3_kernel.h) at the headline shape: M = 32 x 1024 rows, d = 512, hybrid arithmetic, the
eight layers of a stack (dilations 1 ... 128).  The C ABI launches one layer at a time (the stack as grid-z exists only inside the
executor), so a "stack" here is eight launches of 256 workgroups back to back: the same 2048 workgroups, one per CU and round.
    python tools/bench_wavenet_block.py [--iters 20] [--rounds 5] [--gemm2]
    NS2_LIB=/path/to/an/experiment/libns2hip.so python tools/bench_wavenet_block.py      # experiment builds (one process per library)
Prints the median over the rounds of the time per stack and per layer, and one JSON line.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from naturalspeech2_pytorch_amd import ops, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--gemm2", action="store_true", help="also time gemm2_kernel<2, EPI_WAVENET, true, 1> (box drift check)")
ap.add_argument("--tag", default=os.path.basename(_lib.LIB_PATH))
args = ap.parse_args()
dev = torch.device("cuda:0")
B, N, d = 32, 1024, 512
M = B * N
DILS = [1 << i for i in range(8)]
g = torch.Generator().manual_seed(0)
rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
x = ops.split(rnd(M, d), precision=4)
layers = []
for dil in DILS:
    pw = ops.PackedWeight(rnd(d, d, 3, scale=(3 * d) ** -0.5), extra1x1=rnd(d, d, 1, scale=d ** -0.5), precision=4).tile_wavenet()
    layers.append((pw, dil, rnd(d), rnd(d), rnd(B, 2 * d)))
force = lambda k: _lib.check(_lib.load().ns2_debug_force_gemm(k))


def stack():
    for pw, dil, bc, br, film in layers:
        ops.wavenet_block(pw, x, N, dil, bc, br, film, precision=5)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3          # us


KS = (5, 2) if args.gemm2 else (5,)
res = {k: [] for k in KS}
for rd in range(args.rounds):
    for k in KS:
        force(k)
        res[k].append(timed(stack))
force(0)
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
flops = 2.0 * M * d * 4 * d * len(DILS)
print(f"{args.tag:28s} wavenet3 stack {med[5]:8.1f} us  = {med[5] / len(DILS):6.1f} us / layer = {med[5] / len(DILS):6.1f} us / workgroup "
      f"({flops / med[5] / 1e6:6.1f} TF)  min {min(res[5]):8.1f} max {max(res[5]):8.1f}"
      + (f"   gemm2 {med[2]:8.1f} us" if args.gemm2 else ""))
print(json.dumps(dict(tag=args.tag, lib=_lib.LIB_PATH, stack_us=round(med[5], 2), layer_us=round(med[5] / len(DILS), 2), rounds=[round(v, 2) for v in res[5]],
                      gemm2_stack_us=round(med[2], 2) if args.gemm2 else None)))
