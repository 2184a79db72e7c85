#!/usr/bin/env python
"""Self-attention micro-benchmark at the headline shape (B=32, H=8, N=1024, d_head=64): ms per launch and algorithmic TFLOP/s
per precision, plus the relative error against an fp64 softmax(QK^T/8)V.  NS2_LIB selects an experiment build (same-box A/B).

--ab: attn_kernel against attn_fast_kernel (csrc/attn_fast_kernel.h) inside one process at precisions 2 and 4: the switch
ns2_debug_force_attention alternates 1, 0, 1, 0, ... over 15 rounds of 20 launches each after a warm-up of 1000 launches per kernel; prints per precision the
median ms of each kernel, every round's pair, new / old, and whether the two packed outputs are bitwise equal."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from naturalspeech2_pytorch_amd import ops

dev = torch.device("cuda:0")
B, H, N = 32, 8, 1024
g = torch.Generator().manual_seed(3)
q = torch.randn(B * N, H * 64, generator=g)
k = torch.randn(B * N, H * 64, generator=g)
v = torch.randn(B * N, H * 64, generator=g)


def ab(rounds=15, warm=40):
    from naturalspeech2_pytorch_amd import _lib
    lib = _lib.load()
    res = {}
    try:
        for prec in (2, 4):
            qp, kp = ops.split(q.to(dev), precision=2), ops.split(k.to(dev), precision=2)
            vtp = ops.split(v.reshape(B, N, H * 64).transpose(1, 2).reshape(B * H * 64, N).contiguous().to(dev), precision=2)
            outs, ms = {}, {1: [], 0: []}
            for _ in range(warm):                         # ~2000 launches: the clock has settled before the first timed round
                for sw in (1, 0):
                    _lib.check(lib.ns2_debug_force_attention(sw))
                    for _ in range(25):
                        outs[sw] = ops.attention(qp, kp, vtp, B, H, N, N, precision=prec)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for sw in (1, 0):
                    _lib.check(lib.ns2_debug_force_attention(sw))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        ops.attention(qp, kp, vtp, B, H, N, N, precision=prec)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[sw].append(round(e0.elapsed_time(e1) / 20, 4))
            old, new = sorted(ms[1])[rounds // 2], sorted(ms[0])[rounds // 2]
            tf = lambda t: round(4.0 * B * H * N * N * 64 / 1e9 / t, 1)
            res[str(prec)] = dict(old_ms=old, new_ms=new, ratio=round(new / old, 4), old_tflops=tf(old), new_tflops=tf(new),
                                  rounds_old_new=list(zip(ms[1], ms[0])), bitwise_equal=bool(torch.equal(outs[0].buf, outs[1].buf)))
    finally:
        lib.ns2_debug_force_attention(0)
    print(json.dumps(dict(ab="attn_kernel (old) vs attn_fast_kernel (new)", shape=[B, H, N, 64], **res)))


if "--ab" in sys.argv[1:]:
    ab()
    sys.exit(0)

out = {}
for prec in (4, 2, 3):
    attp = 2 if prec == 4 else prec                       # attention operands are IEEE half at precision 4
    qp, kp = ops.split(q.to(dev), precision=attp), ops.split(k.to(dev), precision=attp)
    vt = v.reshape(B, N, H * 64).transpose(1, 2).reshape(B * H * 64, N).contiguous()
    vtp = ops.split(vt.to(dev), precision=attp)
    for _ in range(3):
        o = ops.attention(qp, kp, vtp, B, H, N, N, precision=prec)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        o = ops.attention(qp, kp, vtp, B, H, N, N, precision=prec)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    of = ops.join(o, H * 64)[:N].double().cpu()       # utterance 0
    qd, kd, vd = (t[:N].double().reshape(N, H, 64).transpose(0, 1) for t in (q, k, v))
    ref = (torch.softmax(qd @ kd.transpose(1, 2) / 8.0, dim=-1) @ vd).transpose(0, 1).reshape(N, H * 64)
    out[str(prec)] = dict(ms=round(ms, 4), tflops=round(4.0 * B * H * N * N * 64 / 1e9 / ms, 1),
                          rel_err=float(((of - ref).norm() / ref.norm()).item()))
print(json.dumps(dict(lib=os.environ.get("NS2_LIB", "default"), **out)))
