"""Step wall time against the sum of kernel durations from a `rocprofv3 --kernel-trace` CSV of `bench.py`, and how much of the
kernel time overlapped (two utterance chains).

    rocprofv3 --kernel-trace --stats -d DIR -- python bench.py --steps 10 --warmup 3
    python tools/chains_trace.py DIR/*/*_kernel_trace.csv

A step ends with its ddim_kernel; the steps between the first and the last ddim_kernel of the trace are measured (the first step
carries the set-up).  wall = first-to-last ddim end / steps; sum = every kernel's duration; busy = the union of the kernels'
intervals; overlap = sum - busy.  Under concurrency a kernel's duration is not comparable with its duration alone.
"""
import csv
import json
import sys


def analyse(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Stream_Id") or r.get("Queue_Id")))
    rows.sort()
    ends = [e for s, e, n, q in rows if "ddim_kernel" in n]
    if len(ends) < 3:
        raise SystemExit("fewer than 3 ddim_kernel launches in the trace")
    t0, t1, steps = ends[0], ends[-1], len(ends) - 1
    win = [(s, e, n, q) for s, e, n, q in rows if s >= t0 and e <= t1]
    total = sum(e - s for s, e, n, q in win)
    busy, cur_s, cur_e = 0, None, None
    for s, e, n, q in win:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += (cur_e - cur_s) if cur_e is not None else 0
    ms = lambda ns: round(ns / steps / 1e6, 4)  # noqa: E731
    return {"steps": steps, "kernels_per_step": round(len(win) / steps, 1), "streams": len({q for s, e, n, q in win}),
            "wall_ms_per_step": ms(t1 - t0), "kernel_sum_ms_per_step": ms(total), "busy_ms_per_step": ms(busy),
            "overlap_ms_per_step": ms(total - busy), "idle_ms_per_step": ms((t1 - t0) - busy)}


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(json.dumps({"trace": p, **analyse(p)}))
