"""A/B of the two utterance chains: `python bench.py` of a parent checkout against this tree with libraries
built at each chain skew, alternating in fresh processes on one MI355X, then `--dump-outputs` identity for hybrid and exact.

    # the four skew builds: csrc/model_exec.cpp compiled with -DNS2_CHAIN_SKEW=0 ... 3, linked like csrc/build.sh
    python tools/chains_ab.py --parent DIR_OF_BUILT_PARENT_CHECKOUT --lib skew0=PATH --lib skew1=PATH ... [--rounds 3] [--full]
    # a later A/B with switches read from the environment (profiles/tail_fold_norm_ab.json): this tree's library under each setting
    python tools/chains_ab.py --parent DIR --no-one-chain --side norm_old:NS2_NORM=1 --side both_off:NS2_NORM=1,NS2_TAIL_FOLD=0

Prints one JSON line per run (`ms_per_step`; with --full also the three side workloads the chains may touch) and one per identity check.
Every run has its own time limit; the first abnormal exit ends the job (nothing more is started on the GPU).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = ("d128_config2", "conditioned_config3", "small_batch")
T0 = time.time()


def emit(**kw):
    kw["t"] = round(time.time() - T0, 1)
    print(json.dumps(kw), flush=True)


def bench(tag, cwd, env_extra, args=(), limit=600):
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py", *args], cwd=cwd, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True)
    res = None
    for ln in r.stdout.splitlines():
        if ln.startswith("{") and "ms_per_step" in ln:
            res = json.loads(ln)
    out = dict(tag=tag, rc=r.returncode, wall=round(time.time() - t, 1), ms_per_step=(res or {}).get("ms_per_step"), args=list(args))
    if res and res.get("side"):
        out["side"] = {k: res["side"].get(k) for k in SIDE_KEYS}
    emit(**out)
    if r.returncode != 0 or res is None:
        emit(tag=tag, stderr=r.stderr[-1500:])
        sys.exit(3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit with its library built")
    ap.add_argument("--lib", action="append", default=[], metavar="TAG=PATH", help="a library of this tree to run through NS2_LIB")
    ap.add_argument("--side", action="append", default=[], metavar="TAG:K=V[,K=V]", help="one more side: this tree's first library with these environment variables")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="run bench.py --full (side workloads) instead of the plain headline")
    ap.add_argument("--no-dump", action="store_true")
    ap.add_argument("--no-one-chain", action="store_true", help="skip the runs of this tree forced to one chain (NS2_CHAINS=1)")
    a = ap.parse_args()
    libs = [s.split("=", 1) for s in a.lib] or [["new", os.path.join(ROOT, "naturalspeech2_pytorch_amd", "libns2hip.so")]]
    sides = [("parent", a.parent, {})] + [(t, ROOT, {"NS2_LIB": os.path.abspath(p)}) for t, p in libs]
    for spec in a.side:
        tag, _, kv = spec.partition(":")
        sides.append((tag, ROOT, dict({"NS2_LIB": os.path.abspath(libs[0][1])}, **dict(p.split("=", 1) for p in kv.split(",") if p))))
    if not a.no_one_chain:
        sides.append(("new_one_chain", ROOT, {"NS2_LIB": os.path.abspath(libs[0][1]), "NS2_CHAINS": "1"}))
    for _ in range(a.rounds):
        for tag, cwd, env in sides:
            bench(tag, cwd, env, args=("--full", "--no-cpu-baseline", "--no-parity", "--no-secondary") if a.full else ())
    if a.no_dump or a.full:
        return
    for prec in ("hybrid", "exact"):
        sums = {}
        for tag, cwd, env in sides[:2]:
            with tempfile.TemporaryDirectory() as d:
                bench(f"dump_{tag}_{prec}", cwd, env, args=("--precision", prec, "--steps", "4", "--warmup", "1", "--dump-outputs", d))
                sums[tag] = {f: [hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest()[:16], os.path.getsize(os.path.join(d, f))]
                             for f in sorted(os.listdir(d))}
        emit(tag="dump_compare", precision=prec, sums=sums, identical=sums[sides[0][0]] == sums[sides[1][0]])


if __name__ == "__main__":
    main()
