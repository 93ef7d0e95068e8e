#!/usr/bin/env python3
"""Mean +- standard deviation of every kernel over the last two thirds of its launches in two rocprofv3 kernel traces
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR ...` of the same bench.py command on two commits):

  python tools/kernel_spread.py PARENT_TRACE_DIR NEW_TRACE_DIR

One line per kernel, ordered by the parent's time (profiles/r08_darcy8_kernel_spread.txt).  A kernel whose template arguments
changed is matched by the rename in `key`."""
import csv, glob, math, os, sys
def load(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in f for r in csv.DictReader(open(p))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        by.setdefault(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for k, v in by.items():
        v = v[len(v) // 3:]
        m = sum(v) / len(v)
        sd = math.sqrt(sum((x - m) ** 2 for x in v) / (len(v) - 1)) if len(v) > 1 else 0.0
        out[k] = (m, sd, len(v))
    return out
a, b = load(sys.argv[1]), load(sys.argv[2])
def key(k): return k.replace("<2, true, true>", "<2, true>")
bb = {key(k): (k, v) for k, v in b.items()}
print(f"{'kernel':70s} {'parent us':>10s} {'sd':>6s} {'n':>6s} | {'new us':>10s} {'sd':>6s} {'n':>6s}")
for k, (m, sd, n) in sorted(a.items(), key=lambda t: -t[1][0] * t[1][2]):
    if n < 2 and m < 3: continue
    k2, (m2, sd2, n2) = bb.get(key(k), (k, (float('nan'), float('nan'), 0)))
    print(f"{k[:70]:70s} {m:10.2f} {sd:6.2f} {n:6d} | {m2:10.2f} {sd2:6.2f} {n2:6d}" + (f"   (new: {k2[:40]})" if k2 != k else ""))
