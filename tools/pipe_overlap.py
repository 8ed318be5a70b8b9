"""Where the time of the pipelined HBM-resident plan-label steps goes, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o run -- python bench.py
    python tools/pipe_overlap.py <dir> [--json out.json] [--burst K]

Reads *kernel_trace.csv, keeps plan label's kernels (the first stage `label_kernel`, the fused
first stage `label_carry_kernel`, the dense pass `label_full_kernel`) and finds the bursts of
pipelined calls: runs of such kernels on two or more queues with no idle gap above 100 us.  For
the longest burst (the bench's timed steps; --burst K: the K-th longest) it prints, per PAIR of
calls (one call on each of the two streams):

  * the time with at least one first stage running,
  * the time with only dense passes running,
  * the idle time (no plan-label kernel running),
  * every gap on a queue before a first stage, by the kind of kernel the gap follows,
  * the kernels' own durations (median and range).

The first and last two calls of the burst are left out (ramp-up and drain).
"""
import csv
import glob
import json
import os
import statistics
import sys

FIRST = ("label_kernel", "label_carry_kernel")
DENSE = ("label_full_kernel",)
GAP_NS = 100_000


def kind_of(name):
    base = name.replace("void ", "").replace("(anonymous namespace)::", "").split("<")[0].split("(")[0].strip()
    if base in FIRST:
        return "first", base
    if base in DENSE:
        return "dense", base
    return None, base


def load(src):
    ev = []
    for p in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                k, base = kind_of(r.get("Kernel_Name", ""))
                if k:
                    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, base,
                               r.get("Queue_Id") or r.get("Stream_Id") or "0"))
    ev.sort()
    return ev


def bursts(ev):
    out, cur, end = [], [], 0
    for e in ev:
        if cur and e[0] - end > GAP_NS:
            out.append(cur)
            cur = []
        cur.append(e)
        end = max(end, e[1])
    if cur:
        out.append(cur)
    return [b for b in out if len({e[4] for e in b}) >= 2 and sum(e[2] == "first" for e in b) >= 8]


def med(v):
    return round(statistics.median(v) / 1e3, 2) if v else None


def analyse(b):
    firsts = [e for e in b if e[2] == "first"]
    lo, hi = firsts[2][0], firsts[-3][0]  # window: from the third first stage's start to the third-last's
    calls = sum(lo <= e[0] < hi for e in firsts)
    # sweep: time by what is running
    pts = []
    for s, e, k, _, _ in b:
        s, e = max(s, lo), min(e, hi)
        if s < e:
            pts += [(s, 0, k), (e, 1, k)]
    pts.sort(key=lambda p: (p[0], -p[1]))
    run = {"first": 0, "dense": 0}
    t_first = t_dense = t_idle = 0
    at = lo
    for t, end, k in pts:
        d = t - at
        if run["first"]:
            t_first += d
        elif run["dense"]:
            t_dense += d
        else:
            t_idle += d
        at = t
        run[k] += -1 if end else 1
    t_idle += hi - at
    pairs = calls / 2
    # gaps on a queue before a first stage, by what they follow
    gaps = {}
    byq = {}
    for e in b:
        byq.setdefault(e[4], []).append(e)
    for q, es in byq.items():
        es.sort()
        for prev, cur in zip(es, es[1:]):
            if cur[2] == "first" and lo <= cur[0] < hi:
                gaps.setdefault(prev[3], []).append(cur[0] - prev[1])
    dur = {}
    for s, e, k, base, _ in b:
        if lo <= s < hi:
            dur.setdefault(base, []).append(e - s)
    return {
        "calls": calls, "queues": len(byq), "window_us": round((hi - lo) / 1e3, 1),
        "per_call_us": round((hi - lo) / 1e3 / calls, 2),
        "per_pair_us": {"total": round((hi - lo) / 1e3 / pairs, 2), "first_stage_running": round(t_first / 1e3 / pairs, 2),
                        "dense_only": round(t_dense / 1e3 / pairs, 2), "idle": round(t_idle / 1e3 / pairs, 2)},
        "gap_before_first_stage_us": {k: {"n": len(v), "median": med(v), "min": round(min(v) / 1e3, 2),
                                          "max": round(max(v) / 1e3, 2)} for k, v in gaps.items()},
        "kernel_us": {k: {"n": len(v), "median": med(v), "min": round(min(v) / 1e3, 2), "max": round(max(v) / 1e3, 2)}
                      for k, v in dur.items()},
        "kernels_per_call": round(sum(len(v) for v in dur.values()) / calls, 2),
    }


def main():
    src = sys.argv[1]
    bs = sorted(bursts(load(src)), key=len, reverse=True)
    if not bs:
        raise SystemExit("no burst of pipelined plan-label calls on two queues in this trace")
    k = int(sys.argv[sys.argv.index("--burst") + 1]) if "--burst" in sys.argv else 0
    res = analyse(bs[k])
    res["bursts"] = [len(b) for b in bs]
    print(json.dumps(res, indent=1))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
