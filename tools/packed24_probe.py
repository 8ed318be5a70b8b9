"""Host-to-host check rate with packed 24-bit requests against u32 requests.
    python tools/packed24_probe.py [--scale S] [--reps R] [--warmup W] [--device D]

One engine over a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, 10^6 checks, the same seeds; --scale S divides every size by S).
The requests sit in pinned buffers (u32: two arrays, 8 bytes per check; packed24: one buffer,
6 bytes per check), the result words in a pinned buffer.  After the warm-up calls of both
kinds the u32 call (Engine.check_ids_raw) and the packed call (Engine.check_ids_packed_raw)
alternate, each timed on the host from call to return, and both results are compared with
each other.  Prints one JSON line: both medians, both min-max spreads, the ratio
u32 median / packed median and the path the packed requests took (last_request_path:
2 = read in place by the first stage, 1 = expanded into HBM first)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--reps", type=int, default=30, help="timed calls of each kind (at least 20)")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--device", type=int, default=0)
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20 timed repetitions of each call")
    from keto_amd import check, synth
    from keto_amd.snapshot import Snapshot

    s = max(a.scale, 1)
    sizes = dict(users=10_000_000 // s, groups=100_000 // s, docs=2_000_000 // s, tuples=50_000_000 // s,
                 checks=max(1_000_000 // s, 1024))
    w = synth.rbac(**sizes, seed=synth.SEED, check_seed=synth.SEED + 1)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    if not snap.packed24_ok():
        raise SystemExit(f"the snapshot's {snap.stats()['num_nodes']} nodes do not fit 24-bit ids")
    roots, targets = w.resolve(snap)
    n = len(roots)
    words = (n + 63) // 64
    eng = check.Engine(snap, device=a.device)
    pr, pt = check.pinned(roots), check.pinned(targets)
    pp = check.pinned(check.pack24(roots, targets), np.uint8)
    out32, outp = check.PinnedBuffer(words, np.uint64), check.PinnedBuffer(words, np.uint64)

    def u32():
        eng.check_ids_raw(pr.p.value, pt.p.value, n, out32.p.value)

    def packed():
        eng.check_ids_packed_raw(pp.p.value, n, outp.p.value)

    for _ in range(a.warmup):
        u32()
        packed()
    path = eng.last_request_path()
    plan = eng.last_stats()["plan"]
    t32, tp = [], []
    for _ in range(a.reps):
        for f, ts in ((u32, t32), (packed, tp)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    same = bool((out32.array == outp.array).all())
    m32, mp = float(np.median(t32)), float(np.median(tp))
    print(json.dumps({
        "tool": "packed24_probe", "workload": "config2_rbac" + (f"_div{s}" if s > 1 else ""), **sizes,
        "num_nodes": snap.stats()["num_nodes"], "plan": plan, "reps": a.reps, "warmup": a.warmup,
        "u32_ms_median": round(m32, 4), "u32_ms_min": round(min(t32), 4), "u32_ms_max": round(max(t32), 4),
        "packed_ms_median": round(mp, 4), "packed_ms_min": round(min(tp), 4), "packed_ms_max": round(max(tp), 4),
        "u32_checks_per_s": round(n / m32 * 1e3, 1), "packed_checks_per_s": round(n / mp * 1e3, 1),
        "ratio_u32_over_packed": round(m32 / mp, 4), "bytes_per_check": {"u32": 8, "packed24": 6},
        "last_request_path": path, "results_equal": same,
        "packed_within_u32_spread": bool(mp <= m32 + (max(t32) - min(t32)))}))
    if not same:
        raise SystemExit("the packed call's result words differ from the u32 call's")


if __name__ == "__main__":
    main()
