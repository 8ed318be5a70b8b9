"""What a listing call costs right after an in-place write, on the config #2 shape.
    python tools/refresh_probe.py [--scale S] [--requests B] [--reps R] [--batch G] [--label L] [--out PATH]

One WRITABLE snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k
groups, 2M docs, 50M tuples, the same seed; --scale S divides every size by S).  The lookup
handle lists the (docs, viewer) objects of B uniform users, the subjects handle the users of B
uniform docs:d#viewer roots (class SUBJECT_ID), as tools/lookup_probe.py and subjects_probe.py
do.  Per handle:

  no_write  R calls with no write between them.
  patched   R times: one single-tuple write (a user joins a group), then one call on a handle
            that follows writes by patching rows.  The call's wall time holds the refresh.
  full      the same writes seen by a second handle created under KETOGPU_LIST_REFRESH=full (every
            version change uploads everything), its call right after the patched handle's.
  batch     one write of G tuples into G different groups, then one call on each handle.

Reported per series: the calls' median and min-max ms, the median host time of the write and of
the refresh alone (the handle's last_refresh_ms), the words a refresh uploaded, the calls that
followed a write which gave a user its first node (N moves: the subjects handle drops tier 2's
state and the call builds it again) on their own, and the handle's refresh statistics at the end.  The library of an earlier commit has neither the statistics nor the
knob: run there, the probe reports the series it can (both handles behave alike) and says so;
--label names the run.  Writes one JSON document (default profiles/refresh/probe.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values, unit="ms"):
    if not values:
        return None
    return {f"median_{unit}": round(float(np.median(values)), 4), f"min_{unit}": round(float(min(values)), 4),
            f"max_{unit}": round(float(max(values)), 4), "n": len(values)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per listing call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--batch", type=int, default=1000, help="G: groups the batch write touches")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--label", default="this commit")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh", "probe.json"))
    a = p.parse_args()
    from keto_amd import lookup, synth
    from keto_amd.snapshot import Snapshot

    note = lambda *x: print(*x, file=sys.stderr, flush=True)  # progress; the result alone goes to stdout
    s = max(a.scale, 1)
    sizes = dict(users=10_000_000 // s, groups=100_000 // s, docs=2_000_000 // s, tuples=50_000_000 // s, checks=1024)
    t0 = time.perf_counter()
    w = synth.rbac(**sizes, seed=synth.SEED)
    snap = Snapshot.from_columns(w.namespaces, w.columns, writable=True)
    build_s = time.perf_counter() - t0
    st = snap.stats()
    note(f"writable snapshot built in {build_s:.1f} s: {st['num_nodes']} nodes, {st['num_edges']} edges")
    rng = np.random.default_rng(synth.SEED)
    ty = snap.type_id("docs", "viewer")
    targets = lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in rng.integers(0, sizes["users"], a.requests)])
    roots = lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in rng.integers(0, sizes["docs"], a.requests)])

    has_stats = hasattr(lookup.Lookup, "refresh_stats")
    handles = {"lookup": {}, "subjects": {}}
    for knob in ("patched", "full") if has_stats else ("parent",):
        if knob == "full":
            os.environ["KETOGPU_LIST_REFRESH"] = "full"
        handles["lookup"][knob] = lookup.Lookup(snap, device=a.device)
        handles["subjects"][knob] = lookup.Subjects(snap, device=a.device)
        os.environ.pop("KETOGPU_LIST_REFRESH", None)
    calls = {"lookup": lambda h, cap: h.lookup_ids_raw(targets, ty, cap),
             "subjects": lambda h, cap: h.subject_ids_raw(roots, lookup.CLASS_SUBJECT_ID, cap)}
    cap = {}
    for kind, hs in handles.items():
        for h in hs.values():
            needed = calls[kind](h, 0)[3]
            cap[kind] = int(needed * 1.25) + 65536  # (the lists grow a little with the writes)
            for _ in range(3):
                calls[kind](h, cap[kind])
    note("handles ready:", {k: v for k, v in cap.items()})

    def timed(kind, h):
        t0 = time.perf_counter()
        calls[kind](h, cap[kind])
        return (time.perf_counter() - t0) * 1e3

    def refresh_of(h):
        return h.refresh_stats() if has_stats else {}

    res = {"label": a.label, "has_refresh_stats": has_stats,
           "workload": {"shape": "config #2 (synth.rbac), KETOGPU_BUILD_WRITABLE", "scale_divisor": s, **sizes,
                        "seed": synth.SEED, "snapshot_build_s": round(build_s, 2),
                        **{k: st[k] for k in ("num_nodes", "num_expandable", "num_interior", "num_edges", "num_rev_edges")}},
           "requests": int(a.requests), "reps": a.reps}
    first = next(iter(handles["lookup"]))
    res["no_write"] = {kind: summary([timed(kind, hs[first]) for _ in range(a.reps)]) for kind, hs in handles.items()}
    note("no_write:", res["no_write"])

    def one_write(n_rows):
        """n_rows users join n_rows different groups -> (host ms of the write, refused attempts)"""
        refused = 0
        for _ in range(20):
            gs = rng.choice(sizes["groups"], n_rows, replace=False)
            us = rng.choice(sizes["users"], n_rows, replace=False)
            rows = [(1, f"g{int(g)}", "member", f"u{int(u)}", None, None, None) for g, u in zip(gs, us)]
            t0 = time.perf_counter()
            r = snap.write(rows, [])
            ms = (time.perf_counter() - t0) * 1e3
            if r["applied"]:
                return ms, refused, r
            refused += 1
        raise SystemExit(f"20 writes in a row were refused: {r}")

    series = {kind: {knob: {"call_ms": [], "refresh_ms": [], "words": [], "grown_ms": []} for knob in hs}
              for kind, hs in handles.items()}
    write_ms, refused, grown = [], 0, 0
    for _ in range(a.reps):
        ms, bad, r = one_write(1)
        write_ms.append(ms)
        refused += bad
        grown += r["new_nodes"] > 0
        for kind, hs in handles.items():
            for knob, h in hs.items():
                before = refresh_of(h)
                series[kind][knob]["call_ms"].append(timed(kind, h))
                if r["new_nodes"]:  # the user had no node yet: N moved, and with it the subjects handle's bound
                    series[kind][knob]["grown_ms"].append(series[kind][knob]["call_ms"][-1])
                after = refresh_of(h)
                if has_stats:
                    series[kind][knob]["refresh_ms"].append(after["last_refresh_ms"])
                    series[kind][knob]["words"].append(after["words_uploaded"] - before["words_uploaded"])
    res["single_tuple_write"] = {"write_ms": summary(write_ms), "refused_attempts": refused,
                                 "writes_that_added_a_node": int(grown)}
    res["first_call_after_write"] = {
        kind: {knob: {"call_ms": summary(d["call_ms"]), "refresh_ms": summary(d["refresh_ms"]),
                      "words_uploaded_per_refresh": summary(d["words"], "words"),
                      "call_ms_after_a_write_that_added_a_node": summary(d["grown_ms"])} for knob, d in ks.items()}
        for kind, ks in series.items()}
    note("first_call_after_write:", res["first_call_after_write"])

    ms, bad, r = one_write(a.batch)
    res["batch_write"] = {"groups": a.batch, "write_ms": round(ms, 3), "refused_attempts": bad,
                          "device_rows": r["device_rows"], "new_nodes": r["new_nodes"], "calls": {}}
    for kind, hs in handles.items():
        for knob, h in hs.items():
            before = refresh_of(h)
            call = timed(kind, h)
            after = refresh_of(h)
            res["batch_write"]["calls"][f"{kind}/{knob}"] = {
                "call_ms": round(call, 3), "refresh_ms": round(after.get("last_refresh_ms", 0.0), 3) if has_stats else None,
                "words_uploaded": after["words_uploaded"] - before["words_uploaded"] if has_stats else None}
    res["refresh_stats"] = {f"{kind}/{knob}": refresh_of(h) for kind, hs in handles.items() for knob, h in hs.items()}
    res["uploads"] = {f"{kind}/{knob}": h.stats()["uploads"] for kind, hs in handles.items() for knob, h in hs.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
