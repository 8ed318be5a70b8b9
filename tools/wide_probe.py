"""The wide calls against the plain calls, on the config #2 shape.
    python tools/wide_probe.py [--scale S] [--requests B] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S).  Two handles:

  subjects  tools/subjects_probe.py's requests: B documents drawn uniformly (default 1024), roots
            docs:d#viewer, class SUBJECT_ID
  lookup    tools/lookup_probe.py's requests: B users drawn uniformly, object type (docs, viewer)

On each, host to host, the plain call (ketogpu_*_ids) and the wide call (ketogpu_*_ids_wide)
alternate in one process, R timed calls each (default 30) after 3 warm-up calls each; medians with
min-max:

  full_lists  all B requests with capacity = needed
  count_only  all B requests with capacity 0
  longest     n = 1: the request with the longest list, capacity = its count

with the wide tier's requests, rounds, levels and items per call from its statistics.  Every list
of the wide calls is compared id for id with the plain call's.

Writes one JSON document (default profiles/wide/probe.json) and prints it; exits non-zero when a
list differs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lists_of(out, begin, count):
    return [np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, count)]


def measure(h, raw, ids, filter_id, capacity, reps):
    """plain and wide alternate -> (block, the two last results)"""
    for _ in range(3):
        raw(ids, filter_id, capacity, wide=False)
        raw(ids, filter_id, capacity, wide=True)
    ms = {False: [], True: []}
    before = h.wide_stats()
    for _ in range(reps):  # the two calls alternate, so drift of the host hits both alike
        res = {}
        for wide in (False, True):
            t0 = time.perf_counter()
            res[wide] = raw(ids, filter_id, capacity, wide=wide)
            ms[wide].append((time.perf_counter() - t0) * 1e3)
    after = h.wide_stats()
    per = lambda k: (after[k] - before[k]) / reps
    stat = lambda v: {"ms_per_call_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4),
                      "ms_max": round(max(v), 4)}
    block = {"reps": reps, "requests": int(len(ids)), "capacity": int(capacity), "plain": stat(ms[False]),
             "wide": stat(ms[True]),
             "plain_over_wide": round(float(np.median(ms[False]) / np.median(ms[True])), 3),
             "wide_per_call": {k: per(k) for k in ("tier1_requests", "wide_requests", "wide_rounds", "levels", "items")},
             "slots": after["slots"]}
    return block, res[False], res[True]


def side(h, raw, ids, filter_id, reps, note, name):
    from keto_amd.lookup import TRUNCATED
    _, _, count, needed = raw(ids, filter_id, 0, wide=False)
    same = True
    full, p, w = measure(h, raw, ids, filter_id, needed, reps)
    same = same and p[3] == w[3] == needed and not (w[1] == TRUNCATED).any()
    same = same and all(np.array_equal(a, b) for a, b in zip(lists_of(*p[:3]), lists_of(*w[:3])))
    note(f"{name} full lists: plain {full['plain']['ms_per_call_median']} ms, wide {full['wide']['ms_per_call_median']} ms")
    cnt, p, w = measure(h, raw, ids, filter_id, 0, reps)
    same = same and p[3] == w[3] and (p[2] == w[2]).all()
    note(f"{name} count only: plain {cnt['plain']['ms_per_call_median']} ms, wide {cnt['wide']['ms_per_call_median']} ms")
    k = int(np.argmax(count))
    one, p, w = measure(h, raw, ids[k:k + 1], filter_id, int(count[k]), reps)
    same = same and np.array_equal(lists_of(*p[:3])[0], lists_of(*w[:3])[0]) and int(w[2][0]) == int(count[k])
    note(f"{name} longest ({int(count[k])} ids): plain {one['plain']['ms_per_call_median']} ms, "
         f"wide {one['wide']['ms_per_call_median']} ms")
    return {"ids_per_call": int(needed), "largest_list": int(count[k]), "full_lists": full, "count_only": cnt,
            "longest": one, "chunk": h.wide_stats()["chunk"], "lists_equal_plain": bool(same)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide", "probe.json"))
    a = p.parse_args()
    from keto_amd import lookup, synth
    from keto_amd.snapshot import Snapshot

    note = lambda *x: print(*x, file=sys.stderr, flush=True)  # progress; the result alone goes to stdout
    s = max(a.scale, 1)
    sizes = dict(users=10_000_000 // s, groups=100_000 // s, docs=2_000_000 // s, tuples=50_000_000 // s, checks=1024)
    t0 = time.perf_counter()
    w = synth.rbac(**sizes, seed=synth.SEED)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    build_s = time.perf_counter() - t0
    st = snap.stats()
    note(f"snapshot built in {build_s:.1f} s: {st['num_nodes']} nodes, {st['num_edges']} edges")
    res = {"workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                        "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                            "num_nodes", "num_expandable", "num_interior", "num_edges", "num_rev_edges")}}}

    docs = np.random.default_rng(synth.SEED).integers(0, sizes["docs"], a.requests)
    roots = lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in docs])
    with lookup.Subjects(snap, device=a.device) as sj:
        res["subjects"] = {"class": "SUBJECT_ID", **side(sj, sj.subject_ids_raw, roots, lookup.CLASS_SUBJECT_ID,
                                                         a.reps, note, "subjects")}
    users = np.random.default_rng(synth.SEED).integers(0, sizes["users"], a.requests)
    targets = lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in users])
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"type": ["docs", "viewer"], **side(lk, lk.lookup_ids_raw, targets,
                                                            snap.type_id("docs", "viewer"), a.reps, note, "lookup")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (res["subjects"]["lists_equal_plain"] and res["lookup"]["lists_equal_plain"]):
        raise SystemExit("a wide list differs from the plain call's")


if __name__ == "__main__":
    main()
