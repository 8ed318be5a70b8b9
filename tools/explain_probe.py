"""Shortest-path explanations against the count-only reverse lookup, on the config #2 shape.
    python tools/explain_probe.py [--scale S] [--requests B] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S), as tools/lookup_probe.py
builds it, and one lookup handle.  B (default 1024) pairs (docs:d#viewer, user), documents and
users each drawn uniformly (the documents of tools/subjects_probe.py, the users of tools/
lookup_probe.py).  Two calls over the same B users alternate in one process, 30 timed rounds
after 3 warm-up rounds, host wall time from call to return, host memory to host memory:

  paths       ketogpu_lookup_paths with capacity = needed
  count_only  ketogpu_lookup_ids with capacity 0, type (docs, viewer): the same closures run to
              their end without early exit or parents, nothing written — the reference point

Uniform pairs are almost all denied, so their searches run to exhaustion like the lookup's.  A
second block times B pairs that are all allowed: for every user with a non-empty list, one of
the documents the lookup lists for that user, against the count-only call of those users.
Every path is compared with the host call (the same length) and judged hop by hop against the
snapshot's reverse rows.  Writes one JSON document (default profiles/explain/probe.json) and
prints it; exits non-zero when a path is wrong."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(ms):
    return {"reps": len(ms), "ms_per_call_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def paths_ok(snap, graph, roots, targets, out, begin, count, host_check):
    """every path starts at its root, ends at its target and moves along reverse rows; the first
    `host_check` pairs also have the host call's length (a shortest path: the host searches
    level by level)"""
    from keto_amd import lookup
    ro, rc = graph["rev_off"], graph["rev_col"]
    for k in range(len(roots)):
        c = int(count[k])
        if k < host_check and c != len(lookup.host_path(snap, int(roots[k]), int(targets[k]))):
            return False
        if not c:
            continue
        p = out[int(begin[k]):int(begin[k]) + c]
        if c < 2 or p[0] != roots[k] or p[-1] != targets[k]:
            return False
        for a, b in zip(p[:-1], p[1:]):
            row = rc[int(ro[b]):int(ro[b + 1])]
            j = int(np.searchsorted(row, a))  # the rows are sorted
            if not ((j < len(row) and row[j] == a) or a in row):
                return False
    return True


def probe(lk, snap, graph, roots, targets, ty, reps, host_check, note):
    """the two alternating calls -> a result block"""
    clock = time.perf_counter
    _, _, count, needed = lk.path_ids_raw(roots, targets, 0)
    for _ in range(3):
        lk.path_ids_raw(roots, targets, needed)
        lk.lookup_ids_raw(targets, ty, 0)
    pb, lb = lk.path_stats(), lk.stats()
    ms_path, ms_count = [], []
    for _ in range(reps):  # the two calls alternate, so drift of the host hits both alike
        t0 = clock()
        out, begin, cnt, _ = lk.path_ids_raw(roots, targets, needed)
        ms_path.append((clock() - t0) * 1e3)
        t0 = clock()
        _, _, lcount, lneeded = lk.lookup_ids_raw(targets, ty, 0)
        ms_count.append((clock() - t0) * 1e3)
    pa, la = lk.path_stats(), lk.stats()
    per = lambda a, b, k: (a[k] - b[k]) // reps
    ok = bool((cnt == count).all() and (begin < np.uint64(max(needed, 1))).all()) and \
        paths_ok(snap, graph, roots, targets, out, begin, cnt, host_check)
    res = {"pairs": int(len(roots)), "allowed": int((cnt > 0).sum()), "ids_per_path_call": int(needed),
           "longest_path_nodes": int(cnt.max()) if len(cnt) else 0,
           "path_nodes_histogram": {str(int(v)): int(c) for v, c in zip(*np.unique(cnt, return_counts=True))},
           "paths": stat(ms_path), "count_only": stat(ms_count),
           "paths_over_count_only": round(float(np.median(ms_path) / np.median(ms_count)), 3),
           "paths_tier1_requests_per_call": per(pa, pb, "tier1_requests"),
           "paths_tier2_requests_per_call": per(pa, pb, "tier2_requests"),
           "paths_tier2_rounds_per_call": per(pa, pb, "tier2_rounds"),
           "count_only_tier1_requests_per_call": per(la, lb, "tier1_requests"),
           "count_only_tier2_requests_per_call": per(la, lb, "tier2_requests"),
           "count_only_tier2_rounds_per_call": per(la, lb, "tier2_rounds"),
           "count_only_ids": int(lneeded), "count_only_largest_list": int(lcount.max()) if len(lcount) else 0,
           "slots": la["slots"], "host_checked_pairs": int(min(host_check, len(roots))), "paths_valid": ok}
    note(f"paths {res['paths']['ms_per_call_median']} ms, count only {res['count_only']['ms_per_call_median']} ms; "
         f"{res['allowed']} of {res['pairs']} allowed, longest {res['longest_path_nodes']} nodes; valid: {ok}")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: pairs per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--host-check", type=int, default=1024, help="pairs per block compared with the host call")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain", "probe.json"))
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
    rng = np.random.default_rng(synth.SEED)  # the documents of tools/subjects_probe.py
    docs = rng.integers(0, sizes["docs"], a.requests)
    roots = lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in docs])
    rng = np.random.default_rng(synth.SEED)  # the users of tools/lookup_probe.py
    users = rng.integers(0, sizes["users"], a.requests)
    targets = lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in users])
    ty = snap.type_id("docs", "viewer")
    assert ty not in (lookup.TYPE_NONE, lookup.TYPE_ANY)
    graph = snap.graph()

    res = {"workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                        "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                            "num_nodes", "num_expandable", "num_interior", "num_edges")}}}
    with lookup.Lookup(snap, device=a.device) as lk:
        res["set_capacity"] = lk.stats()["set_capacity"]
        res["uniform_pairs"] = {"roots": "docs:d#viewer, uniform", "targets": "users, uniform",
                                "count_only_type": "(docs, viewer)",
                                **probe(lk, snap, graph, roots, targets, ty, a.reps, a.host_check, note)}
        # pairs that are all allowed: one listed document per user that has any
        lists = lk.lookup_ids(targets, ty)
        rng = np.random.default_rng(synth.SEED + 1)
        have = [k for k, ids in enumerate(lists) if len(ids)]
        r2 = np.array([lists[k][int(rng.integers(0, len(lists[k])))] for k in have], dtype=np.uint32)
        t2 = targets[have]
        res["allowed_pairs"] = {"roots": "one document of the user's own list, uniform", "targets": "the same users, "
                                "those with a non-empty list", "count_only_type": "(docs, viewer)",
                                **probe(lk, snap, graph, r2, t2, ty, a.reps, a.host_check, note)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (res["uniform_pairs"]["paths_valid"] and res["allowed_pairs"]["paths_valid"]):
        raise SystemExit("a path is wrong")


if __name__ == "__main__":
    main()
