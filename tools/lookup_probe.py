"""Reverse lookup against the brute-force route, on the config #2 shape.
    python tools/lookup_probe.py [--scale S] [--targets B] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S).  B users drawn
uniformly (default 1024), object type (docs, viewer).

  lookup       Lookup.lookup_ids_raw over the B users with capacity = needed (taken from one
               count-only call), 30 timed calls after 3 warm-up calls, host wall time from call
               to return: median ms per call, lists/s, ids/s, the tier split.
  brute force  the route a caller has without the lookup: every docs root against ONE user as a
               device-resident batch (ketogpu_queries_upload / _run / _download), in the same
               process on the same device.  Timed for 4 of the users (median of 5 runs each after
               one warm-up run; the run alone, and upload + run + download) and multiplied out
               to B.  The 4 answers are compared id for id with the lookup's.

Writes one JSON document (default profiles/lookup/probe.json) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--targets", type=int, default=1024, help="B: users per lookup call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup", "probe.json"))
    a = p.parse_args()
    from keto_amd import _lib as L
    from keto_amd import check, lookup, persistence, synth
    from keto_amd.snapshot import Snapshot

    s = max(a.scale, 1)
    sizes = dict(users=10_000_000 // s, groups=100_000 // s, docs=2_000_000 // s, tuples=50_000_000 // s, checks=1024)
    t0 = time.perf_counter()
    w = synth.rbac(**sizes, seed=synth.SEED)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    build_s = time.perf_counter() - t0
    st = snap.stats()
    ty = snap.type_id("docs", "viewer")
    rng = np.random.default_rng(synth.SEED)
    users = rng.integers(0, sizes["users"], a.targets)
    targets = lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in users])

    lk = lookup.Lookup(snap, device=a.device)
    t0 = time.perf_counter()
    _, _, count, needed = lk.lookup_ids_raw(targets, ty, 0)
    first_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(3):
        lk.lookup_ids_raw(targets, ty, needed)
    before = lk.stats()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, begin, count, needed2 = lk.lookup_ids_raw(targets, ty, needed)
        ms.append((time.perf_counter() - t0) * 1e3)
    after = lk.stats()
    assert needed2 == needed and not (begin == lookup.TRUNCATED).any()
    med = float(np.median(ms))
    calls = a.reps
    res = {
        "workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                     "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                         "num_nodes", "num_expandable", "num_interior", "num_rev_edges")}},
        "type": ["docs", "viewer"],
        "targets": int(a.targets),
        "lookup": {
            "reps": a.reps, "ms_per_call_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "first_call_ms": round(first_ms, 3),
            "lists_per_s": round(a.targets / med * 1e3, 1), "ids_per_call": int(needed),
            "ids_per_s": round(needed / med * 1e3, 1),
            "largest_list": int(count.max()) if len(count) else 0,
            "tier1_requests_per_call": (after["tier1_requests"] - before["tier1_requests"]) // calls,
            "tier2_requests_per_call": (after["tier2_requests"] - before["tier2_requests"]) // calls,
            "tier2_rounds_per_call": (after["tier2_rounds"] - before["tier2_rounds"]) // calls,
            "set_capacity": after["set_capacity"], "slots": after["slots"],
        },
    }

    # the brute-force route: every docs root against one user
    t0 = time.perf_counter()
    docs = [("docs", f"d{i}", "viewer", {"subject_id": "u0"}) for i in range(sizes["docs"])]
    roots, _, _ = snap.resolve_batch(persistence.request_columns(docs))
    roots = np.ascontiguousarray(roots[roots != L.NODE_NONE])
    resolve_s = time.perf_counter() - t0
    eng = check.Engine(snap, device=a.device)
    run_ms, route_ms, same = [], [], True
    for k in range(min(4, a.targets)):
        t = int(targets[k])
        tg = np.full(len(roots), t, dtype=np.uint32)
        q = eng.upload(roots, tg)
        q.run()
        r1, r2 = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            q2 = eng.upload(roots, tg)
            t1 = time.perf_counter()
            q2.run()
            t2 = time.perf_counter()
            allowed = q2.download()
            t3 = time.perf_counter()
            q2.close()
            r1.append((t2 - t1) * 1e3)
            r2.append((t3 - t0) * 1e3)
        q.close()
        run_ms.append(float(np.median(r1)))
        route_ms.append(float(np.median(r2)))
        brute = np.sort(roots[np.asarray(allowed, dtype=bool)])
        mine = np.sort(out[int(begin[k]):int(begin[k]) + int(count[k])])
        same = same and np.array_equal(brute, mine)
    res["brute_force"] = {
        "roots_per_user": int(len(roots)), "users_timed": len(run_ms),
        "run_ms_per_user": [round(x, 4) for x in run_ms], "route_ms_per_user": [round(x, 4) for x in route_ms],
        "run_ms_for_all_targets": round(float(np.mean(run_ms)) * a.targets, 2),
        "route_ms_for_all_targets": round(float(np.mean(route_ms)) * a.targets, 2),
        "resolve_roots_s": round(resolve_s, 2),
        "answers_equal_lookup": bool(same),
    }
    res["ratio_run_only_over_lookup"] = round(res["brute_force"]["run_ms_for_all_targets"] / med, 1)
    res["ratio_route_over_lookup"] = round(res["brute_force"]["route_ms_for_all_targets"] / med, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("the brute-force answers differ from the lookup's")


if __name__ == "__main__":
    main()
