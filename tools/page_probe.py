"""Sorted, paged lists against the full-list calls, on the config #2 shape.
    python tools/page_probe.py [--scale S] [--requests B] [--reps R] [--limit L] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S), as tools/
subjects_probe.py and tools/lookup_probe.py build it.  Two handles in one process:

  subjects   B documents drawn uniformly (default 1024), roots docs:d#viewer, class SUBJECT_ID
  lookup     B users drawn uniformly, object type (docs, viewer)

On each handle three calls over the same B requests alternate, 30 timed rounds after 3 warm-up
rounds, host wall time from call to return (every call ends in a stream synchronise):

  page        the first page: *_page_raw with limit L (default 100), from 0
  count_only  *_ids_raw with capacity 0: the same closures and counts, nothing written — the
              reference point of the paged call
  full_sorted *_ids_raw with capacity = needed, then np.sort of every list on the host: what a
              caller had to do for an ordered first page before; the call and the sort are also
              reported apart

Then the pages of 8 of the requests (the longest lists among them) are walked to the end with
limit 65536 and must concatenate to the full sorted lists; the first page must equal their
first L ids.  Writes one JSON document (default profiles/paged/probe.json) and prints it;
exits non-zero when a walk differs."""
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


def probe(h, page_raw, ids_raw, ids, filt, limit, reps, note):
    """the three alternating calls on one handle, then the walk -> a result block"""
    clock = time.perf_counter
    _, _, count, needed = ids_raw(ids, filt, 0)

    def full():
        t0 = clock()
        out, begin, cnt, _ = ids_raw(ids, filt, needed)
        t1 = clock()
        lists = [np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, cnt)]
        return lists, (t1 - t0) * 1e3, (clock() - t1) * 1e3

    for _ in range(3):
        page_raw(ids, None, filt, limit)
        ids_raw(ids, filt, 0)
        lists, _, _ = full()
    before = h.stats()
    ms_page, ms_count, ms_call, ms_sort = [], [], [], []
    for _ in range(reps):  # the three calls alternate, so drift of the host hits all alike
        t0 = clock()
        out, ret, cnt, rem = page_raw(ids, None, filt, limit)
        ms_page.append((clock() - t0) * 1e3)
        t0 = clock()
        ids_raw(ids, filt, 0)
        ms_count.append((clock() - t0) * 1e3)
        _, c, s = full()
        ms_call.append(c)
        ms_sort.append(s)
    after = h.stats()
    per = lambda k: (after[k] - before[k]) // (3 * reps)
    same = bool((cnt == count).all() and (rem == count).all())
    for i, w in enumerate(lists):
        same = same and int(ret[i]) == min(limit, len(w)) and np.array_equal(out[i, :int(ret[i])], w[:limit])
    # the walk: the 8 longest lists, pages of 65536 ids to the end
    pick = np.argsort(-count.astype(np.int64), kind="stable")[:8]
    lo = np.zeros(len(pick), dtype=np.uint32)
    acc = [[] for _ in pick]
    active = np.arange(len(pick))
    calls, t0 = 0, clock()
    while len(active):
        out, ret, cnt, rem = page_raw(ids[pick[active]], lo[active], filt, 65536)
        calls += 1
        for j, k in enumerate(active):
            r = int(ret[j])
            acc[k].append(out[j, :r].copy())
            if r:
                lo[k] = int(out[j, r - 1]) + 1
        active = active[rem > ret]
    walk_ms = (clock() - t0) * 1e3
    walked = all(np.array_equal(np.concatenate(a) if a else np.zeros(0, np.uint32), lists[int(i)])
                 for a, i in zip(acc, pick))
    full_ms = [c + s for c, s in zip(ms_call, ms_sort)]
    res = {"requests": int(len(ids)), "limit": int(limit), "ids_per_full_call": int(needed),
           "ids_per_page_call": int(sum(min(limit, len(w)) for w in lists)),
           "largest_list": int(count.max()) if len(count) else 0,
           "requests_with_more_pages": int(sum(len(w) > limit for w in lists)),
           "page": stat(ms_page), "count_only": stat(ms_count), "full_sorted": stat(full_ms),
           "full_call_alone": stat(ms_call), "host_sort_alone": stat(ms_sort),
           "tier1_requests_per_call": per("tier1_requests"), "tier2_requests_per_call": per("tier2_requests"),
           "tier2_rounds_per_call": per("tier2_rounds"), "slots": after["slots"],
           "page_over_count_only": round(float(np.median(ms_page) / np.median(ms_count)), 3),
           "full_sorted_over_page": round(float(np.median(full_ms) / np.median(ms_page)), 3),
           "first_pages_equal_sorted_lists": same,
           "walk": {"requests": int(len(pick)), "limit": 65536, "calls": calls,
                    "ids": int(sum(len(lists[int(i)]) for i in pick)), "ms": round(walk_ms, 3),
                    "pages_concatenate_to_sorted_lists": bool(walked)}}
    note(f"page {res['page']['ms_per_call_median']} ms, count only {res['count_only']['ms_per_call_median']} ms, "
         f"full + sort {res['full_sorted']['ms_per_call_median']} ms; walk ok: {walked}")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--limit", type=int, default=100)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged", "probe.json"))
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

    res = {"workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                        "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                            "num_nodes", "num_expandable", "num_interior", "num_edges")}}}
    with lookup.Subjects(snap, device=a.device) as sj:
        res["subjects"] = {"roots": "docs:d#viewer, uniform", "class": "SUBJECT_ID",
                           **probe(sj, sj.subject_page_raw, sj.subject_ids_raw, roots, lookup.CLASS_SUBJECT_ID,
                                   a.limit, a.reps, note)}
        res["subjects"]["list_capacity"] = sj.stats()["list_capacity"]
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"targets": "users, uniform", "type": "(docs, viewer)",
                         **probe(lk, lk.lookup_page_raw, lk.lookup_ids_raw, targets, ty, a.limit, a.reps, note)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ok = all(res[k]["walk"]["pages_concatenate_to_sorted_lists"] and res[k]["first_pages_equal_sorted_lists"]
             for k in ("subjects", "lookup"))
    if not ok:
        raise SystemExit("a paged answer differs from the sorted full list")


if __name__ == "__main__":
    main()
