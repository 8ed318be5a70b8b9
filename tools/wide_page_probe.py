"""The wide paged and depth calls against the plain ones, on the config #2 shape.
    python tools/wide_page_probe.py [--scale S] [--requests B] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S).  Two handles:

  subjects  tools/subjects_probe.py's requests: B documents drawn uniformly (default 1024), roots
            docs:d#viewer, class SUBJECT_ID
  lookup    tools/lookup_probe.py's requests: B users drawn uniformly, object type (docs, viewer)

On each, host to host, the plain call (ketogpu_*_page, ketogpu_*_page_depth, ketogpu_*_ids_depth)
and the wide call (ketogpu_*_page_wide, ketogpu_*_ids_depth_wide) alternate in one process, R timed
calls each (default 30) after 3 warm-up calls each; medians with min-max.  The legs:

  first_page        limit 100, from 0
  mid_page          limit 100, from the middle id of each list
  page_65536        limit 65536, from 0
  depth1/2/3_page   limit 100, from 0, max_depth 1, 2, 3
  depth2_lists      full lists at max_depth 2, capacity = needed
  longest_page      n = 1: the request with the longest list, limit 100
  sparse_page       n = 1: that request under a filter that passes few of its members, the
                    (groups, member) sets, limit 100: one workgroup selects over the whole bitmap

with the wide tier's requests, rounds, levels and items per call from its statistics.  Every answer
of a wide call is compared field for field with the plain call's.

Writes one JSON document (default profiles/wide_page/probe.json) and prints it; exits non-zero
when an answer differs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def same_page(p, w):
    """out[:returned], returned, count, remaining and (where both have one) frontier"""
    ok = all(np.array_equal(a, b) for a, b in zip(p[1:], w[1:]))
    return ok and all(np.array_equal(p[0][i, :int(k)], w[0][i, :int(k)]) for i, k in enumerate(p[1]))


def same_lists(p, w):
    out, begin, count, frontier, needed = p
    lists = lambda r: [np.sort(r[0][int(b):int(b) + int(c)]) for b, c in zip(r[1], r[2])]
    ok = needed == w[4] and np.array_equal(count, w[2]) and np.array_equal(frontier, w[3])
    return ok and all(np.array_equal(a, b) for a, b in zip(lists(p), lists(w)))


def measure(h, call, same, reps):
    """call(wide) -> a result; plain and wide alternate -> a block"""
    for _ in range(3):
        call(False)
        call(True)
    ms = {False: [], True: []}
    before = h.wide_stats()
    equal = True
    for _ in range(reps):  # the two calls alternate, so drift of the host hits both alike
        res = {}
        for wide in (False, True):
            t0 = time.perf_counter()
            res[wide] = call(wide)
            ms[wide].append((time.perf_counter() - t0) * 1e3)
        equal = equal and bool(same(res[False], res[True]))  # (outside the timed part)
    after = h.wide_stats()
    per = lambda k: (after[k] - before[k]) / reps
    stat = lambda v: {"ms_per_call_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4),
                      "ms_max": round(max(v), 4)}
    return {"reps": reps, "plain": stat(ms[False]), "wide": stat(ms[True]),
            "plain_over_wide": round(float(np.median(ms[False]) / np.median(ms[True])), 3),
            "wide_per_call": {k: per(k) for k in ("tier1_requests", "wide_requests", "wide_rounds", "levels", "items",
                                                  "ids_produced")},
            "slots": after["slots"], "equal_plain": equal}


def side(h, ids_raw, page_raw, depth_page_raw, depth_raw, ids, filt, sparse_filt, reps, note, name):
    out, begin, count, needed = ids_raw(ids, filt, 0)
    out, begin, count, needed = ids_raw(ids, filt, needed)
    mid = np.zeros(len(ids), dtype=np.uint32)
    for i, (b, c) in enumerate(zip(begin, count)):
        if c:
            mid[i] = np.sort(out[int(b):int(b) + int(c)])[int(c) // 2]
    del out
    res = {"requests": int(len(ids)), "ids_in_all_lists": int(needed), "largest_list": int(count.max())}

    def leg(key, call, same=same_page):
        res[key] = measure(h, call, same, reps)
        note(f"{name} {key}: plain {res[key]['plain']['ms_per_call_median']} ms, wide "
             f"{res[key]['wide']['ms_per_call_median']} ms, equal: {res[key]['equal_plain']}")

    leg("first_page", lambda wide: page_raw(ids, None, filt, 100, wide=wide))
    leg("mid_page", lambda wide: page_raw(ids, mid, filt, 100, wide=wide))
    leg("page_65536", lambda wide: page_raw(ids, None, filt, 65536, wide=wide))
    for k in (1, 2, 3):
        leg(f"depth{k}_page", lambda wide, k=k: depth_page_raw(ids, k, None, filt, 100, wide=wide))
    need2 = depth_raw(ids, 2, filt, 0)[4]
    res["ids_within_2_hops"] = int(need2)
    leg("depth2_lists", lambda wide: depth_raw(ids, 2, filt, need2, wide=wide), same_lists)
    one = ids[int(np.argmax(count)):int(np.argmax(count)) + 1]
    leg("longest_page", lambda wide: page_raw(one, None, filt, 100, wide=wide))
    leg("sparse_page", lambda wide: page_raw(one, None, sparse_filt, 100, wide=wide))
    res["sparse_page"]["members_under_the_filter"] = int(page_raw(one, None, sparse_filt, 100)[2][0])
    res["chunk"] = h.wide_stats()["chunk"]
    res["answers_equal_plain"] = all(v["equal_plain"] for v in res.values() if isinstance(v, dict))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_page", "probe.json"))
    a = p.parse_args()
    from keto_amd import _lib, lookup, synth
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
                            "num_nodes", "num_expandable", "num_interior", "num_edges", "num_rev_edges")}},
           "clear_tile_ids": int(_lib.lib().ketogpu_wide_clear_tile_ids())}
    sparse = snap.type_id("groups", "member")
    assert sparse not in (lookup.TYPE_NONE, lookup.TYPE_ANY)

    docs = np.random.default_rng(synth.SEED).integers(0, sizes["docs"], a.requests)
    roots = lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in docs])
    with lookup.Subjects(snap, device=a.device) as sj:
        res["subjects"] = {"class": "SUBJECT_ID", "sparse_filter": ["groups", "member"],
                           **side(sj, sj.subject_ids_raw, sj.subject_page_raw, sj.subject_depth_page_raw,
                                  sj.subject_depth_raw, roots, lookup.CLASS_SUBJECT_ID, sparse, a.reps, note,
                                  "subjects")}
    users = np.random.default_rng(synth.SEED).integers(0, sizes["users"], a.requests)
    targets = lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in users])
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"type": ["docs", "viewer"], "sparse_filter": ["groups", "member"],
                         **side(lk, lk.lookup_ids_raw, lk.lookup_page_raw, lk.lookup_depth_page_raw,
                                lk.lookup_depth_raw, targets, snap.type_id("docs", "viewer"), sparse, a.reps, note,
                                "lookup")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (res["subjects"]["answers_equal_plain"] and res["lookup"]["answers_equal_plain"]):
        raise SystemExit("a wide answer differs from the plain call's")


if __name__ == "__main__":
    main()
