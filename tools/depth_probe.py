"""Depth-limited listings against the plain calls, on the config #2 shape.
    python tools/depth_probe.py [--scale S] [--requests B] [--reps R] [--limit L] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S), as tools/page_probe.py
builds it.  Two handles in one process:

  subjects   B documents drawn uniformly (default 1024), roots docs:d#viewer, class SUBJECT_ID
  lookup     B users drawn uniformly, object type (docs, viewer)

On each handle ten calls over the same B requests alternate, 30 timed rounds after 3 warm-up
rounds, host wall time from call to return, host memory to host memory (every call ends in a
stream synchronise):

  depth k list   *_depth_raw at k = 1, 2, 3 and DEPTH_ALL with capacity = what the call needs
  depth k page   *_depth_page_raw at the same k: the first page of L ids (default 100), from 0
  plain list     *_ids_raw with capacity = needed: the reference point of DEPTH_ALL, in the same run
  plain count    *_ids_raw with capacity 0

Per k the tier split, the ids produced and the cut requests of one list call are reported from
the depth stats.  The answers of the first and of the last round are compared with the host
twins (ketogpu_snapshot_*_depth) on a sample of 64 requests per k: lists as sorted arrays,
frontiers, counts and first pages.  Writes one JSON document (default profiles/depth/probe.json)
and prints it; exits non-zero on a difference."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 2, 3, 0)  # 0: DEPTH_ALL


def stat(ms):
    return {"reps": len(ms), "ms_per_call_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def probe(h, snap, depth_raw, depth_page_raw, ids_raw, host_depth, ids, filt, limit, reps, note):
    """the ten alternating calls on one handle, checked against the host twins -> a result block"""
    clock = time.perf_counter
    n = len(ids)
    depths = {k: np.full(n, k, dtype=np.uint32) for k in KS}
    need = {k: depth_raw(ids, depths[k], filt, 0)[4] for k in KS}
    plain_need = ids_raw(ids, filt, 0)[3]
    sample = np.random.default_rng(11).choice(n, min(64, n), replace=False)
    twin = {k: [host_depth(snap, int(ids[i]), k, filt) for i in sample] for k in KS}

    def same(k, lst, page):
        out, begin, count, frontier, _ = lst
        pout, ret, pcnt, prem, pfr = page
        ok = True
        for j, i in enumerate(sample):
            w, f = twin[k][j]
            got = np.sort(out[int(begin[i]):int(begin[i]) + int(count[i])])
            ok = ok and np.array_equal(got, w) and int(frontier[i]) == f == int(pfr[i])
            ok = ok and int(pcnt[i]) == len(w) == int(prem[i]) and np.array_equal(pout[i, :int(ret[i])], w[:limit])
        return bool(ok)

    def one_round(ms):
        res = {}
        for k in KS:
            t0 = clock()
            lst = depth_raw(ids, depths[k], filt, need[k])
            t1 = clock()
            page = depth_page_raw(ids, depths[k], None, filt, limit)
            t2 = clock()
            ms[f"list_{k}"].append((t1 - t0) * 1e3)
            ms[f"page_{k}"].append((t2 - t1) * 1e3)
            res[k] = (lst, page)
        t0 = clock()
        ids_raw(ids, filt, plain_need)
        t1 = clock()
        ids_raw(ids, filt, 0)
        ms["plain_list"].append((t1 - t0) * 1e3)
        ms["plain_count"].append((clock() - t1) * 1e3)
        return res

    names = [f"{c}_{k}" for k in KS for c in ("list", "page")] + ["plain_list", "plain_count"]
    ms = {name: [] for name in names}
    for _ in range(3):
        one_round(ms)
    ms = {name: [] for name in names}
    checks = []
    for r in range(reps):  # the calls alternate, so drift of the host hits all alike
        res = one_round(ms)
        if r in (0, reps - 1):
            checks.append(all(same(k, *res[k]) for k in KS))
    per_k = {}
    for k in KS:  # one more list call per k, for the stats of exactly one call
        before = h.depth_stats()
        out, begin, count, frontier, needed = depth_raw(ids, depths[k], filt, need[k])
        after = h.depth_stats()
        d = lambda key: int(after[key] - before[key])
        per_k["all" if k == 0 else str(k)] = {
            "list": stat(ms[f"list_{k}"]), "page": stat(ms[f"page_{k}"]),
            "tier1_requests": d("tier1_requests"), "tier2_requests": d("tier2_requests"),
            "tier2_rounds": d("tier2_rounds"), "list_finishes": d("list_finishes"),
            "scan_finishes": d("scan_finishes"), "ids_produced": d("ids_produced"),
            "cut_requests": d("cut_requests"), "largest_list": int(count.max()) if n else 0}
    plain = stat(ms["plain_list"])
    res = {"requests": int(n), "limit": int(limit), "depth": per_k, "plain_list": plain,
           "plain_count_only": stat(ms["plain_count"]), "ids_per_plain_call": int(plain_need),
           "slots": h.depth_stats()["slots"],
           "depth_all_over_plain": round(per_k["all"]["list"]["ms_per_call_median"] / plain["ms_per_call_median"], 3),
           "plain_spread_ms": round(plain["ms_max"] - plain["ms_min"], 4),
           "answers_equal_host_twins": {"first_round": checks[0], "last_round": checks[-1],
                                        "sample_per_k": int(len(sample))}}
    note("; ".join(f"k={k}: list {v['list']['ms_per_call_median']} ms, page {v['page']['ms_per_call_median']} ms, "
                   f"tier 2 {v['tier2_requests']}" for k, v in per_k.items())
         + f"; plain {plain['ms_per_call_median']} ms; equal to the host twins: {checks}")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--limit", type=int, default=100)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth", "probe.json"))
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
                           **probe(sj, snap, sj.subject_depth_raw, sj.subject_depth_page_raw, sj.subject_ids_raw,
                                   lookup.host_subjects_depth, roots, lookup.CLASS_SUBJECT_ID, a.limit, a.reps, note)}
        res["subjects"]["list_capacity"] = sj.stats()["list_capacity"]
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"targets": "users, uniform", "type": "(docs, viewer)",
                         **probe(lk, snap, lk.lookup_depth_raw, lk.lookup_depth_page_raw, lk.lookup_ids_raw,
                                 lookup.host_lookup_depth, targets, ty, a.limit, a.reps, note)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ok = all(res[k]["answers_equal_host_twins"][r] for k in ("subjects", "lookup") for r in ("first_round", "last_round"))
    if not ok:
        raise SystemExit("a depth-limited answer differs from the host twin")


if __name__ == "__main__":
    main()
