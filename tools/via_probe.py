"""Listings that say why against the depth calls, and against what a caller did before, on the
config #2 shape.
    python tools/via_probe.py [--scale S] [--requests B] [--sample N] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S), as tools/depth_probe.py
builds it.  Two handles in one process:

  subjects   B documents drawn uniformly (default 1024), roots docs:d#viewer, class SUBJECT_ID
  lookup     B users drawn uniformly, object type (docs, viewer)

On each handle the calls over the same requests alternate, 30 timed rounds after 3 warm-up
rounds, host wall time from call to return, host memory to host memory (every call ends in a
stream synchronise):

  via list      *_via_raw with a NULL depth array and capacity = what the call needs
  depth list    *_depth_raw with a NULL depth array and the same capacity: the same lists
                without via and hops.  via_over_depth is the price of the two arrays.
  via bare      the via call with via and hops NULL: the closure still keeps its parent and hop
                words, but nothing is gathered, stored next to the ids or copied back
  via k = 1,    both calls at max_depth 1, where (nearly) every request stays in LDS: the price
  depth k = 1   in tier 1
  lookup only, over a fixed-seed sample of N requests (default 64):
  via sample    lookup_via_raw over the sample
  before        what a caller did before: lookup_ids_raw over the sample, then one
                path_ids_raw request per listed member (capacities known in advance, no
                re-issue); the pairs are built on the host from the list, inside the timing

Every sampled answer is checked in the first and in the last round: the via call's ids equal the
plain list's, and hops == len(path) - 1 for every member.  Writes one JSON document (default
profiles/via/probe.json) and prints it; exits non-zero on a difference, or when the via call
over the sample is not faster than what a caller did before."""
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


def delta(h, call):
    before = h.via_stats()
    res = call()
    after = h.via_stats()
    keys = ("tier1_requests", "tier2_requests", "tier2_rounds", "list_finishes", "scan_finishes", "ids_produced")
    return res, {k: int(after[k] - before[k]) for k in keys}


def owners(out, begin, count):
    """per word of a cursor call's output the request it belongs to (every list was written)"""
    where = np.empty(len(out), dtype=np.int64)
    for k, (b, c) in enumerate(zip(begin, count)):
        where[int(b):int(b) + int(c)] = k
    return where


def probe(h, via_raw, depth_raw, ids, filt, reps, sample, note, before_calls=None):
    """the alternating calls on one handle -> a result block"""
    clock = time.perf_counter
    need = via_raw(ids, None, filt, 0)[6]
    sub = ids[sample]
    one = np.ones(len(ids), dtype=np.uint32)
    need1 = via_raw(ids, one, filt, 0)[6]
    names = ["via_list", "depth_list", "via_bare", "via_k1", "depth_k1"] + \
        (["via_sample", "before_sample"] if before_calls else [])
    if before_calls:
        ids_raw, path_raw = before_calls
        sub_need = ids_raw(sub, filt, 0)[3]
        out, begin, count, _ = ids_raw(sub, filt, sub_need)
        path_need = path_raw(out, sub[owners(out, begin, count)], 0)[3]

    def before():
        """the plain list, then one path request per listed member -> per pair (request, member, hops)"""
        out, begin, count, _ = ids_raw(sub, filt, sub_need)
        where = owners(out, begin, count)
        pout, pbegin, pcount, _ = path_raw(out, sub[where], path_need)
        return where, out, pcount.astype(np.int64) - 1

    def one_round(ms):
        t0 = clock()
        v = via_raw(ids, None, filt, need)
        t1 = clock()
        d = depth_raw(ids, None, filt, need)
        t2 = clock()
        b = via_raw(ids, None, filt, need, want_via=False, want_hops=False)
        t3 = clock()
        v1 = via_raw(ids, one, filt, need1)
        t4 = clock()
        d1 = depth_raw(ids, one, filt, need1)
        t5 = clock()
        for name, t in zip(names, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            ms[name].append(t * 1e3)
        ok = v[6] == d[4] == b[6] == need and np.array_equal(v[4], d[2]) and np.array_equal(v1[4], d1[2])
        if before_calls:
            t0 = clock()
            sv = via_raw(sub, None, filt, sub_need)
            t1 = clock()
            where, members, hops = before()
            t2 = clock()
            ms["via_sample"].append((t1 - t0) * 1e3)
            ms["before_sample"].append((t2 - t1) * 1e3)
            return ok, (sv, where, members, hops)
        return ok, None

    def same(sv, where, members, hops):
        """the sampled answers: the same members, and hops == len(path) - 1 for every one"""
        out, via, vhops, begin, count, _, _ = sv
        vwhere = owners(out, begin, count)
        a = np.lexsort((out, vwhere))
        b = np.lexsort((members, where))
        return bool(len(out) == len(members) and np.array_equal(out[a], members[b]) and
                    np.array_equal(vwhere[a], where[b]) and np.array_equal(vhops[a].astype(np.int64), hops[b]))

    ms = {name: [] for name in names}
    for _ in range(3):
        one_round(ms)
    ms = {name: [] for name in names}
    counts_equal, checks = True, []
    for r in range(reps):  # the calls alternate, so drift of the host hits all alike
        ok, sampled = one_round(ms)
        counts_equal = counts_equal and bool(ok)
        if before_calls and r in (0, reps - 1):
            checks.append(same(*sampled))
    v, moved = delta(h, lambda: via_raw(ids, None, filt, need))
    hops = v[2]
    res = {"requests": int(len(ids)), "ids_per_call": int(need), "largest_list": int(v[4].max()) if len(ids) else 0,
           "deepest_member_hops": int(hops.max()) if len(hops) else 0, **moved,
           "via_slots": h.via_stats()["slots"], "depth_slots": h.depth_stats()["slots"],
           "via_list": stat(ms["via_list"]), "depth_list": stat(ms["depth_list"]),
           "counts_equal_the_depth_call": counts_equal}
    res["via_over_depth"] = round(res["via_list"]["ms_per_call_median"] / res["depth_list"]["ms_per_call_median"], 3)
    res["via_bare"] = stat(ms["via_bare"])
    _, moved1 = delta(h, lambda: via_raw(ids, one, filt, need1))
    res["k1"] = {"ids_per_call": int(need1), "tier1_requests": moved1["tier1_requests"],
                 "tier2_requests": moved1["tier2_requests"], "via_list": stat(ms["via_k1"]),
                 "depth_list": stat(ms["depth_k1"])}
    res["k1"]["via_over_depth"] = round(res["k1"]["via_list"]["ms_per_call_median"] /
                                        res["k1"]["depth_list"]["ms_per_call_median"], 3)
    line = f"via {res['via_list']['ms_per_call_median']} ms, depth {res['depth_list']['ms_per_call_median']} ms " \
           f"(x{res['via_over_depth']}), bare {res['via_bare']['ms_per_call_median']} ms, tier 2 " \
           f"{moved['tier2_requests']} in {moved['tier2_rounds']} rounds; k = 1: via " \
           f"{res['k1']['via_list']['ms_per_call_median']} ms, depth {res['k1']['depth_list']['ms_per_call_median']} ms"
    if before_calls:
        res["sample"] = {"requests": int(len(sub)), "ids_per_call": int(sub_need),
                         "path_requests_per_call": int(sub_need),
                         "via": stat(ms["via_sample"]), "before": stat(ms["before_sample"]),
                         "hops_equal_path_lengths": {"first_round": checks[0], "last_round": checks[-1]}}
        res["sample"]["before_over_via"] = round(res["sample"]["before"]["ms_per_call_median"] /
                                                 res["sample"]["via"]["ms_per_call_median"], 2)
        line += f"; sample of {len(sub)}: via {res['sample']['via']['ms_per_call_median']} ms, list + paths " \
                f"{res['sample']['before']['ms_per_call_median']} ms, hops equal path lengths: {checks}"
    note(line)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: requests per call")
    p.add_argument("--sample", type=int, default=64, help="N: requests of the before / after comparison")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "via", "probe.json"))
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
    sample = np.sort(np.random.default_rng(11).choice(a.requests, min(a.sample, a.requests), replace=False))

    res = {"workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                        "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                            "num_nodes", "num_expandable", "num_interior", "num_edges")}}}
    with lookup.Subjects(snap, device=a.device) as sj:
        res["subjects"] = {"roots": "docs:d#viewer, uniform", "class": "SUBJECT_ID",
                           **probe(sj, sj.subject_via_raw, sj.subject_depth_raw, roots, lookup.CLASS_SUBJECT_ID, a.reps,
                                   sample, note)}
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"targets": "users, uniform", "type": "(docs, viewer)",
                         **probe(lk, lk.lookup_via_raw, lk.lookup_depth_raw, targets, ty, a.reps, sample, note,
                                 (lk.lookup_ids_raw, lk.path_ids_raw))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    smp = res["lookup"]["sample"]
    if not all(smp["hops_equal_path_lengths"].values()) or not all(
            res[k]["counts_equal_the_depth_call"] for k in ("subjects", "lookup")):
        raise SystemExit("a via answer differs from the plain list and its paths")
    if not smp["via"]["ms_per_call_median"] < smp["before"]["ms_per_call_median"]:
        raise SystemExit("the via call is not faster than the plain list plus one path request per member")


if __name__ == "__main__":
    main()
