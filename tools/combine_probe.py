"""Combined listings against what a caller did before them, on the config #2 shape.
    python tools/combine_probe.py [--scale S] [--requests B] [--reps R] [--limit L] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S), as tools/page_probe.py
builds it.  Two handles in one process:

  subjects   B pairs of documents (default 1024), roots docs:d#viewer, class SUBJECT_ID
  lookup     B pairs of users, object type (docs, viewer)

The first ids are page_probe's; the second of each pair is drawn uniformly as well, and the
share of pairs whose AND is non-empty is reported as drawn (and_nonempty_share).  For each of
the three operators, per timed round (30 after 3 warm-up rounds, host memory to host memory,
every call ends in a stream synchronise) these alternate:

  baseline_full  two plain calls on the same handle (*_ids_raw with capacity = needed, lists
                 downloaded) and the numpy set operation per pair: what a caller does today
  baseline_page  the same plus the numpy sort and slice of the first L ids (default 100),
                 timed on top of the round's baseline_full
  combined_full  one *combine* call with capacity = needed
  combined_page  one *combine_page* call with limit L, from 0

The baseline is never the code under test.  Every combined answer is compared with the
baseline's.  Writes one JSON document (default profiles/combine/probe.json) and prints it; exits
non-zero when an answer differs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETOPS = {"and": lambda x, y: np.intersect1d(x, y, assume_unique=True),
          "andnot": np.setdiff1d, "or": np.union1d}  # (every result ascending)


def stat(ms):
    return {"reps": len(ms), "ms_per_call_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def probe(h, ids_raw, a, b, filt, limit, reps, note):
    """the alternating calls on one handle, per operator -> a result block"""
    clock = time.perf_counter
    need = [int(ids_raw(x, filt, 0)[3]) for x in (a, b)]

    def plain(x, needed):
        out, begin, count, _ = ids_raw(x, filt, needed)
        return [out[int(bg):int(bg) + int(c)] for bg, c in zip(begin, count)]

    res = {"pairs": int(len(a)), "limit": int(limit), "ids_per_plain_call": need}
    for op, fn in SETOPS.items():
        needed = int(h.combine_ids_raw(a, b, op, filt, 0)[3])
        ms = {k: [] for k in ("baseline_full", "baseline_page", "combined_full", "combined_page")}
        same = True
        before = h.combine_stats()
        for rep in range(3 + reps):  # the calls alternate, so drift of the host hits all alike
            t0 = clock()
            want = [fn(x, y) for x, y in zip(plain(a, need[0]), plain(b, need[1]))]
            t1 = clock()
            pages = [np.sort(w)[:limit] for w in want]
            t2 = clock()
            out, begin, count, _ = h.combine_ids_raw(a, b, op, filt, needed)
            t3 = clock()
            pout, ret, pcount, rem = h.combine_page_raw(a, b, op, None, filt, limit)
            t4 = clock()
            if rep >= 3:
                ms["baseline_full"].append((t1 - t0) * 1e3)
                ms["baseline_page"].append((t2 - t0) * 1e3)
                ms["combined_full"].append((t3 - t2) * 1e3)
                ms["combined_page"].append((t4 - t3) * 1e3)
            if rep in (0, 3 + reps - 1):  # every list of the first and the last round
                for i, w in enumerate(want):
                    same = same and int(count[i]) == len(w) == int(pcount[i]) and int(ret[i]) == len(pages[i]) \
                        and np.array_equal(np.sort(out[int(begin[i]):int(begin[i]) + int(count[i])]), w) \
                        and np.array_equal(pout[i, :int(ret[i])], pages[i])
            else:
                same = same and [int(c) for c in count] == [len(w) for w in want] == [int(c) for c in pcount]
        after = h.combine_stats()
        per = lambda k: (after[k] - before[k]) // (2 * (3 + reps))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res[op] = {"ids_per_combined_call": needed, "nonempty_share": round(float(np.mean([len(w) > 0 for w in want])), 4),
                   "largest_list": int(max(len(w) for w in want)), **{k: stat(v) for k, v in ms.items()},
                   "tier1_pairs_per_call": per("tier1_requests"), "tier2_pairs_per_call": per("tier2_requests"),
                   "tier2_rounds_per_call": per("tier2_rounds"), "slots": after["slots"],
                   "baseline_full_over_combined_full": round(med["baseline_full"] / med["combined_full"], 3),
                   "baseline_page_over_combined_page": round(med["baseline_page"] / med["combined_page"], 3),
                   "answers_equal_baseline": bool(same)}
        note(f"  {op}: full {med['combined_full']:.2f} ms against {med['baseline_full']:.2f} ms, page "
             f"{med['combined_page']:.2f} ms against {med['baseline_page']:.2f} ms; equal: {same}")
    res["and_nonempty_share"] = res["and"]["nonempty_share"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--requests", type=int, default=1024, help="B: pairs per call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--limit", type=int, default=100)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine", "probe.json"))
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
    rng = np.random.default_rng(synth.SEED)  # the documents of tools/page_probe.py, then their partners
    docs = [rng.integers(0, sizes["docs"], a.requests) for _ in range(2)]
    roots = [lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in ds]) for ds in docs]
    rng = np.random.default_rng(synth.SEED)  # the users of tools/page_probe.py, then their partners
    users = [rng.integers(0, sizes["users"], a.requests) for _ in range(2)]
    targets = [lookup.resolve_subjects(snap, [{"subject_id": f"u{int(u)}"} for u in us]) for us in users]
    ty = snap.type_id("docs", "viewer")
    assert ty not in (lookup.TYPE_NONE, lookup.TYPE_ANY)

    res = {"workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                        "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                            "num_nodes", "num_expandable", "num_interior", "num_edges")}},
           "method": {"warmup_rounds": 3, "timed_rounds": a.reps, "pairs": "both sides drawn uniformly",
                      "baseline": "two plain full-list calls on the same handle + numpy set operation per pair "
                                  "(page: + numpy sort and slice)"}}
    note("subjects")
    with lookup.Subjects(snap, device=a.device) as sj:
        res["subjects"] = {"roots": "pairs of docs:d#viewer", "class": "SUBJECT_ID",
                           **probe(sj, sj.subject_ids_raw, roots[0], roots[1], lookup.CLASS_SUBJECT_ID, a.limit,
                                   a.reps, note)}
    note("lookup")
    with lookup.Lookup(snap, device=a.device) as lk:
        res["lookup"] = {"targets": "pairs of users", "type": "(docs, viewer)",
                         **probe(lk, lk.lookup_ids_raw, targets[0], targets[1], ty, a.limit, a.reps, note)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not all(res[k][op]["answers_equal_baseline"] for k in ("subjects", "lookup") for op in SETOPS):
        raise SystemExit("a combined answer differs from the baseline's")


if __name__ == "__main__":
    main()
