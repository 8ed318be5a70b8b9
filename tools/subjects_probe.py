"""Subject listing against the brute-force route, on the config #2 shape.
    python tools/subjects_probe.py [--scale S] [--roots B] [--reps R] [--device D] [--out PATH]

One snapshot of a synth.rbac workload of bench.py's config #2 shape (10M users, 100k groups,
2M docs, 50M tuples, the same seed; --scale S divides every size by S).  B documents drawn
uniformly (default 1024), roots docs:d#viewer, class SUBJECT_ID ("which users").

  listing      Subjects.subject_ids_raw over the B roots with capacity = needed (taken from one
               count-only call), 30 timed calls after 3 warm-up calls, host wall time from call
               to return: median and min-max ms per call, lists/s, ids/s, the largest list, the
               tier split and tier 2's list / scan finish split.
  list_cap_0   the same calls on a second handle created under KETOGPU_SUBJECTS_LIST_CAP=0
               (every tier-2 finish scans the bitmap), in the same process, its timed calls
               alternating with the default handle's.
  count_only   10 calls of the default handle with capacity 0: the same closures and counts,
               nothing written and no ids copied back.
  brute force  the route a caller has without the listing: every user node as target against
               ONE document root as a device-resident batch (ketogpu_queries_upload / _run /
               _download), in the same process on the same device.  Timed for 4 of the
               documents (median of 5 runs each after one warm-up run; the run alone, and
               upload + run + download) and multiplied out to B.  The 4 answers are compared id
               for id with the listing's.

Writes one JSON document (default profiles/subjects/probe.json) and prints it; exits non-zero
when a brute-force answer differs from the listing's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def user_nodes(snap, n_users, chunk=1 << 21):
    """the node ids of the subject ids u0 .. u{n_users - 1} that some tuple names, ascending
    (request columns built with numpy: no per-user Python objects are kept)"""
    from keto_amd import _lib as L
    const = lambda s, n: (np.frombuffer(s * n, dtype=np.uint8).copy(),
                          (np.arange(n + 1, dtype=np.uint64) * len(s)))
    empty = lambda n: (np.zeros(1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64))
    found = []
    for lo in range(0, n_users, chunk):
        hi = min(lo + chunk, n_users)
        n = hi - lo
        ids = np.arange(lo, hi, dtype=np.int64)
        digits = np.ones(n, dtype=np.uint64)
        for p in range(1, 19):
            digits += ids >= 10 ** p
        cols = {"n": n, "subject_kind": np.zeros(n, dtype=np.uint8)}
        cols["ns_data"], cols["ns_off"] = const(b"-", n)
        cols["obj_data"], cols["obj_off"] = const(b"-", n)
        cols["rel_data"], cols["rel_off"] = const(b"-", n)
        cols["sid_data"] = np.frombuffer("".join(f"u{i}" for i in range(lo, hi)).encode(), dtype=np.uint8).copy()
        cols["sid_off"] = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(digits + 1, dtype=np.uint64)])
        for k in ("ss_ns", "ss_obj", "ss_rel"):
            cols[k + "_data"], cols[k + "_off"] = empty(n)
        _, targets, status = snap.resolve_batch(cols)
        assert not status.any()
        found.append(targets[targets != L.NODE_NONE].copy())
    return np.sort(np.concatenate(found)) if found else np.zeros(0, dtype=np.uint32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide config #2's sizes by this")
    p.add_argument("--roots", type=int, default=1024, help="B: documents per listing call")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "subjects", "probe.json"))
    a = p.parse_args()
    from keto_amd import check, lookup, synth
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
    cls = lookup.CLASS_SUBJECT_ID
    rng = np.random.default_rng(synth.SEED)
    docs = rng.integers(0, sizes["docs"], a.roots)
    roots = lookup.resolve_roots(snap, [("docs", f"d{int(d)}", "viewer") for d in docs])
    t0 = time.perf_counter()
    users = user_nodes(snap, sizes["users"])
    resolve_s = time.perf_counter() - t0
    assert len(users) and int(users[0]) >= st["num_expandable"]  # subject ids are never expanded

    sj = lookup.Subjects(snap, device=a.device)
    os.environ["KETOGPU_SUBJECTS_LIST_CAP"] = "0"
    sj0 = lookup.Subjects(snap, device=a.device)
    del os.environ["KETOGPU_SUBJECTS_LIST_CAP"]
    t0 = time.perf_counter()
    _, _, count, needed = sj.subject_ids_raw(roots, cls, 0)
    first_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(3):
        sj.subject_ids_raw(roots, cls, needed)
        sj0.subject_ids_raw(roots, cls, needed)
    before, before0 = sj.stats(), sj0.stats()
    ms, ms0 = [], []
    for _ in range(a.reps):  # the two handles alternate, so drift of the host hits both alike
        t0 = time.perf_counter()
        out, begin, count, needed2 = sj.subject_ids_raw(roots, cls, needed)
        ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        out0, begin0, count0, needed0 = sj0.subject_ids_raw(roots, cls, needed)
        ms0.append((time.perf_counter() - t0) * 1e3)
    after, after0 = sj.stats(), sj0.stats()
    ms_count = []  # the same closures without the writes and the download of the ids
    for _ in range(10):
        t0 = time.perf_counter()
        sj.subject_ids_raw(roots, cls, 0)
        ms_count.append((time.perf_counter() - t0) * 1e3)
    assert needed2 == needed == needed0 and not (begin == lookup.TRUNCATED).any()
    assert (count == count0).all() and not (begin0 == lookup.TRUNCATED).any()
    med, med0 = float(np.median(ms)), float(np.median(ms0))
    note(f"listing: median {med:.3f} ms (list_cap 0: {med0:.3f} ms), {needed} ids per call")
    calls = a.reps

    def block(ms, med, before, after):
        per = lambda k: (after[k] - before[k]) // calls
        return {"reps": a.reps, "ms_per_call_median": round(med, 4), "ms_min": round(min(ms), 4),
                "ms_max": round(max(ms), 4), "lists_per_s": round(a.roots / med * 1e3, 1),
                "ids_per_s": round(needed / med * 1e3, 1),
                "tier1_requests_per_call": per("tier1_requests"), "tier2_requests_per_call": per("tier2_requests"),
                "tier2_rounds_per_call": per("tier2_rounds"), "list_finishes_per_call": per("list_finishes"),
                "scan_finishes_per_call": per("scan_finishes"), "set_capacity": after["set_capacity"],
                "slots": after["slots"], "list_capacity": after["list_capacity"]}

    res = {
        "workload": {"shape": "config #2 (synth.rbac)", "scale_divisor": s, **sizes, "seed": synth.SEED,
                     "snapshot_build_s": round(build_s, 2), **{k: st[k] for k in (
                         "num_nodes", "num_expandable", "num_interior", "num_edges")}},
        "class": "SUBJECT_ID",
        "roots": int(a.roots),
        "ids_per_call": int(needed),
        "largest_list": int(count.max()) if len(count) else 0,
        "first_call_ms": round(first_ms, 3),
        "listing": block(ms, med, before, after),
        "list_cap_0": block(ms0, med0, before0, after0),
        "count_only": {"reps": len(ms_count), "ms_per_call_median": round(float(np.median(ms_count)), 4),
                       "ms_min": round(min(ms_count), 4), "ms_max": round(max(ms_count), 4)},
    }
    # the default stays unless its min-max range lies wholly above the other's
    res["list_capacity_verdict"] = ("scan is faster: the default's range lies wholly above list_cap_0's"
                                    if min(ms) > max(ms0) else "the default list_capacity stays")

    # the brute-force route: every user node against one document root
    eng = check.Engine(snap, device=a.device)
    note("check engine ready")
    run_ms, route_ms, same, timed = [], [], True, []
    for k in [int(x) for x in np.nonzero(count)[0][:4]]:  # documents somebody holds
        rt_ = np.full(len(users), int(roots[k]), dtype=np.uint32)
        q = eng.upload(rt_, users)
        q.run()
        r1, r2 = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            q2 = eng.upload(rt_, users)
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
        brute = users[np.asarray(allowed, dtype=bool)]  # (users is ascending)
        for o, b, c in ((out, begin, count), (out0, begin0, count0)):
            same = same and np.array_equal(brute, np.sort(o[int(b[k]):int(b[k]) + int(c[k])]))
        timed.append({"doc": int(docs[k]), "subjects": int(count[k])})
    res["brute_force"] = {
        "targets_per_doc": int(len(users)), "docs_timed": timed,
        "run_ms_per_doc": [round(x, 4) for x in run_ms], "route_ms_per_doc": [round(x, 4) for x in route_ms],
        "run_ms_for_all_roots": round(float(np.mean(run_ms)) * a.roots, 2),
        "route_ms_for_all_roots": round(float(np.mean(route_ms)) * a.roots, 2),
        "resolve_users_s": round(resolve_s, 2),
        "answers_equal_listing": bool(same and len(timed) > 0),
    }
    res["ratio_run_only_over_listing"] = round(res["brute_force"]["run_ms_for_all_roots"] / med, 2)
    res["ratio_route_over_listing"] = round(res["brute_force"]["route_ms_for_all_roots"] / med, 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not res["brute_force"]["answers_equal_listing"]:
        raise SystemExit("the brute-force answers differ from the listing's")


if __name__ == "__main__":
    main()
