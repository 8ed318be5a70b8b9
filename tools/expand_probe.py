"""BuildTree in batches: the device call against the host walks, host to host.
    python tools/expand_probe.py [--scale S] [--requests B] [--sample N] [--reps R] [--host-reps H]
                                 [--device D] [--out PATH]

Two snapshots, one after the other (--scale S divides every size by S):

  rbac     bench.py's config #2 shape (synth.rbac: 10M users, 100k groups, 2M docs, 50M tuples,
           the same seed), as tools/via_probe.py builds it.  Requests: the viewers trees of B
           documents drawn uniformly (default 1024), roots docs:d#viewer, no depth limit.
  folders  synth.folders at a tenth of config #3 (1M users, 10k groups, 2M folders, 50M tuples):
           nested folders, so deeper trees.  Requests: the roots of its first B check requests.

On each, over the same B roots, host wall time from call to return, host memory to host memory:

  device       ketogpu_subjects_expand with capacity = what the call needs (known in advance)
  count_only   the same call with capacity 0: one walk instead of two, nothing copied back
  twin_1       ketogpu_snapshot_expand_ids looped over the roots on one thread (arrays freed)
  twin_16      ... on 16 threads (the library call releases the interpreter's lock)
  expand       ketogpu_expand looped over the same roots as subjects: the tree with strings

The device calls run R timed rounds (default 30) after 3 warm-up rounds, the host loops H
(default 5) after one.  A sample of N roots (default 64, fixed seed) is checked against the
host twin word for word in both arrays, with count and status; every root's count is checked
against the twin's tree size.  Writes one JSON document (default profiles/expand/probe.json)
and prints it; exits non-zero on a difference.  No speed-up is asserted: a one-wave depth-first
walk is bound by latency on chains, and the document says who won on each shape."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(ms):
    return {"reps": len(ms), "ms_per_call_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def timed(call, reps, warm):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stat(ms)


def probe(snap, roots, subjects, a, note):
    from keto_amd import _lib as L
    from keto_amd import expand
    ALL = L.EXPAND_DEPTH_ALL
    lib = L.lib()
    host = expand.Engine(snap)
    depths = np.full(len(roots), ALL, dtype=np.uint32)

    def twin_size(r):
        nodes, kids, n, flags = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        rc = lib.ketogpu_snapshot_expand_ids(snap.h, int(r), ALL, C.byref(nodes), C.byref(kids), C.byref(n),
                                             C.byref(flags))
        lib.ketogpu_free(nodes), lib.ketogpu_free(kids)
        return -1 if rc or flags.value else int(n.value)

    def twin_chunk(chunk):
        return [twin_size(r) for r in chunk]

    pool = ThreadPoolExecutor(16)
    chunks = np.array_split(roots, 64)

    def expand_loop():
        return [host.tree_size(s, 2**31 - 1) for s in subjects]

    with expand.DeviceEngine(snap) as dev:
        *_, count0, status0, need = dev.expand_ids_raw(roots, depths, 0)
        before = dev.expand_stats()
        nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, need)
        after = dev.expand_stats()
        sizes = twin_chunk(roots)
        ok = needed == need and np.array_equal(count, count0) and np.array_equal(status, status0)
        for i, sz in enumerate(sizes):  # every count against the twin's tree size
            ok = ok and (status[i] == L.EXPAND_HOST if sz < 0 else int(count[i]) == sz)
        sample = np.sort(np.random.default_rng(11).choice(len(roots), min(a.sample, len(roots)), replace=False))
        for i in sample:
            if sizes[i] <= 0:
                continue
            wn, wk, _ = host.expand_ids(int(roots[i]), ALL)
            b, c = int(begin[i]), int(count[i])
            ok = ok and status[i] == L.EXPAND_OK and np.array_equal(nodes[b:b + c], wn) and \
                np.array_equal(kids[b:b + c], wk)
        res = {"requests": int(len(roots)), "nodes_per_call": int(need), "largest_tree": int(count.max()),
               "unions_per_call": int((kids > 0).sum()), "host_status_requests": int((status == L.EXPAND_HOST).sum()),
               **{k: int(after[k] - before[k]) for k in ("tier1_requests", "tier2_requests", "tier2_rounds")},
               "slots": after["slots"], "sample_checked": int(len(sample)), "equals_the_host_twin": bool(ok)}
        note(f"  {need} nodes per call, largest tree {res['largest_tree']}, tier 2 {res['tier2_requests']}, "
             f"equal to the host twin: {ok}")
        res["device"] = timed(lambda: dev.expand_ids_raw(roots, depths, need), a.reps, 3)
        res["count_only"] = timed(lambda: dev.expand_ids_raw(roots, depths, 0), a.reps, 3)
    res["twin_1"] = timed(lambda: twin_chunk(roots), a.host_reps, 1)
    res["twin_16"] = timed(lambda: list(pool.map(twin_chunk, chunks)), a.host_reps, 1)
    res["expand"] = timed(expand_loop, a.host_reps, 1)
    pool.shutdown()
    med = lambda k: res[k]["ms_per_call_median"]
    res["twin_1_over_device"] = round(med("twin_1") / med("device"), 2)
    res["twin_16_over_device"] = round(med("twin_16") / med("device"), 2)
    res["expand_over_device"] = round(med("expand") / med("device"), 2)
    res["fastest"] = min(("device", "twin_1", "twin_16", "expand"), key=med)
    note(f"  device {med('device')} ms, count only {med('count_only')} ms, twin x1 {med('twin_1')} ms, "
         f"twin x16 {med('twin_16')} ms, ketogpu_expand {med('expand')} ms")
    return res, bool(ok)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide every size by this")
    p.add_argument("--requests", type=int, default=1024, help="B: trees per call")
    p.add_argument("--sample", type=int, default=64, help="N: trees compared word for word")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--host-reps", type=int, default=5)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand", "probe.json"))
    a = p.parse_args()
    from keto_amd import _lib as L
    from keto_amd import lookup, synth
    from keto_amd import relationtuple as rt
    from keto_amd.snapshot import Snapshot

    note = lambda *x: print(*x, file=sys.stderr, flush=True)  # progress; the result alone goes to stdout
    s = max(a.scale, 1)
    res, all_ok = {}, True
    shapes = (
        ("rbac", "config #2 (synth.rbac)", synth.rbac,
         dict(users=10_000_000 // s, groups=100_000 // s, docs=2_000_000 // s, tuples=50_000_000 // s, checks=1024)),
        ("folders", "a tenth of config #3 (synth.folders)", synth.folders,
         dict(users=1_000_000 // s, groups=10_000 // s, folders=2_000_000 // s, tuples=50_000_000 // s,
              checks=max(a.requests, 1024))))
    for name, shape, make, sizes in shapes:
        t0 = time.perf_counter()
        w = make(**sizes, seed=synth.SEED)
        snap = Snapshot.from_columns(w.namespaces, w.columns)
        build_s = time.perf_counter() - t0
        st = snap.stats()
        note(f"{name}: snapshot built in {build_s:.1f} s: {st['num_nodes']} nodes, {st['num_edges']} edges")
        if name == "rbac":
            rng = np.random.default_rng(synth.SEED)  # the documents of tools/subjects_probe.py
            objects = [("docs", f"d{int(d)}", "viewer") for d in rng.integers(0, sizes["docs"], a.requests)]
        else:
            objects = [(ns, o, r) for ns, o, r, _ in w.requests(range(a.requests))]
        ids = lookup.resolve_roots(snap, objects)
        keep = ids != L.NODE_NONE
        roots = np.ascontiguousarray(ids[keep], dtype=np.uint32)
        subjects = [rt.SubjectSet(*o) for o, k in zip(objects, keep) if k]
        block, ok = probe(snap, roots, subjects, a, note)
        all_ok = all_ok and ok
        res[name] = {"workload": {"shape": shape, "scale_divisor": s, **sizes, "seed": synth.SEED,
                                  "snapshot_build_s": round(build_s, 2),
                                  **{k: st[k] for k in ("num_nodes", "num_expandable", "num_interior", "num_edges")},
                                  "roots_without_rows_dropped": int((~keep).sum())}, **block}
        del snap, w
    res["rest_depth"] = "no limit"
    res["ok"] = all_ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
