"""Chip-wide BuildTree: ketogpu_subjects_expand_wide against ketogpu_subjects_expand and the host
walks, host to host.
    python tools/expand_wide_probe.py [--scale S] [--requests B] [--sample N] [--reps R] [--host-reps H]
                                      [--writes W] [--device D] [--out PATH]

The two snapshots and the requests of tools/expand_probe.py (--scale S divides every size by S):

  rbac     bench.py's config #2 shape; the viewers trees of B documents (default 1024), no depth
           limit.  Long rows of users: nearly everything is a run of leaves.
  folders  synth.folders at a tenth of config #3; the roots of its first B check requests.  Rows
           of folders that open with short runs of users between them: little to hand to the
           fill kernel, the wide call should cost no more than the plain one.

On each, over the same B roots, host wall time from call to return, host memory to host memory.
The plain and the wide call alternate within one loop, R timed rounds (default 30) after 3
warm-up rounds, so both see the same machine:

  fresh        the writing call (capacity = what it needs) into arrays allocated per call, as
               expand_ids_raw does by default: the first touch of their pages is in the time
  kept         the same call with out= arrays kept across the calls
  count_only   capacity 0: one walk, nothing copied back
  twin_1 / twin_16   ketogpu_snapshot_expand_ids looped over the roots on 1 / 16 threads, H rounds
                     (default 5) after one, in the same run

Then the same data as a writable snapshot (the handle's rows lie in its arena then): the first
wide call behind a single-tuple write, which patches one row and rebuilds the mask
(last_mask_ms, and the call's time next to the calls before and after it), W writes (default 5).

Every tree's count is checked against the twin's tree size and a sample of N roots (default 64,
fixed seed) word for word in both arrays, for both calls, with fresh and with kept arrays.  Writes
one JSON document (default profiles/expand_wide/probe.json) and prints it; exits non-zero on a
difference.  No speed is asserted: the document says who won on each shape, and says LOSES."""
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
    return alternating({"x": call}, reps, warm)["x"]


def alternating(calls, reps, warm):
    """the calls in turn, round after round -> {name: stat}"""
    ms = {k: [] for k in calls}
    for r in range(warm + reps):
        for k, call in calls.items():
            t0 = time.perf_counter()
            call()
            if r >= warm:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stat(v) for k, v in ms.items()}


def verdict(ours, theirs, spread=None):
    """who won, by the medians; within `spread` (the other's min .. max) it is a tie"""
    a, b = ours["ms_per_call_median"], theirs["ms_per_call_median"]
    if spread and theirs["ms_min"] <= a <= theirs["ms_max"]:
        return "within the other's run-to-run spread"
    return "wins" if a < b else "LOSES"


def probe(snap, roots, a, note):
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
    with expand.DeviceEngine(snap) as dev:
        *_, count0, status0, need = dev.expand_ids_raw(roots, depths, 0, wide=True)
        kept = {w: (np.zeros(max(need, 1), np.uint32), np.zeros(max(need, 1), np.uint32)) for w in (False, True)}
        sizes = twin_chunk(roots)
        sample = np.sort(np.random.default_rng(11).choice(len(roots), min(a.sample, len(roots)), replace=False))
        want = {int(i): host.expand_ids(int(roots[i]), ALL)[:2] for i in sample if sizes[i] > 0}
        ok = True
        before = dev.expand_wide_stats()
        for wide in (True, False):
            for out in (None, kept[wide]):
                nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, need, wide=wide, out=out)
                good = needed == need and np.array_equal(count, count0) and np.array_equal(status, status0)
                for i, sz in enumerate(sizes):  # every count against the twin's tree size
                    good = good and (status[i] == L.EXPAND_HOST if sz < 0 else int(count[i]) == sz)
                for i, (wn, wk) in want.items():
                    b, c = int(begin[i]), int(count[i])
                    good = good and status[i] == L.EXPAND_OK and np.array_equal(nodes[b:b + c], wn) and \
                        np.array_equal(kids[b:b + c], wk)
                ok = ok and bool(good)
                if wide and out is None:
                    after = dev.expand_wide_stats()
        per_call = {k: int(after[k] - before[k]) for k in (
            "tier1_requests", "tier2_requests", "run_steps", "skipped_entries", "runs_queued", "items_queued",
            "runs_self_copied", "runs_queue_full")}
        res = {"requests": int(len(roots)), "nodes_per_call": int(need), "largest_tree": int(count0.max()),
               "host_status_requests": int((status0 == L.EXPAND_HOST).sum()), "wide_writing_call": per_call,
               "mask_words": int(after["mask_words"]), "mask_bytes": int(after["mask_words"]) * 8,
               "first_mask_ms": round(after["last_mask_ms"], 4), "queue_capacity": int(after["queue_capacity"]),
               "chunk": int(after["chunk"]), "sample_checked": len(want), "equals_the_host_twin": bool(ok)}
        note(f"  {need} nodes per call, largest tree {res['largest_tree']}, per wide writing call {per_call}, "
             f"equal to the host twin: {ok}")
        call = lambda wide, cap, out=None: (lambda: dev.expand_ids_raw(roots, depths, cap, wide=wide, out=out))
        fresh = alternating({"plain": call(False, need), "wide": call(True, need)}, a.reps, 3)
        keep = alternating({"plain": call(False, need, kept[False]), "wide": call(True, need, kept[True])}, a.reps, 3)
        cnt = alternating({"plain": call(False, 0), "wide": call(True, 0)}, a.reps, 3)
        for w in ("plain", "wide"):
            res[w] = {"fresh": fresh[w], "kept": keep[w], "count_only": cnt[w]}
    res["twin_1"] = timed(lambda: twin_chunk(roots), a.host_reps, 1)
    res["twin_16"] = timed(lambda: list(pool.map(twin_chunk, chunks)), a.host_reps, 1)
    pool.shutdown()
    med = lambda d: d["ms_per_call_median"]
    res["wide_kept_against_twin_16"] = verdict(res["wide"]["kept"], res["twin_16"])
    res["wide_fresh_against_twin_16"] = verdict(res["wide"]["fresh"], res["twin_16"])
    res["plain_kept_against_twin_16"] = verdict(res["plain"]["kept"], res["twin_16"])
    res["wide_kept_against_plain_kept"] = verdict(res["wide"]["kept"], res["plain"]["kept"], spread=True)
    res["wide_count_only_against_plain"] = verdict(res["wide"]["count_only"], res["plain"]["count_only"], spread=True)
    res["plain_kept_over_wide_kept"] = round(med(res["plain"]["kept"]) / med(res["wide"]["kept"]), 2)
    res["twin_16_over_wide_kept"] = round(med(res["twin_16"]) / med(res["wide"]["kept"]), 2)
    for w in ("plain", "wide"):
        note(f"  {w}: fresh {med(res[w]['fresh'])} ms, kept {med(res[w]['kept'])} ms, count only "
             f"{med(res[w]['count_only'])} ms")
    note(f"  twin x1 {med(res['twin_1'])} ms, twin x16 {med(res['twin_16'])} ms; wide with kept arrays "
         f"{res['wide_kept_against_twin_16']} against twin x16")
    return res, bool(ok)


def probe_writes(snap, roots, namespaces, objects, a, note):
    """the first wide call behind a single-tuple write, on a writable snapshot"""
    from keto_amd import _lib as L
    from keto_amd import expand
    depths = np.full(len(roots), L.EXPAND_DEPTH_ALL, dtype=np.uint32)
    ns_id = dict(namespaces)
    host = expand.Engine(snap)
    with expand.DeviceEngine(snap) as dev:
        *_, need = dev.expand_ids_raw(roots, depths, 0, wide=True)
        cap = need + 1024
        out = (np.zeros(cap, np.uint32), np.zeros(cap, np.uint32))
        call = lambda: dev.expand_ids_raw(roots, depths, cap, wide=True, out=out)
        steady = timed(call, 5, 2)
        first, second, mask, refresh, ok = [], [], [], [], True
        for k in range(a.writes):
            ns, obj, rel = objects[k % len(objects)]
            r = snap.write([(ns_id[ns], obj, rel, f"wide-probe-user-{k}", None, None, None)], [])
            if not r["applied"]:
                note(f"  write {k} refused: {r['reason']}")
                continue
            builds = dev.expand_wide_stats()["mask_builds"]
            t0 = time.perf_counter()
            nodes, kids, begin, count, status, _ = call()
            first.append((time.perf_counter() - t0) * 1e3)
            st = dev.expand_wide_stats()
            ok = ok and st["mask_builds"] == builds + 1
            mask.append(st["last_mask_ms"]), refresh.append(dev.subjects.refresh_stats()["last_refresh_ms"])
            i = k % len(objects)  # the written tree against the twin
            wn, wk, _ = host.expand_ids(int(roots[i]), L.EXPAND_DEPTH_ALL)
            b, c = int(begin[i]), int(count[i])
            ok = ok and np.array_equal(nodes[b:b + c], wn) and np.array_equal(kids[b:b + c], wk)
            t0 = time.perf_counter()
            call()
            second.append((time.perf_counter() - t0) * 1e3)
            ok = ok and dev.expand_wide_stats()["mask_builds"] == builds + 1
        rs = dev.subjects.refresh_stats()
        res = {"writes_applied": len(first), "steady_call": steady, "mask_words": int(dev.expand_wide_stats()["mask_words"]),
               "patched_refreshes": int(rs["patched_refreshes"]), "full_uploads": int(rs["full_uploads"]),
               "equal_and_one_rebuild_per_write": bool(ok)}
        if first:
            res.update(first_call_after_write=stat(first), next_call=stat(second), last_mask_ms=stat(mask),
                       last_refresh_ms=stat(refresh))
        note(f"  writes: {res}")
    return res, bool(ok) and bool(first)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=1, help="divide every size by this")
    p.add_argument("--requests", type=int, default=1024, help="B: trees per call")
    p.add_argument("--sample", type=int, default=64, help="N: trees compared word for word")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--host-reps", type=int, default=5)
    p.add_argument("--writes", type=int, default=5, help="W: single-tuple writes (0: no writable snapshot)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_wide", "probe.json"))
    a = p.parse_args()
    from keto_amd import _lib as L
    from keto_amd import lookup, synth
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
        w = make(**sizes, seed=synth.SEED)
        if name == "rbac":
            rng = np.random.default_rng(synth.SEED)  # the documents of tools/subjects_probe.py
            objects = [("docs", f"d{int(d)}", "viewer") for d in rng.integers(0, sizes["docs"], a.requests)]
        else:
            objects = [(ns, o, r) for ns, o, r, _ in w.requests(range(a.requests))]
        for writable in (False, True) if a.writes else (False,):
            t0 = time.perf_counter()
            snap = Snapshot.from_columns(w.namespaces, w.columns, writable=writable)
            build_s = time.perf_counter() - t0
            st = snap.stats()
            note(f"{name}{' (writable)' if writable else ''}: snapshot built in {build_s:.1f} s: {st['num_nodes']} "
                 f"nodes, {st['num_edges']} edges")
            ids = lookup.resolve_roots(snap, objects)
            keep = ids != L.NODE_NONE
            roots = np.ascontiguousarray(ids[keep], dtype=np.uint32)
            if not writable:
                block, ok = probe(snap, roots, a, note)
                res[name] = {"workload": {"shape": shape, "scale_divisor": s, **sizes, "seed": synth.SEED,
                                          "snapshot_build_s": round(build_s, 2),
                                          **{k: st[k] for k in ("num_nodes", "num_expandable", "num_interior",
                                                                "num_edges")},
                                          "roots_without_rows_dropped": int((~keep).sum())}, **block}
            else:
                block, ok = probe_writes(snap, roots, w.namespaces, [o for o, k in zip(objects, keep) if k], a, note)
                res[name]["after_a_single_tuple_write"] = block
            all_ok = all_ok and ok
            del snap
        del w
    res["rest_depth"] = "no limit"
    res["not_measured"] = ["kernel times (host wall time only)", "other scales and batch sizes", "tier 2",
                           "wider loads or stores in the fill kernel"]
    res["ok"] = all_ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
