"""BuildTree with the copying spread over the chip (ketogpu_subjects_expand_wide,
keto_amd/csrc/expand_wide.hpp) against the host twin ketogpu_snapshot_expand_ids and against the
plain device call: the trees word for word in both arrays; count, status, begin and needed exact
(tests/expand_wide_cases.py assert_device_wide).  Every test runs under the default tiers and
with KETOGPU_SUBJECTS_TIER=2, which sends every walked request to the plain call's tier 2."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import expand, lookup
from keto_amd.snapshot import Snapshot
from tests import expand_cases as EC
from tests import expand_wide_cases as WC
from tests import lookup_cases as LC

pytestmark = pytest.mark.gpu

ALL = WC.ALL
SENTINEL = 0xDEADBEEF
QUEUE = ("run_steps", "skipped_entries", "runs_queued", "items_queued", "runs_self_copied", "runs_queue_full")


@pytest.fixture(params=["default", "tier2"])
def tiers(request, monkeypatch):
    if request.param == "tier2":
        monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    else:
        monkeypatch.delenv("KETOGPU_SUBJECTS_TIER", raising=False)
    return request.param


def same(a, b):
    if isinstance(a, expand.NotFound) or isinstance(b, expand.NotFound):
        return isinstance(a, expand.NotFound) and isinstance(b, expand.NotFound) and str(a) == str(b)
    return (a.to_node() if a else None) == (b.to_node() if b else None)


def host_answers(ex, subjects, depths):
    res = []
    for s, d in zip(subjects, depths):
        try:
            res.append(ex.BuildTree(s, d))
        except expand.NotFound as e:
            res.append(e)
    return res


def moved(dev, before, keys=QUEUE):
    st = dev.expand_wide_stats()
    return {k: st[k] - before[k] for k in keys}


@pytest.mark.parametrize("table", LC.TABLES, ids=lambda t: f"seed{t[0]}")
def test_truth_tables_every_node_as_root(table, tiers):
    _, _, snap = LC.table(*table)
    ex = expand.Engine(snap)
    n = snap.stats()["num_nodes"]
    roots = np.tile(np.arange(n, dtype=np.uint32), 4)
    depths = np.repeat(np.array([1, 2, 3, ALL], dtype=np.uint32), n)
    with expand.DeviceEngine(snap) as dev:
        status = WC.assert_device_wide(dev, ex, roots, depths)  # (HOST iff the twin's NEEDS_HOST: inside)
        host = int((status == L.EXPAND_HOST).sum())
        if not table[4]:  # tables 31 and 41: no poison
            assert host == 0
        else:  # 42 and 43
            assert 0 < host < len(roots)
        st = dev.expand_wide_stats()
        assert st["requests"] == 2 * len(roots) and st["host_requests"] == 2 * host and st["mask_builds"] == 1
        if tiers == "tier2":
            assert st["tier2_requests"] > 0 and st["tier2_rounds"] > 0
        else:
            assert st["tier1_requests"] > 0
        # through the wrapper every answer is Engine.BuildTree's, errors included
        subjects = [snap.describe(v) for v in range(n)]
        for d in (2, 2**31 - 1):
            got = dev.build_trees_batch(subjects, [d] * n, wide=True)
            for s, g, w in zip(subjects, got, host_answers(ex, subjects, [d] * n)):
                assert same(g, w), (s, d)
        for s, g in zip(subjects, dev.build_trees_json_batch(subjects, [3] * n, wide=True)):
            try:
                assert g == ex.build_tree_json(s, 3), s
            except expand.NotFound as e:
                assert isinstance(g, expand.NotFound) and str(g) == str(e), s
        assert same(dev.BuildTree(subjects[0], 3, wide=True), host_answers(ex, subjects[:1], [3])[0])
        assert dev.expand_wide_stats()["requests"] > st["requests"] and dev.expand_stats()["requests"] == len(roots)


def test_runs_of_the_new_graph(tiers):
    snap = WC.graph()
    ex = expand.Engine(snap)
    roots = WC.roots(snap)
    bad = list(WC.root_names()).index("wbad")
    with expand.DeviceEngine(snap) as dev:
        for d in (2, 3, ALL):
            status = WC.assert_device_wide(dev, ex, roots, d)
            assert status[bad] == L.EXPAND_HOST and (np.delete(status, bad) == L.EXPAND_OK).all()
            # the same two calls once more, for what each of them counts
            s0 = dev.expand_wide_stats()
            *_, needed = dev.expand_ids_raw(roots, d, 0, wide=True)
            counting = moved(dev, s0)
            s1 = dev.expand_wide_stats()
            dev.expand_ids_raw(roots, d, needed, wide=True)
            writing = moved(dev, s1)
            if tiers == "tier2":
                assert not any(counting.values()) and not any(writing.values())
                continue
            assert counting["run_steps"] > 0 and counting["skipped_entries"] >= sum(WC.LEAF_ROWS) + WC.FAN * (d != 2)
            assert not any(counting[k] for k in QUEUE[2:])  # a count-only call queues and copies nothing
            # a writing call walks every tree twice, in the same steps (the HOST request once, both times)
            runs = writing["run_steps"] - counting["run_steps"]
            assert runs > 0 and writing["items_queued"] > 0
            assert writing["runs_queued"] + writing["runs_self_copied"] == runs
            assert writing["items_queued"] >= writing["runs_queued"] and writing["runs_queue_full"] == 0
            assert writing["skipped_entries"] <= 2 * counting["skipped_entries"]
        st = dev.expand_wide_stats()
        assert st["mask_builds"] == 1 and st["mask_words"] > 0 and st["queue_capacity"] > 1
        assert st["chunk"] == dev.subjects.wide_stats()["chunk"] < WC.WINDOW  # a full window is several items
        assert st["tier2_requests" if tiers == "default" else "tier1_requests"] == 0


def test_fan_at_the_set_capacity(tiers):
    snap = EC.fans()
    ex = expand.Engine(snap)
    fits, over = EC.node_of(snap, WC.view("Atop")), EC.node_of(snap, WC.view("Btop"))
    with expand.DeviceEngine(snap) as dev:
        for d in (2, 3):  # children marked at the limit, and children opened
            for root, opened in ((fits, EC.SET_CAP), (over, EC.SET_CAP + 1)):
                before = dev.expand_wide_stats()
                assert (WC.assert_device_wide(dev, ex, [root], d) == L.EXPAND_OK).all()
                st = dev.expand_wide_stats()
                t2 = 2 if tiers == "tier2" or opened > EC.SET_CAP else 0
                assert st["tier2_requests"] - before["tier2_requests"] == t2, (d, opened)
                assert st["tier1_requests"] - before["tier1_requests"] == 2 - t2, (d, opened)
                if t2:
                    assert st["items_queued"] == before["items_queued"] and st["slots"] >= 1


def test_a_full_queue_is_copied_by_the_walk(tiers, monkeypatch):
    monkeypatch.setenv("KETOGPU_EXPAND_WIDE_QUEUE", "1")
    snap = WC.graph()
    ex = expand.Engine(snap)
    roots = WC.roots(snap)
    with expand.DeviceEngine(snap) as dev:
        before = dev.expand_wide_stats()
        assert before["queue_capacity"] == 1
        for d in (3, ALL):
            WC.assert_device_wide(dev, ex, roots, d)
        got = moved(dev, before)
        if tiers == "default":
            assert got["runs_queue_full"] > 0 and got["items_queued"] <= 2
            assert got["runs_self_copied"] >= got["runs_queue_full"]
        else:
            assert not any(got.values())


def _sentinels(n):
    return np.full(n, SENTINEL, dtype=np.uint32), np.full(n, SENTINEL, dtype=np.uint32)


def test_truncation(tiers):
    snap = WC.graph()
    ex = expand.Engine(snap)
    roots = np.array([EC.node_of(snap, WC.view(x)) for x in ("WL4097_r", "wdm", "wfan", "WP63_r", "WT200_r", "wres077")],
                     dtype=np.uint32)
    depths = np.full(len(roots), ALL, dtype=np.uint32)
    want = [EC.twin(ex, r, ALL) for r in roots]
    total = sum(len(w[1]) for w in want)
    assert total > WC.FAN
    with expand.DeviceEngine(snap) as dev:
        before = dev.expand_wide_stats()["truncated_trees"]
        cap = total - 1
        out = _sentinels(cap)
        nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, cap, wide=True, out=out)
        assert np.shares_memory(nodes, out[0]) and np.shares_memory(kids, out[1])
        assert needed == total and [int(c) for c in count] == [len(w[1]) for w in want]
        cut = [i for i in range(len(roots)) if begin[i] == L.LOOKUP_TRUNCATED]
        assert len(cut) == 1 and (status == L.EXPAND_OK).all()
        written = np.zeros(cap, dtype=bool)
        for i, (_, wn, wk, _) in enumerate(want):
            if i in cut:
                continue
            b = int(begin[i])
            assert (nodes[b:b + len(wn)] == wn).all() and (kids[b:b + len(wn)] == wk).all()
            assert not written[b:b + len(wn)].any()
            written[b:b + len(wn)] = True
        assert (nodes[~written] == SENTINEL).all() and (kids[~written] == SENTINEL).all()
        assert dev.expand_wide_stats()["truncated_trees"] == before + 1
        # with room to spare, nothing behind the trees is touched
        cap = total + 100
        out = _sentinels(cap)
        nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, cap, wide=True, out=out)
        assert needed == total and (begin != L.LOOKUP_TRUNCATED).all()
        for i, (_, wn, wk, _) in enumerate(want):
            b = int(begin[i])
            assert (nodes[b:b + len(wn)] == wn).all() and (kids[b:b + len(wn)] == wk).all()
        assert (out[0][total:] == SENTINEL).all() and (out[1][total:] == SENTINEL).all()
        assert dev.expand_wide_stats()["truncated_trees"] == before + 1


def test_writes_are_seen_by_the_next_call(tiers):
    rows = [LC.sset("doc", "view", f"x{i:03d}", "member") for i in range(500)]
    rows += [LC.sid("x250", "member", "alice"), LC.sid("x400", "member", "bob"), LC.sid("x400", "member", "carol")]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    ex = expand.Engine(snap)
    roots = [EC.node_of(snap, s) for s in (WC.view("doc"), EC.member("x250"), EC.member("x400"))]
    with expand.DeviceEngine(snap) as dev:

        def check(first):
            """the wide call against the twin; the mask is rebuilt by the first call behind a write only"""
            builds = dev.expand_wide_stats()["mask_builds"]
            *_, needed = dev.expand_ids_raw(roots, ALL, 0, wide=True)
            assert dev.expand_wide_stats()["mask_builds"] == builds + first
            for d in (2, ALL):
                WC.assert_device_wide(dev, ex, roots, d)
            assert dev.expand_wide_stats()["mask_builds"] == builds + first
            return needed

        size = check(1)
        assert size == 501 + 3 + 2 + 3
        # a set loses its last row: x250 turns into a leaf inside the run
        assert snap.write(delete_rows=[LC.sid("x250", "member", "alice")])["applied"]
        assert check(1) == size - 3 and check(0) == size - 3
        # ... and gets its first row again
        assert snap.write(insert_rows=[LC.sid("x250", "member", "dave"), LC.sid("x250", "member", "erin")])["applied"]
        assert check(1) == size + 2 and check(0) == size + 2
        # an insert in the middle of the long run
        assert snap.write(insert_rows=[LC.sset("doc", "view", "x100a", "member")])["applied"]
        assert check(1) == size + 3 and check(0) == size + 3
        a, _, _ = ex.expand_ids(roots[0], ALL)
        assert len(a) == 506 and a[102] == EC.node_of(snap, EC.member("x100a"))
        assert dev.subjects.refresh_stats()["patched_refreshes"] >= 1
        assert same(dev.BuildTree(WC.view("doc"), 10, wide=True), ex.BuildTree(WC.view("doc"), 10))


def test_statistics_stay_put(tiers):
    snap = WC.graph()
    ex = expand.Engine(snap)
    roots = [EC.node_of(snap, WC.view(x)) for x in ("wdm", "wfan", "WP129_r")]
    drop = lambda d: {k: v for k, v in d.items() if k != "last_call_ms"}
    with lookup.Subjects(snap) as sj:
        sj.subject_ids(roots)
        dev = expand.DeviceEngine(snap, subjects=sj)
        dev.expand_ids_raw(roots, ALL, 0)
        others = (sj.stats, sj.depth_stats, sj.via_stats, sj.combine_stats, sj.wide_stats, dev.expand_stats)
        before = [drop(f()) for f in others]
        *_, needed = dev.expand_ids_raw(roots, ALL, 0, wide=True)
        dev.expand_ids_raw(roots, ALL, needed, wide=True)
        assert [drop(f()) for f in others] == before
        wide = dev.expand_wide_stats()
        assert wide["requests"] == 6 and wide["nodes_produced"] == 2 * needed
        # ... and a plain call moves no wide expand statistic
        dev.expand_ids_raw(roots, ALL, needed)
        assert dev.expand_wide_stats() == wide and dev.expand_stats()["requests"] == before[5]["requests"] + 3
        # the state the wide call left behind serves a listing unchanged
        want = [lookup.host_subjects(snap, r) for r in roots]
        assert all((np.sort(g) == w).all() for g, w in zip(sj.subject_ids(roots), want))
        WC.assert_device_wide(dev, ex, roots, ALL)
        dev.close()
        assert sj.h  # a handle that was passed in stays open


def test_kept_out_arrays(tiers):
    snap = WC.graph()
    roots = [EC.node_of(snap, WC.view(x)) for x in ("wfan", "WT10_r", "wgdup", "wres129")]
    with expand.DeviceEngine(snap) as dev:
        *_, needed = dev.expand_ids_raw(roots, ALL, 0, wide=True)
        for wide in (True, False):
            fresh = dev.expand_ids_raw(roots, ALL, needed, wide=wide)
            kept = _sentinels(needed + 7)
            for depths in (2, ALL):  # the second call overwrites what the first left
                got = dev.expand_ids_raw(roots, depths, needed, wide=wide, out=kept)
            assert np.shares_memory(got[0], kept[0]) and np.shares_memory(got[1], kept[1])
            assert got[5] == fresh[5] == needed and (got[3] == fresh[3]).all() and (got[4] == fresh[4]).all()
            for i in range(len(roots)):
                a, b = WC.tree_of(got[:2], got[2], got[3], i), WC.tree_of(fresh[:2], fresh[2], fresh[3], i)
                assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
            assert (kept[0][needed:] == SENTINEL).all() and (kept[1][needed:] == SENTINEL).all()
