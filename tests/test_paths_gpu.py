"""Why a check is allowed, on the device (ketogpu_lookup_paths, keto_amd/csrc/lookup.hip) against
the host call (ketogpu_snapshot_path), which test_paths_host.py pins against the oracle.  Counts
are compared with the host's; paths are judged valid and shortest by tests/path_cases.py, never
compared node for node: any path with the fewest hops is right."""
import gc

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import path_cases as PC

pytestmark = pytest.mark.gpu
ANY = lookup.TYPE_ANY
NONE = PC.NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["default", "tier2", "tier2_slots3"])
def tiers(request, monkeypatch):
    """handles created while active: the default tiers, every request through tier 2, or tier 2
    with three slots (several rounds, every slot used again and again)"""
    if request.param != "default":
        monkeypatch.setenv("KETOGPU_LOOKUP_TIER", "2")
    if request.param == "tier2_slots3":
        monkeypatch.setenv("KETOGPU_LOOKUP_SLOTS", "3")
    return request.param


def root_of(snap, obj, rel):
    return int(lookup.resolve_roots(snap, [("n", obj, rel)])[0])


def user(snap, u):
    return int(lookup.resolve_subjects(snap, [rt.SubjectID(u)])[0])


def u32(*v):
    return np.array(v, dtype=np.uint32)


def one_path(lk, rows, r, t, nodes):
    """a single pair in a call of its own: `nodes` nodes (0: denied), valid and shortest"""
    out, begin, count, needed = lk.path_ids_raw(u32(r), u32(t), max(nodes, 1))
    assert int(count[0]) == nodes == needed, (int(count[0]), nodes)
    if nodes:
        assert begin[0] == 0
        rows.assert_shortest(out[:nodes], r, t)
    else:
        assert begin[0] == 0  # neither truncated nor invalid
    return out[:nodes]


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_all_pairs_on_the_device(case, tiers):
    snap, rows, roots, targets, want, dists = PC.table_truth(case)
    total = sum(len(w) for w in want)
    with lookup.Lookup(snap) as lk:
        PC.check_raw(rows, roots, targets, want, lk.path_ids_raw(roots, targets, total), dists)
        st, ls = lk.path_stats(), lk.stats()
        assert st["requests"] == len(roots) and st["tier1_requests"] + st["tier2_requests"] == len(roots)
        assert (st["tier2_requests"] == len(roots)) == (tiers != "default")
        assert st["allowed"] == sum(len(w) > 0 for w in want) and st["ids_produced"] == total
        assert st["truncated_lists"] == 0
        if tiers == "tier2_slots3":
            assert ls["slots"] == 3 and st["tier2_rounds"] == (len(roots) + 2) // 3
        # ketogpu_lookup_stats does not move for path calls
        assert ls["requests"] == 0 and ls["tier1_requests"] == 0 and ls["tier2_requests"] == 0
        assert ls["tier2_rounds"] == 0 and ls["ids_produced"] == 0 and ls["uploads"] == 1


@pytest.fixture(scope="module")
def structure():
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows())
    return snap, PC.Rows(snap)


def test_chains_and_the_early_exit(structure):
    snap, rows = structure
    with lookup.Lookup(snap) as lk:
        assert lk.stats()["set_capacity"] == 1024
        moved = lambda a, b: (b["tier1_requests"] - a["tier1_requests"], b["tier2_requests"] - a["tier2_requests"])
        s0 = lk.path_stats()
        # B(ud) has 1000 nodes: the whole chain is walked in tier 1, the longest walk it can make
        one_path(lk, rows, root_of(snap, "e999", "member"), user(snap, "ud"), 1001)
        s1 = lk.path_stats()
        assert moved(s0, s1) == (1, 0)
        # B(uc) has 3000 nodes and the root is its last: tier 2, no depth cutoff
        p = one_path(lk, rows, root_of(snap, "c2999", "member"), user(snap, "uc"), 3001)
        assert len(set(p.tolist())) == 3001
        s2 = lk.path_stats()
        assert moved(s1, s2) == (0, 1)
        # the same B(uc), but the root is in the target's own row: the search ends in tier 1
        one_path(lk, rows, root_of(snap, "c0", "member"), user(snap, "uc"), 2)
        one_path(lk, rows, root_of(snap, "c700", "member"), user(snap, "uc"), 702)
        s3 = lk.path_stats()
        assert moved(s2, s3) == (2, 0)
        one_path(lk, rows, root_of(snap, "c1500", "member"), user(snap, "uc"), 1502)  # past the set: tier 2
        assert moved(s3, lk.path_stats()) == (0, 1)


def test_structure_cases(structure, tiers):
    snap, rows = structure
    with lookup.Lookup(snap) as lk:
        for name, k in (("u65", 65), ("u129", 129)):  # row entries on the 64-entry step boundaries
            t = user(snap, name)
            row = rows.row(t)
            assert len(row) == k
            for pos in (0, 63, 64, k - 1):
                one_path(lk, rows, int(row[pos]), t, 2)
        ya, yb = root_of(snap, "ya", "member"), root_of(snap, "yb", "member")
        assert one_path(lk, rows, ya, ya, 3)[1] == yb  # root = target through the 2-cycle
        one_path(lk, rows, yb, ya, 2)
        one_path(lk, rows, ya, user(snap, "uy"), 2)
        one_path(lk, rows, yb, user(snap, "uy"), 3)
        me = root_of(snap, "self", "member")
        assert one_path(lk, rows, me, me, 2).tolist() == [me, me]
        top, g0 = root_of(snap, "top", "view"), root_of(snap, "g0", "member")
        p = one_path(lk, rows, top, user(snap, "ux"), 4)  # the diamond, through either branch
        assert p[1] in (root_of(snap, "g1", "member"), root_of(snap, "g2", "member")) and p[2] == g0
        one_path(lk, rows, g0, g0, 0)  # no cycle: a node does not reach itself
        lonely = root_of(snap, "lonely", "view")
        one_path(lk, rows, top, lonely, 0)  # an empty reverse row
        one_path(lk, rows, top, user(snap, "uc"), 0)  # another part of the graph
        one_path(lk, rows, root_of(snap, "c5", "member"), user(snap, "ud"), 0)


def test_exhausted_searches_at_the_set_boundary():
    """denied pairs run the closure to its end: B(t) of set_capacity nodes stays in tier 1, one
    more overflows"""
    table = []
    for k in (1024, 1025):
        table += LC.split_star_rows(f"split{k}", k, f"b{k}_")
    table += [LC.sid("other", "view", "someone")]
    snap = Snapshot.from_rows(LC.NS1, table)
    rows = PC.Rows(snap)
    other = root_of(snap, "other", "view")
    with lookup.Lookup(snap) as lk:
        for k in (1024, 1025):
            t = user(snap, f"split{k}")
            assert len(rows.distances(t)) == k and other not in rows.distances(t)
            before = lk.path_stats()
            one_path(lk, rows, other, t, 0)
            after = lk.path_stats()
            assert after["tier1_requests"] - before["tier1_requests"] == (1 if k == 1024 else 0)
            assert after["tier2_requests"] - before["tier2_requests"] == (0 if k == 1024 else 1)
            # and a member found after the set is nearly full: through a group, three nodes
            one_path(lk, rows, root_of(snap, f"b{k}_d{k - 3}", "view"), t, 3)
        assert lk.path_stats()["allowed"] == 2


def test_truncation_protocol(tiers):
    snap, rows, roots, targets, want, dists = PC.table_truth(LC.TABLES[1])
    sel = np.nonzero([len(w) > 0 for w in want])[0]
    sel = np.sort(np.concatenate([sel, np.arange(0, len(want), 97)]))  # the allowed pairs and some denied
    roots, targets, want = roots[sel], targets[sel], [want[k] for k in sel]
    counts = [len(w) for w in want]
    total = sum(counts)
    with lookup.Lookup(snap) as lk:
        out, begin, count, needed = lk.path_ids_raw(roots, targets, 0)  # count only
        assert needed == total and [int(c) for c in count] == counts
        assert all((b == lookup.TRUNCATED) == (c > 0) for b, c in zip(begin, counts))
        assert lk.path_stats()["truncated_lists"] == sum(c > 0 for c in counts)
        PC.check_raw(rows, roots, targets, want, lk.path_ids_raw(roots, targets, total), dists)  # capacity = needed
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = lk.path_ids_raw(roots, targets, cap)
            assert needed == total and [int(c) for c in count] == counts
            lost = begin == lookup.TRUNCATED
            assert lost.any() and not (begin == lookup.INVALID).any()
            used = np.zeros(cap + 1, dtype=np.int32)
            for k, p in enumerate(PC.split_paths(out, begin, count)):
                if p is not None and counts[k]:  # a path that was written is complete and in place
                    assert int(begin[k]) + counts[k] <= cap
                    rows.assert_shortest(p, roots[k], targets[k], dists[int(targets[k])])
                    used[int(begin[k]):int(begin[k]) + counts[k]] += 1
            assert used.max() <= 1
        got = lk.path_ids(roots, targets)
        assert [len(p) for p in got] == counts
        for p, r, t in zip(got, roots, targets):
            if len(p):
                rows.assert_shortest(p, r, t, dists[int(t)])


def test_path_ids_asks_for_no_path_more_than_twice(structure, tiers):
    snap, rows = structure
    top = root_of(snap, "top", "view")
    roots = u32(root_of(snap, "c2999", "member"), top, root_of(snap, "e999", "member"), top, top)
    targets = u32(user(snap, "uc"), user(snap, "ux"), user(snap, "ud"), user(snap, "uc"), user(snap, "ux"))
    with lookup.Lookup(snap) as lk:
        calls = []
        raw = lk.path_ids_raw
        lk.path_ids_raw = lambda r, t, cap: (calls.append((len(r), cap)), raw(r, t, cap))[1]
        got = lk.path_ids(roots, targets)  # starts from 8 ids per pair: the chains do not fit
        assert [len(p) for p in got] == [3001, 4, 1001, 0, 4]
        assert len(calls) == 2 and calls[0] == (5, 40)
        # the second call: the two chains and whichever diamond paths reserved after one of them,
        # with exactly the capacity they need
        assert 2 <= calls[1][0] <= 4 and calls[1][1] == 4002 + 4 * (calls[1][0] - 2)
        for p, r, t in zip(got, roots, targets):
            if len(p):
                rows.assert_shortest(p, r, t)


def test_invalid_none_and_duplicated_pairs_in_one_batch(structure, tiers):
    snap, rows = structure
    top, ux, uc = root_of(snap, "top", "view"), user(snap, "ux"), user(snap, "uc")
    c9 = root_of(snap, "c9", "member")
    n = rows.n
    assert ux >= rows.nx
    roots = u32(top, n, top, NONE, top, ux, c9, top, 0xFFFFFFFE, NONE, c9, n + 5)
    targets = u32(ux, ux, n, ux, NONE, ux, uc, ux, NONE, NONE, uc, n + 5)
    counts = [4, 0, 0, 0, 0, 0, 11, 4, 0, 0, 11, 0]
    invalid = [False, True, True, False, False, False, False, False, True, False, False, True]
    with lookup.Lookup(snap) as lk:
        out, begin, count, needed = lk.path_ids_raw(roots, targets, 30)
        assert needed == 30 and [int(c) for c in count] == counts
        assert [b == lookup.INVALID for b in begin] == invalid
        assert not (begin == lookup.TRUNCATED).any()
        used = np.zeros(31, dtype=np.int32)
        for k, p in enumerate(PC.split_paths(out, begin, count)):
            if counts[k]:
                rows.assert_shortest(p, roots[k], targets[k])
                used[int(begin[k]):int(begin[k]) + counts[k]] += 1
        assert (used[:30] == 1).all()  # duplicated pairs have segments of their own
        with pytest.raises(L.KetoError) as e:
            lk.path_ids(roots, targets)
        assert e.value.code == L.EINVAL
        out, begin, count, needed = lk.path_ids_raw(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 8)
        assert needed == 0 and len(begin) == 0
        got = lk.Explain("n", "c9", "member", rt.SubjectID("uc"))
        assert got == lookup.HostLookup(snap).Explain("n", "c9", "member", rt.SubjectID("uc"))  # a chain: one path


def test_slots_stay_clean_between_paths_lists_and_pages(structure, monkeypatch):
    monkeypatch.setenv("KETOGPU_LOOKUP_TIER", "2")
    monkeypatch.setenv("KETOGPU_LOOKUP_SLOTS", "2")
    snap, rows = structure
    names = ("u129", "uc", "ux", "u65", "uy")
    t = u32(*(user(snap, u) for u in names))
    r = u32(*(root_of(snap, o, rel) for o, rel in (("s129_77", "view"), ("c2000", "member"), ("top", "view"),
                                                   ("top", "view"), ("yb", "member"))))
    want_paths = [lookup.host_path(snap, int(a), int(b)) for a, b in zip(r, t)]
    assert [len(w) for w in want_paths] == [2, 2002, 4, 0, 3]
    want_lists = [lookup.host_lookup(snap, int(x), ANY) for x in t]
    host = lookup.HostLookup(snap)
    want_page = host.lookup_page_raw(t, None, ANY, 50)
    with lookup.Lookup(snap) as lk:
        for _ in range(2):
            PC.check_raw(rows, r, t, want_paths, lk.path_ids_raw(r, t, 2011))
            got = lk.lookup_ids(t, ANY)
            assert all(np.array_equal(g, w) for g, w in zip(got, want_lists))
            PC.check_raw(rows, r, t, want_paths, lk.path_ids_raw(r, t, 4000))
            out, returned, count, remaining = lk.lookup_page_raw(t, None, ANY, 50)
            assert np.array_equal(returned, want_page[1]) and np.array_equal(count, want_page[2])
            assert np.array_equal(remaining, want_page[3])
            for k in range(len(t)):
                assert np.array_equal(out[k, :returned[k]], want_page[0][k, :returned[k]])
        assert lk.stats()["slots"] == 2 and lk.path_stats()["tier2_rounds"] == 4 * 3


def test_writes_are_seen_by_the_next_call(tiers):
    table = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
             LC.sset("doc2", "view", "h", "member")]
    snap = Snapshot.from_rows(LC.NS1, table, writable=True)
    alice = rt.SubjectID("alice")
    want = [rt.SubjectSet("n", "doc2", "view"), rt.SubjectSet("n", "h", "member"), alice]
    with lookup.Lookup(snap) as lk:
        assert lk.Explain("n", "doc2", "view", alice) == []
        assert lk.Explain("n", "doc1", "view", alice) == [rt.SubjectSet("n", "doc1", "view"),
                                                          rt.SubjectSet("n", "g", "member"), alice]
        assert lk.stats()["uploads"] == 1
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert lk.Explain("n", "doc2", "view", alice) == want
        assert lk.stats()["uploads"] == 2
        assert lk.Explain("n", "doc2", "view", alice) == lookup.HostLookup(snap).Explain("n", "doc2", "view", alice)
        assert lk.stats()["uploads"] == 2  # no write since: no upload
        assert snap.write((), [LC.sid("h", "member", "alice")])["applied"]
        assert lk.Explain("n", "doc2", "view", alice) == []
        assert lk.stats()["uploads"] == 3
        assert lk.path_stats()["requests"] == 5 and lk.stats()["requests"] == 0


def test_handle_outlives_its_snapshot():
    snap = Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])
    lk = lookup.Lookup(snap)
    r, t = root_of(snap, "d", "view"), user(snap, "u")
    out, begin, count, needed = lk.path_ids_raw(u32(r), u32(t), 4)
    assert needed == 2 and out[:2].tolist() == [r, t]
    lk.snapshot = None
    del snap
    gc.collect()
    with pytest.raises(L.KetoError) as e:  # the rows in HBM are a copy, but the version cannot be read
        lk.path_ids_raw(u32(0), u32(1), 4)
    assert e.value.code == L.EINVAL
    lk.close()
