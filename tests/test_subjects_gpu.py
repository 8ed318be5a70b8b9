"""Subject listing on the device (ketogpu_subjects_*, keto_amd/csrc/subjects.hip) against the
host implementation (ketogpu_snapshot_subjects), which test_subjects_host.py pins against the
oracle.  Lists are compared as sorted arrays: the device writes segments and ids in any order."""
import functools
import gc

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup, synth
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC

pytestmark = pytest.mark.gpu
ANY, IDS = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["default", "tier2", "tier2-scan"])
def tiers(request, monkeypatch):
    """handles created while active: the default tiers, every request through tier 2 with the
    default seen list, or through tier 2 with every finish by scan"""
    if request.param != "default":
        monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    if request.param == "tier2-scan":
        monkeypatch.setenv("KETOGPU_SUBJECTS_LIST_CAP", "0")
    return request.param


def split(out, begin, count):
    """the lists of one raw call, each sorted; a truncated list is None"""
    return [None if b == lookup.TRUNCATED else np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, count)]


def assert_call_matches(sj, snap, roots, cls, want=None):
    """one call with exactly the capacity the host lists need: nothing truncated, every list
    equal to the host's, segments tiling [0, needed)"""
    want = SC.host_lists(snap, roots, cls) if want is None else want
    total = sum(len(w) for w in want)
    out, begin, count, needed = sj.subject_ids_raw(roots, cls, total)
    assert needed == total
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    got = split(out, begin, count)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, int(roots[k]), len(g), len(w))
    used = np.zeros(total + 1, dtype=np.int32)
    for b, c in zip(begin, count):
        used[int(b):int(b) + int(c)] += 1
    assert (used[:total] == 1).all()
    return want


@functools.lru_cache(maxsize=None)
def table_lists(case):
    _, _, snap = LC.table(*case)
    return SC.host_lists(snap, range(snap.stats()["num_expandable"]))


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables_on_the_device(case, tiers):
    _, _, snap = LC.table(*case)
    nx = snap.stats()["num_expandable"]
    with lookup.Subjects(snap) as sj:
        assert_call_matches(sj, snap, np.arange(nx, dtype=np.uint32), ANY, table_lists(case))
        st = sj.stats()
        assert st["requests"] == nx and st["tier1_requests"] + st["tier2_requests"] == nx
        assert (st["tier2_requests"] == nx) == (tiers != "default")
        assert st["list_finishes"] + st["scan_finishes"] == st["tier2_requests"]
        if tiers == "tier2":  # the largest closure of the tables has 246 nodes
            assert st["list_capacity"] == 65536 and st["list_finishes"] == nx
        if tiers == "tier2-scan":
            assert st["list_capacity"] == 0 and st["scan_finishes"] == nx


WORKLOADS = {
    "rbac": (lambda: synth.rbac(users=20000, groups=2000, docs=4000, tuples=150000, checks=6000, seed=41),
             ("groups", "member")),
    "folders": (lambda: synth.folders(users=20000, groups=1000, folders=30000, tuples=150000, seed=42),
                ("groups", "member")),
    "social": (lambda: synth.social(users=30000, groups=6000, tuples=150000, seed=43), ("groups", "member")),
}


@functools.lru_cache(maxsize=None)
def workload(kind):
    w = WORKLOADS[kind][0]()
    return Snapshot.from_columns(w.namespaces, w.columns)


@pytest.mark.parametrize("kind", list(WORKLOADS))
def test_synthetic_workloads_match_the_host(kind):
    snap = workload(kind)
    roots = np.random.default_rng(7).integers(0, snap.stats()["num_expandable"], 2000).astype(np.uint32)
    with lookup.Subjects(snap) as sj:
        every = assert_call_matches(sj, snap, roots, ANY)
        st = sj.stats()
        # a list passes the LDS set exactly when F(r) has more than set_capacity nodes
        over = sum(len(w) > st["set_capacity"] for w in every)
        print(kind, "closures above the set:", over, "largest:", max(len(w) for w in every),
              "ids:", sum(len(w) for w in every))
        assert st["tier2_requests"] == over and st["tier1_requests"] == len(roots) - over
        assert st["list_finishes"] + st["scan_finishes"] == over
        if kind == "folders":
            assert over == 0, "the folders sample stays in tier 1"
        else:
            assert 0 < over < len(roots), "the sample uses both tiers"
        users = assert_call_matches(sj, snap, roots, IDS)
        assert 0 < sum(len(w) for w in users) <= sum(len(w) for w in every)
        ty = snap.type_id(*WORKLOADS[kind][1])
        assert ty not in (lookup.TYPE_NONE, ANY)
        typed = assert_call_matches(sj, snap, roots, ty)
        assert 0 < sum(len(w) for w in typed) <= sum(len(w) for w in every)
        for nothing in (lookup.TYPE_NONE, lookup.CLASS_UNTYPED_SET):
            out, begin, count, needed = sj.subject_ids_raw(roots, nothing, 16)
            assert needed == 0 and not count.any()


def test_set_boundary():
    with lookup.Subjects(Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])) as sj0:
        cap = sj0.stats()["set_capacity"]
    assert cap >= 64
    sizes = (cap - 1, cap, cap + 1)
    rows = []
    for k in sizes:
        rows += SC.fwd_star_rows(f"star{k}", k, f"a{k}_") + SC.fwd_split_rows(f"split{k}", k, f"b{k}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with lookup.Subjects(snap) as sj:
        for shape in ("star", "split"):
            for k in sizes:
                r = lookup.resolve_roots(snap, [("n", f"{shape}{k}", "view")])
                before = sj.stats()
                want = assert_call_matches(sj, snap, r, ANY)
                assert len(want[0]) == k  # F(r) has exactly k nodes
                after = sj.stats()
                assert after["tier2_requests"] - before["tier2_requests"] == (1 if k > cap else 0), (shape, k)
                assert after["tier1_requests"] - before["tier1_requests"] == (0 if k > cap else 1), (shape, k)
                assert len(assert_call_matches(sj, snap, r, IDS)[0]) == (k if shape == "star" else k - 2)


def test_list_finish_boundary(monkeypatch):
    k = 130
    monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    monkeypatch.setenv("KETOGPU_SUBJECTS_LIST_CAP", str(k))
    sizes = (k - 1, k, k + 1)
    rows = []
    for m in sizes:
        rows += SC.fwd_star_rows(f"star{m}", m, f"a{m}_") + SC.fwd_split_rows(f"split{m}", m, f"b{m}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with lookup.Subjects(snap) as sj:
        assert sj.stats()["list_capacity"] == k
        for rep in range(2):  # the second round finds the bitmaps clean after both finishes
            for shape in ("star", "split"):
                for m in sizes:
                    r = lookup.resolve_roots(snap, [("n", f"{shape}{m}", "view")])
                    before = sj.stats()
                    assert len(assert_call_matches(sj, snap, r, ANY)[0]) == m
                    after = sj.stats()
                    assert after["list_finishes"] - before["list_finishes"] == (1 if m <= k else 0), (shape, m)
                    assert after["scan_finishes"] - before["scan_finishes"] == (0 if m <= k else 1), (shape, m)
        # all six in one call, then the same call again: the same lists from reused slots
        r = lookup.resolve_roots(snap, [("n", f"{shape}{m}", "view") for shape in ("star", "split") for m in sizes])
        before = sj.stats()
        want = assert_call_matches(sj, snap, r, ANY)
        assert_call_matches(sj, snap, r, IDS)
        assert_call_matches(sj, snap, r, ANY, want)
        after = sj.stats()
        assert after["list_finishes"] - before["list_finishes"] == 12
        assert after["scan_finishes"] - before["scan_finishes"] == 6


@functools.lru_cache(maxsize=None)
def structure():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    return snap, SC.host_lists(snap, range(snap.stats()["num_nodes"]))


def test_structure_cases(tiers):
    snap, want = structure()
    n = snap.stats()["num_nodes"]
    root = lambda obj, rel: int(lookup.resolve_roots(snap, [("n", obj, rel)])[0])
    with lookup.Subjects(snap) as sj:
        assert_call_matches(sj, snap, np.arange(n, dtype=np.uint32), ANY, want)  # every node, one call
        one = lambda r, cls=ANY: sj.subject_ids([r], cls)[0]
        assert len(one(root("c2999", "member"))) == 3000 and len(one(root("e999", "member"))) == 1000
        for name in ("ya", "yb", "self"):
            r = root(name, "member")
            assert r in one(r)
        assert len(one(root("top", "view"))) == 4  # the diamond
        assert len(one(root("f65", "view"), IDS)) == 65 and len(one(root("f129", "view"), IDS)) == 129
        assert len(one(root("two", "view"))) == 42 and len(one(root("two", "view"), IDS)) == 40


def test_batch_sizes_none_leaf_and_invalid_roots(tiers):
    snap, want = structure()
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    with lookup.Subjects(snap) as sj:
        out, begin, count, needed = sj.subject_ids_raw(np.zeros(0, dtype=np.uint32), ANY, 8)
        assert needed == 0 and len(begin) == 0
        for m in (1, 63, 64, 65):
            r = np.arange(5, 5 + m, dtype=np.uint32)
            assert_call_matches(sj, snap, r, ANY, [want[int(x)] for x in r])
        r = np.array([7, L.NODE_NONE, n, 9, 0xFFFFFFFE, n - 1, nx, nx - 1], dtype=np.uint32)
        total = sum(len(want[int(x)]) for x in (7, 9, nx - 1))
        assert total > 0
        out, begin, count, needed = sj.subject_ids_raw(r, ANY, total)
        assert needed == total
        assert begin[2] == lookup.INVALID and begin[4] == lookup.INVALID and count[2] == 0 and count[4] == 0
        for k in (1, 5, 6):  # no root and roots without rows: the empty list, not an error
            assert begin[k] not in (lookup.INVALID, lookup.TRUNCATED) and count[k] == 0
        got = split(out, begin, count)
        for k in (0, 3, 7):
            assert np.array_equal(got[k], want[int(r[k])])
        with pytest.raises(L.KetoError) as e:
            sj.subject_ids(r)
        assert e.value.code == L.EINVAL


def test_truncation_protocol(tiers):
    snap = workload("rbac")
    roots = np.random.default_rng(11).integers(0, snap.stats()["num_expandable"], 300).astype(np.uint32)
    want = SC.host_lists(snap, roots)
    total = sum(len(w) for w in want)
    with lookup.Subjects(snap) as sj:
        out, begin, count, needed = sj.subject_ids_raw(roots, ANY, 0)  # count only
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert all(b == lookup.TRUNCATED for b, w in zip(begin, want) if len(w))
        assert_call_matches(sj, snap, roots, ANY, want)  # capacity = needed: nothing truncated
        trunc_before = sj.stats()["truncated_lists"]
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = sj.subject_ids_raw(roots, ANY, cap)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
            lost = begin == lookup.TRUNCATED
            assert lost.any()
            written = 0
            for g, w, b in zip(split(out, begin, count), want, begin):
                if g is not None:  # a list that was written is complete
                    assert np.array_equal(g, w) and int(b) + len(w) <= cap
                    written += len(w)
            assert written <= cap
        assert sj.stats()["truncated_lists"] > trunc_before
        for start in (1, 1000):  # the re-issue loop, from a tiny capacity
            got = sj.subject_ids(roots, ANY, capacity=start)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_slot_reuse_and_repeated_calls(monkeypatch):
    monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    monkeypatch.setenv("KETOGPU_SUBJECTS_SLOTS", "1")
    monkeypatch.setenv("KETOGPU_SUBJECTS_LIST_CAP", "200")
    snap, want = structure()
    r = lookup.resolve_roots(snap, [("n", "f129", "view"), ("n", "c2999", "member"), ("n", "f65", "view")])
    w = [want[int(x)] for x in r]
    assert [len(x) for x in w] == [129, 3000, 65]
    with lookup.Subjects(snap) as sj:
        assert_call_matches(sj, snap, r, ANY, w)
        st = sj.stats()
        assert st["tier2_rounds"] == 3 and st["tier2_requests"] == 3 and st["slots"] == 1
        assert st["list_finishes"] == 2 and st["scan_finishes"] == 1
        assert_call_matches(sj, snap, r, ANY, w)  # the slot's bitmap was left clean by both finishes
        total = sum(len(x) for x in w)
        out, begin, count, needed = sj.subject_ids_raw(r, ANY, 50 * total)  # the output buffer grows
        assert needed == total and all(np.array_equal(g, x) for g, x in zip(split(out, begin, count), w))
        assert sj.stats()["tier2_rounds"] == 9 and sj.stats()["uploads"] == 1


def test_writes_are_seen_by_the_next_call(tiers):
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
            LC.sset("doc2", "view", "h", "member"), LC.sid("doc3", "view", "bob")]
    rows += [LC.sid("h", "member", f"m{i}") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    members = sorted(["bob"] + [f"m{i}" for i in range(40)])
    users = lambda sj, d: [s.id for s in sj.ListSubjects("n", d, "view")]
    with lookup.Subjects(snap) as sj:
        assert users(sj, "doc1") == ["alice"] and users(sj, "doc2") == members
        assert sj.stats()["uploads"] == 1
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert users(sj, "doc2") == sorted(members + ["alice"])
        assert sj.stats()["uploads"] == 2
        assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (reserved id)
        assert users(sj, "doc2") == sorted(members + ["alice", "carol"])
        assert sj.stats()["uploads"] == 3
        assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]  # a deleted row disappears
        assert users(sj, "doc1") == [] and users(sj, "doc2") == sorted(members + ["alice", "carol"])
        assert sj.stats()["uploads"] == 4
        ids = list(range(snap.stats()["num_nodes"]))
        real = []
        for v in ids:  # every node but the placeholders, as the host lists them
            try:
                snap.describe(v)
                real.append(v)
            except L.KetoError:
                pass
        assert len(real) == len(ids) - 3
        want = assert_call_matches(sj, snap, np.array(real, dtype=np.uint32), ANY)
        listed = set(int(t) for w in want for t in w)
        assert listed and not (set(ids) - set(real)) & listed  # placeholders are never listed
        assert sj.stats()["uploads"] == 4  # no write since: no upload


def test_handle_outlives_its_snapshot():
    snap = Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])
    sj = lookup.Subjects(snap)
    assert len(sj.subject_ids([0])) == 1
    sj.snapshot = None
    del snap
    gc.collect()
    with pytest.raises(L.KetoError) as e:  # the rows in HBM are a copy, but the version cannot be read
        sj.subject_ids_raw(np.zeros(1, dtype=np.uint32), ANY, 4)
    assert e.value.code == L.EINVAL
    sj.close()


def test_list_subjects_by_name():
    snap = workload("rbac")
    docs = [("docs", f"d{i}", "viewer") for i in (0, 3, 17, 3999)] + [("docs", "no such doc", "viewer"),
                                                                       ("nowhere", "d0", "viewer")]
    with lookup.Subjects(snap) as sj:
        for kind in ("ids", "any", ("groups", "member"), ("groups", "no such relation")):
            got = sj.list_subjects_batch(docs, kind)
            for d, g in zip(docs, got):
                assert g == lookup.host_list_subjects(snap, *d, kind=kind), (d, kind)
            assert got[-1] == [] and got[-2] == []
            assert any(got[:4]) == (kind != ("groups", "no such relation"))
        ids = sj.ListSubjects("docs", "d3", "viewer")
        assert ids == sj.list_subjects_batch(docs, "ids")[1] and all(isinstance(s, rt.SubjectID) for s in ids)
        every = sj.ListSubjects("docs", "d3", "viewer", kind="any")
        k = len(ids)
        assert every[:k] == ids and all(isinstance(s, rt.SubjectSet) for s in every[k:]) and len(every) > k
