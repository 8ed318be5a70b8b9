"""The checks of the wide calls (ketogpu_subjects_ids_wide / ketogpu_lookup_ids_wide,
keto_amd/csrc/wide.hpp), shared by test_wide_subjects_gpu.py and test_wide_lookup_gpu.py.  A `Side`
is one listing handle as the checks see it; every list is compared with the host's, which
test_subjects_host.py and test_lookup_host.py pin against the oracle.  Lists are compared as sorted
arrays: the device writes segments and ids in any order.

Routing: by default tier 1 answers what fits its LDS set and the wide tier the rest;
KETOGPU_<SIDE>_TIER=2 ("forced") sends every request that has a row to the wide tier."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup, synth
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC

ANY = lookup.TYPE_ANY


class Side:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def force(self, monkeypatch, slots=None):
        monkeypatch.setenv(self.env + "_TIER", "2")
        if slots is not None:
            monkeypatch.setenv(self.env + "_SLOTS", str(slots))


SUBJECTS = Side(
    name="subjects", env="KETOGPU_SUBJECTS", handle=lookup.Subjects,
    raw=lambda h, ids, f=ANY, cap=0, wide=True: h.subject_ids_raw(ids, f, cap, wide=wide),
    lists=lambda h, ids, f=ANY, **kw: h.subject_ids(ids, f, wide=True, **kw),
    host=lambda snap, ids, f=ANY: SC.host_lists(snap, ids, f),
    starts=lambda st: st["num_expandable"],  # the ids that can have a row
    second_filter=lambda snap: lookup.CLASS_SUBJECT_ID,
    view_filter=lambda snap: lookup.CLASS_SUBJECT_ID,  # the users of a star or split document
    structure_rows=SC.structure_rows, star=SC.fwd_star_rows, split=SC.fwd_split_rows,
    start=lambda snap, name: int(lookup.resolve_roots(snap, [("n", name, "view")])[0]),
    # starts of the structure graph: the 3000-chain, a star of 129, a star of 65
    structure_starts=lambda snap: lookup.resolve_roots(
        snap, [("n", "f129", "view"), ("n", "c2999", "member"), ("n", "f65", "view"), ("n", "f129", "view")]),
    cycle_starts=lambda snap: lookup.resolve_roots(snap, [("n", x, "member") for x in ("ya", "yb", "self")]),
    workload_starts=lambda st: st["num_expandable"],
)

LOOKUP = Side(
    name="lookup", env="KETOGPU_LOOKUP", handle=lookup.Lookup,
    raw=lambda h, ids, f=ANY, cap=0, wide=True: h.lookup_ids_raw(ids, f, cap, wide=wide),
    lists=lambda h, ids, f=ANY, **kw: h.lookup_ids(ids, f, wide=True, **kw),
    host=lambda snap, ids, f=ANY: [lookup.host_lookup(snap, int(t), f) for t in ids],
    starts=lambda st: st["num_nodes"],
    second_filter=lambda snap: snap.node_info(0)["type"],  # an object type that occurs
    view_filter=lambda snap: snap.type_id("n", "view"),  # the documents of a star or split user
    structure_rows=LC.structure_rows, star=LC.star_rows, split=LC.split_star_rows,
    start=lambda snap, name: int(lookup.resolve_subjects(snap, [rt.SubjectID(name)])[0]),
    structure_starts=lambda snap: lookup.resolve_subjects(
        snap, [rt.SubjectID(u) for u in ("u129", "uc", "u65", "u129")]),
    cycle_starts=lambda snap: lookup.resolve_subjects(
        snap, [rt.SubjectSet("n", x, "member") for x in ("ya", "yb", "self")]),
    workload_starts=lambda st: st["num_nodes"],
)


def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def split(out, begin, count):
    """the lists of one raw call, each sorted; a truncated list is None"""
    return [None if b == lookup.TRUNCATED else np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, count)]


def assert_call_matches(S, h, ids, f, want, wide=True):
    """one call with exactly the capacity the host lists need: nothing truncated, every list
    equal to the host's, segments tiling [0, needed)"""
    total = sum(len(w) for w in want)
    out, begin, count, needed = S.raw(h, ids, f, total, wide=wide)
    assert needed == total
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    for k, (g, w) in enumerate(zip(split(out, begin, count), want)):
        assert np.array_equal(g, w), (k, int(ids[k]), len(g), len(w))
    used = np.zeros(total + 1, dtype=np.int32)
    for b, c in zip(begin, count):
        used[int(b):int(b) + int(c)] += 1
    assert (used[:total] == 1).all()
    return want


def plain_stats_do_not_move(h, before):
    """a wide call counts in wide_stats() only (uploads and the wall time aside)"""
    after = h.stats()
    for k in after:
        if k not in ("uploads", "last_call_ms"):
            assert after[k] == before[k], k


# ---------------------------------------------------------------------- truth tables
@functools.lru_cache(maxsize=None)
def _table_lists(side, case, f):
    S = SIDES[side]
    _, _, snap = LC.table(*case)
    return S.host(snap, range(S.starts(snap.stats())), f)


def check_truth_table(S, case, forced, monkeypatch):
    if forced:
        S.force(monkeypatch)
    _, _, snap = LC.table(*case)
    n = S.starts(snap.stats())
    ids = np.arange(n, dtype=np.uint32)
    with S.handle(snap) as h:
        plain = h.stats()
        calls = 0
        for f in (ANY, S.second_filter(snap), lookup.TYPE_NONE):
            want = _table_lists(S.name, case, f)
            assert_call_matches(S, h, ids, f, want)
            calls += 1
            if f == lookup.TYPE_NONE:
                assert not any(len(w) for w in want)
        assert any(len(w) for w in _table_lists(S.name, case, ANY))
        st = h.wide_stats()
        assert st["requests"] == calls * n and st["tier1_requests"] + st["wide_requests"] == calls * n
        if forced:  # (every one of these ids can have a row)
            assert st["wide_requests"] == calls * n
            assert st["wide_rounds"] >= calls and st["levels"] >= calls and st["items"] >= st["levels"]
        else:  # the largest closure of the tables has 246 nodes
            assert st["wide_requests"] == 0 and st["wide_rounds"] == 0 and st["levels"] == 0
        plain_stats_do_not_move(h, plain)


# ---------------------------------------------------------------------- structure
@functools.lru_cache(maxsize=None)
def structure(side):
    S = SIDES[side]
    snap = Snapshot.from_rows(LC.NS1, S.structure_rows())
    return snap, S.host(snap, range(snap.stats()["num_nodes"]))


def check_structure(S, monkeypatch):
    """every node as a start in one call under forced routing: the 3000-chain (3000 levels, one
    item each), the 1000-chain, the cycles back to the start, the diamond, the rows of 65 and 129"""
    S.force(monkeypatch)
    snap, want = structure(S.name)
    n = snap.stats()["num_nodes"]
    with S.handle(snap) as h:
        assert_call_matches(S, h, np.arange(n, dtype=np.uint32), ANY, want)
        st = h.wide_stats()
        assert st["wide_requests"] == S.starts(snap.stats()) and st["levels"] >= 3000
        assert sorted(len(w) for w in want)[-1] == 3000
        cyc = S.cycle_starts(snap)
        got = S.lists(h, cyc)
        for r, g in zip(cyc, got):  # the start is listed only where a cycle leads back to it
            assert int(r) in g
        listed_self = [v for v in range(n) if v in want[v]]
        assert sorted(listed_self) == sorted(int(r) for r in cyc)


# ---------------------------------------------------------------------- chunk boundaries
def check_chunk_boundaries(S, monkeypatch):
    S.force(monkeypatch)
    with S.handle(Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])) as h0:
        C = h0.wide_stats()["chunk"]
    assert C >= 64
    sizes = (C - 1, C, C + 1, 2 * C + 1)
    rows = []
    for k in sizes:
        rows += S.star(f"star{k}", k, f"a{k}_") + S.split(f"split{k}", k, f"b{k}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    f2 = S.view_filter(snap)
    with S.handle(snap) as h:
        for shape in ("star", "split"):
            for k in sizes:
                r = np.array([S.start(snap, f"{shape}{k}")], dtype=np.uint32)
                before = h.wide_stats()
                want = assert_call_matches(S, h, r, ANY, S.host(snap, r))
                assert len(want[0]) == k
                after = h.wide_stats()
                assert after["wide_requests"] - before["wide_requests"] == 1
                if shape == "star":  # one row of k entries, none of which has a row to read
                    assert after["items"] - before["items"] == -(-k // C), (k, C)
                    assert after["levels"] - before["levels"] == 1
                typed = assert_call_matches(S, h, r, f2, S.host(snap, r, f2))
                assert len(typed[0]) == (k if shape == "star" else k - 2)
        every = np.array([S.start(snap, f"{shape}{k}") for shape in ("star", "split") for k in sizes], dtype=np.uint32)
        assert_call_matches(S, h, every, ANY, S.host(snap, every))  # all of them, one round


# ---------------------------------------------------------------------- default routing
def check_set_boundary(S):
    with S.handle(Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])) as h0:
        cap = h0.stats()["set_capacity"]
    sizes = (cap - 1, cap, cap + 1)
    rows = []
    for k in sizes:
        rows += S.star(f"star{k}", k, f"a{k}_") + S.split(f"split{k}", k, f"b{k}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with S.handle(snap) as h:
        for shape in ("star", "split"):
            for k in sizes:
                r = np.array([S.start(snap, f"{shape}{k}")], dtype=np.uint32)
                before = h.wide_stats()
                want = assert_call_matches(S, h, r, ANY, S.host(snap, r))
                assert len(want[0]) == k
                after = h.wide_stats()
                assert after["wide_requests"] - before["wide_requests"] == (1 if k > cap else 0), (shape, k)
                assert after["tier1_requests"] - before["tier1_requests"] == (0 if k > cap else 1), (shape, k)


WORKLOADS = {  # test_subjects_gpu.py's sizes
    "rbac": lambda: synth.rbac(users=20000, groups=2000, docs=4000, tuples=150000, checks=6000, seed=41),
    "social": lambda: synth.social(users=30000, groups=6000, tuples=150000, seed=43),
}


@functools.lru_cache(maxsize=None)
def workload(kind):
    w = WORKLOADS[kind]()
    return Snapshot.from_columns(w.namespaces, w.columns)


@functools.lru_cache(maxsize=None)
def workload_lists(side, kind, seed, n):
    S = SIDES[side]
    snap = workload(kind)
    ids = np.random.default_rng(seed).integers(0, S.workload_starts(snap.stats()), n).astype(np.uint32)
    return ids, S.host(snap, ids)


def check_workload(S, kind):
    snap = workload(kind)
    ids, want = workload_lists(S.name, kind, 7, 2000)
    with S.handle(snap) as h:
        plain = h.stats()
        assert_call_matches(S, h, ids, ANY, want)
        st = h.wide_stats()
        over = sum(len(w) > h.stats()["set_capacity"] for w in want)
        print(S.name, kind, "closures above the set:", over, "largest:", max(len(w) for w in want), "wide:", st)
        assert 0 < over < len(ids), "the sample uses both tiers"
        assert st["wide_requests"] == over and st["tier1_requests"] == len(ids) - over
        assert st["wide_rounds"] >= 1 and st["slots"] >= 1 and st["ids_produced"] == sum(len(w) for w in want)
        plain_stats_do_not_move(h, plain)
        assert_call_matches(S, h, ids, ANY, want, wide=False)  # ... and the plain call finds its bitmaps clean


# ---------------------------------------------------------------------- rounds and clean state
def check_rounds(S, slots, monkeypatch):
    """more wide requests than slots, the same start twice in one call, and the same call again"""
    S.force(monkeypatch, slots)
    snap, want = structure(S.name)
    r = S.structure_starts(snap)
    w = [want[int(x)] for x in r]
    assert [len(x) for x in w] == [129, 3000, 65, 129]
    with S.handle(snap) as h:
        assert_call_matches(S, h, r, ANY, w)
        st = h.wide_stats()
        assert st["slots"] == slots and st["wide_requests"] == 4 and st["wide_rounds"] == 4 // slots
        assert_call_matches(S, h, r, ANY, w)  # every bitmap was left clean
        total = sum(len(x) for x in w)
        out, begin, count, needed = S.raw(h, r, ANY, 50 * total)  # the output buffer grows
        assert needed == total and all(np.array_equal(g, x) for g, x in zip(split(out, begin, count), w))
        assert h.wide_stats()["wide_rounds"] == 3 * (4 // slots)


def check_plain_wide_plain(S, monkeypatch):
    """the two tiers share their bitmaps: each finds them all zero behind the other"""
    S.force(monkeypatch)
    snap, want = structure(S.name)
    r = S.structure_starts(snap)
    w = [want[int(x)] for x in r]
    with S.handle(snap) as h:
        assert_call_matches(S, h, r, ANY, w, wide=False)
        assert_call_matches(S, h, r, ANY, w, wide=True)
        assert_call_matches(S, h, r, ANY, w, wide=False)
        assert_call_matches(S, h, r, ANY, w, wide=True)
        assert h.stats()["tier2_requests"] == 8 and h.wide_stats()["wide_requests"] == 8


# ---------------------------------------------------------------------- truncation
def check_truncation(S, forced, monkeypatch):
    if forced:
        S.force(monkeypatch)
    snap = workload("rbac")
    ids, want = workload_lists(S.name, "rbac", 11, 300)
    total = sum(len(w) for w in want)
    with S.handle(snap) as h:
        out, begin, count, needed = S.raw(h, ids, ANY, 0)  # count only
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert all(b == lookup.TRUNCATED for b, w in zip(begin, want) if len(w))
        assert_call_matches(S, h, ids, ANY, want)  # capacity = needed: nothing truncated
        trunc_before = h.wide_stats()["truncated_lists"]
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = S.raw(h, ids, ANY, cap)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
            assert (begin == lookup.TRUNCATED).any()
            written = 0
            for g, w, b in zip(split(out, begin, count), want, begin):
                if g is not None:  # a list that was written is complete
                    assert np.array_equal(g, w) and int(b) + len(w) <= cap
                    written += len(w)
            assert written <= cap
        assert h.wide_stats()["truncated_lists"] > trunc_before
        got = S.lists(h, ids, capacity=1)  # the re-issue loop, from a tiny capacity
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert_call_matches(S, h, ids, ANY, want)  # truncated lists left their bitmaps clean too
        if forced:
            assert h.wide_stats()["tier1_requests"] == 0


# ---------------------------------------------------------------------- starts
def check_starts(S, forced, monkeypatch):
    """NODE_NONE, ids without rows, ids outside the snapshot, n = 0 and n = 1, 63, 64, 65"""
    if forced:
        S.force(monkeypatch)
    snap, want = structure(S.name)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    with S.handle(snap) as h:
        out, begin, count, needed = S.raw(h, np.zeros(0, dtype=np.uint32), ANY, 8)
        assert needed == 0 and len(begin) == 0
        for m in (1, 63, 64, 65):
            r = np.arange(5, 5 + m, dtype=np.uint32)
            assert_call_matches(S, h, r, ANY, [want[int(x)] for x in r])
        r = np.array([7, L.NODE_NONE, n, 9, 0xFFFFFFFE, n - 1, nx, nx - 1], dtype=np.uint32)
        valid = (0, 3, 5, 6, 7)
        total = sum(len(want[int(r[k])]) for k in valid)
        assert total > 0
        before = h.wide_stats()
        out, begin, count, needed = S.raw(h, r, ANY, total)
        assert needed == total
        assert begin[2] == lookup.INVALID and begin[4] == lookup.INVALID and count[2] == 0 and count[4] == 0
        assert begin[1] not in (lookup.INVALID, lookup.TRUNCATED) and count[1] == 0
        got = split(out, begin, count)
        for k in valid:  # (ids without rows among them: the empty list, not an error)
            assert begin[k] not in (lookup.INVALID, lookup.TRUNCATED)
            assert np.array_equal(got[k], want[int(r[k])])
        after = h.wide_stats()
        rowed = sum(1 for k in valid if int(r[k]) < S.starts(st))
        assert after["requests"] - before["requests"] == len(r)
        assert (after["tier1_requests"] - before["tier1_requests"]) + (after["wide_requests"]
                                                                       - before["wide_requests"]) == len(valid)
        if forced:
            assert after["wide_requests"] - before["wide_requests"] == rowed
        with pytest.raises(L.KetoError) as e:
            S.lists(h, r)
        assert e.value.code == L.EINVAL


SIDES = {"subjects": SUBJECTS, "lookup": LOOKUP}
