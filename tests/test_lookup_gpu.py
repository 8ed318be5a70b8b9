"""Reverse lookup on the device (ketogpu_lookup_*, keto_amd/csrc/lookup.hip) against the host
implementation (ketogpu_snapshot_lookup), which test_lookup_host.py pins against the oracle.
Lists are compared as sorted arrays: the device writes segments and ids in any order."""
import functools
import gc

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup, synth
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC

pytestmark = pytest.mark.gpu
ANY = lookup.TYPE_ANY


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["default", "tier2"])
def tiers(request, monkeypatch):
    """handles created while active: the default tiers, or every request through tier 2"""
    if request.param == "tier2":
        monkeypatch.setenv("KETOGPU_LOOKUP_TIER", "2")
    return request.param


def host_lists(snap, targets, ty=ANY):
    return [lookup.host_lookup(snap, int(t), ty) for t in targets]


def split(out, begin, count):
    """the lists of one raw call, each sorted; a truncated list is None"""
    return [None if b == lookup.TRUNCATED else np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, count)]


def assert_call_matches(lk, snap, targets, ty, want=None):
    """one call with exactly the capacity the host lists need: nothing truncated, every list
    equal to the host's, segments disjoint"""
    want = host_lists(snap, targets, ty) if want is None else want
    total = sum(len(w) for w in want)
    out, begin, count, needed = lk.lookup_ids_raw(targets, ty, total)
    assert needed == total
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    got = split(out, begin, count)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, int(targets[k]), len(g), len(w))
    used = np.zeros(total + 1, dtype=np.int32)  # the segments tile [0, needed)
    for b, c in zip(begin, count):
        used[int(b):int(b) + int(c)] += 1
    assert (used[:total] == 1).all()
    return want


@functools.lru_cache(maxsize=None)
def table_lists(case):
    _, _, snap = LC.table(*case)
    return host_lists(snap, range(snap.stats()["num_nodes"]))


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables_on_the_device(case, tiers):
    _, _, snap = LC.table(*case)
    n = snap.stats()["num_nodes"]
    with lookup.Lookup(snap) as lk:
        assert_call_matches(lk, snap, np.arange(n, dtype=np.uint32), ANY, table_lists(case))
        st = lk.stats()
        assert st["requests"] == n and st["tier1_requests"] + st["tier2_requests"] == n
        assert (st["tier2_requests"] == n) == (tiers == "tier2")


WORKLOADS = {
    "rbac": (lambda: synth.rbac(users=20000, groups=2000, docs=4000, tuples=150000, checks=6000, seed=41),
             [("docs", "viewer"), ("groups", "member")]),
    "folders": (lambda: synth.folders(users=20000, groups=1000, folders=30000, tuples=150000, seed=42),
                [("folders", "viewer"), ("groups", "member")]),
    "social": (lambda: synth.social(users=30000, groups=6000, tuples=150000, seed=43), [("groups", "member")]),
}


@functools.lru_cache(maxsize=None)
def workload(kind):
    w = WORKLOADS[kind][0]()
    return Snapshot.from_columns(w.namespaces, w.columns)


@pytest.mark.parametrize("kind", list(WORKLOADS))
def test_synthetic_workloads_match_the_host(kind):
    snap = workload(kind)
    targets = np.random.default_rng(7).integers(0, snap.stats()["num_nodes"], 2000).astype(np.uint32)
    with lookup.Lookup(snap) as lk:
        every = assert_call_matches(lk, snap, targets, ANY)
        st = lk.stats()
        # a list passes the LDS set exactly when B(t) has more than set_capacity nodes
        over = sum(len(w) > st["set_capacity"] for w in every)
        assert st["tier2_requests"] == over and st["tier1_requests"] == len(targets) - over
        assert over > 0 and over < len(targets), "the sample uses both tiers"
        for ns, rel in WORKLOADS[kind][1]:
            ty = snap.type_id(ns, rel)
            assert ty not in (lookup.TYPE_NONE, ANY)
            typed = assert_call_matches(lk, snap, targets, ty)
            assert 0 < sum(len(w) for w in typed) <= sum(len(w) for w in every)
        out, begin, count, needed = lk.lookup_ids_raw(targets, lookup.TYPE_NONE, 16)
        assert needed == 0 and not count.any()


def test_rbac_list_objects_by_name():
    snap = workload("rbac")
    users = [rt.SubjectID(f"u{u}") for u in (3, 17, 4242, 19999)] + [rt.SubjectID("nobody")]
    with lookup.Lookup(snap) as lk:
        got = lk.list_objects_batch("docs", "viewer", users)
        for u, g in zip(users, got):
            assert g == lookup.host_list_objects(snap, "docs", "viewer", u)
        assert got[-1] == [] and any(got[:-1])
        assert lk.ListObjects("docs", "viewer", users[0]) == got[0]
        assert lk.ListObjects("nowhere", "viewer", users[0]) == []


def test_set_boundary():
    with lookup.Lookup(Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])) as lk0:
        cap = lk0.stats()["set_capacity"]
    assert cap >= 64
    sizes = (cap - 1, cap, cap + 1)
    rows = []
    for k in sizes:
        rows += LC.star_rows(f"star{k}", k, f"a{k}_") + LC.split_star_rows(f"split{k}", k, f"b{k}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with lookup.Lookup(snap) as lk:
        for shape in ("star", "split"):
            for k in sizes:
                t = lookup.resolve_subjects(snap, [rt.SubjectID(f"{shape}{k}")])
                before = lk.stats()
                want = assert_call_matches(lk, snap, t, ANY)
                assert len(want[0]) == k  # B(t) has exactly k nodes
                after = lk.stats()
                assert after["tier2_requests"] - before["tier2_requests"] == (1 if k > cap else 0), (shape, k)
                assert after["tier1_requests"] - before["tier1_requests"] == (0 if k > cap else 1), (shape, k)
                ty = snap.type_id("n", "view")
                assert len(assert_call_matches(lk, snap, t, ty)[0]) == (k if shape == "star" else k - 2)


@functools.lru_cache(maxsize=None)
def structure():
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows())
    return snap, host_lists(snap, range(snap.stats()["num_nodes"]))


def test_structure_cases(tiers):
    snap, want = structure()
    n = snap.stats()["num_nodes"]
    tgt = lambda s: int(lookup.resolve_subjects(snap, [s])[0])
    with lookup.Lookup(snap) as lk:
        assert_call_matches(lk, snap, np.arange(n, dtype=np.uint32), ANY, want)  # every node, one call
        one = lambda t: lk.lookup_ids([t])[0]
        assert len(one(tgt(rt.SubjectID("uc")))) == 3000 and len(one(tgt(rt.SubjectID("ud")))) == 1000
        for name in ("ya", "yb", "self"):
            t = tgt(rt.SubjectSet("n", name, "member"))
            assert t in one(t)
        assert len(one(tgt(rt.SubjectID("ux")))) == 4  # the diamond
        assert len(one(tgt(rt.SubjectID("u65")))) == 65 and len(one(tgt(rt.SubjectID("u129")))) == 129
        assert len(one(tgt(rt.SubjectSet("n", "lonely", "view")))) == 0  # an empty reverse row


def test_batch_sizes_none_and_invalid_targets(tiers):
    snap, want = structure()
    n = snap.stats()["num_nodes"]
    with lookup.Lookup(snap) as lk:
        out, begin, count, needed = lk.lookup_ids_raw(np.zeros(0, dtype=np.uint32), ANY, 8)
        assert needed == 0 and len(begin) == 0
        for m in (1, 63, 64, 65):
            t = np.arange(5, 5 + m, dtype=np.uint32)
            assert_call_matches(lk, snap, t, ANY, [want[int(x)] for x in t])
        t = np.array([7, L.NODE_NONE, n, 9, 0xFFFFFFFE, n - 1], dtype=np.uint32)
        total = sum(len(want[int(x)]) for x in (7, 9, n - 1))
        out, begin, count, needed = lk.lookup_ids_raw(t, ANY, total)
        assert needed == total
        assert begin[2] == lookup.INVALID and begin[4] == lookup.INVALID and count[2] == 0 and count[4] == 0
        assert begin[1] not in (lookup.INVALID, lookup.TRUNCATED) and count[1] == 0
        got = split(out, begin, count)
        for k in (0, 3, 5):
            assert np.array_equal(got[k], want[int(t[k])])
        with pytest.raises(L.KetoError) as e:
            lk.lookup_ids(t)
        assert e.value.code == L.EINVAL


def test_truncation_protocol(tiers):
    snap = workload("rbac")
    targets = np.random.default_rng(11).integers(0, snap.stats()["num_nodes"], 300).astype(np.uint32)
    want = host_lists(snap, targets)
    total = sum(len(w) for w in want)
    with lookup.Lookup(snap) as lk:
        out, begin, count, needed = lk.lookup_ids_raw(targets, ANY, 0)  # count only
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert all(b == lookup.TRUNCATED for b, w in zip(begin, want) if len(w))
        assert_call_matches(lk, snap, targets, ANY, want)  # capacity = needed: nothing truncated
        trunc_before = lk.stats()["truncated_lists"]
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = lk.lookup_ids_raw(targets, ANY, cap)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
            lost = begin == lookup.TRUNCATED
            assert lost.any()
            written = 0
            for g, w, b in zip(split(out, begin, count), want, begin):
                if g is not None:  # a list that was written is complete
                    assert np.array_equal(g, w) and int(b) + len(w) <= cap
                    written += len(w)
            assert written <= cap
        assert lk.stats()["truncated_lists"] > trunc_before
        for start in (1, 1000):  # the re-issue loop, from a tiny capacity
            got = lk.lookup_ids(targets, ANY, capacity=start)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_slot_reuse_and_repeated_calls(monkeypatch):
    monkeypatch.setenv("KETOGPU_LOOKUP_TIER", "2")
    monkeypatch.setenv("KETOGPU_LOOKUP_SLOTS", "1")
    snap, want = structure()
    t = lookup.resolve_subjects(snap, [rt.SubjectID(u) for u in ("u129", "uc", "u65")])
    w = [want[int(x)] for x in t]
    with lookup.Lookup(snap) as lk:
        assert_call_matches(lk, snap, t, ANY, w)
        st = lk.stats()
        assert st["tier2_rounds"] == 3 and st["tier2_requests"] == 3 and st["slots"] == 1
        assert_call_matches(lk, snap, t, ANY, w)  # the slot's bitmap was left clean
        total = sum(len(x) for x in w)
        out, begin, count, needed = lk.lookup_ids_raw(t, ANY, 50 * total)  # the output buffer grows
        assert needed == total and all(np.array_equal(g, x) for g, x in zip(split(out, begin, count), w))
        assert lk.stats()["tier2_rounds"] == 9 and lk.stats()["uploads"] == 1


def test_writes_are_seen_by_the_next_call(tiers):
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
            LC.sid("doc3", "view", "bob")]
    rows += [LC.sset(f"h{i}", "view", "h", "member") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    alice = rt.SubjectID("alice")
    with lookup.Lookup(snap) as lk:
        assert lk.ListObjects("n", "view", alice) == ["doc1"]
        assert lk.stats()["uploads"] == 1
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert lk.ListObjects("n", "view", alice) == sorted(["doc1"] + [f"h{i}" for i in range(40)])
        assert lk.stats()["uploads"] == 2
        assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (reserved id)
        assert len(lk.ListObjects("n", "view", rt.SubjectID("carol"))) == 40
        assert lk.stats()["uploads"] == 3
        ids = [v for v in range(snap.stats()["num_nodes"])]
        real = []
        for v in ids:  # every node but the placeholders, as the host lists them
            try:
                snap.describe(v)
                real.append(v)
            except L.KetoError:
                pass
        assert len(real) == len(ids) - 3
        assert_call_matches(lk, snap, np.array(real, dtype=np.uint32), ANY)
        assert lk.stats()["uploads"] == 3  # no write since: no upload


def test_handle_outlives_its_snapshot():
    snap = Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])
    lk = lookup.Lookup(snap)
    assert len(lk.lookup_ids([0])) == 1
    lk.snapshot = None
    del snap
    gc.collect()
    with pytest.raises(L.KetoError) as e:  # the rows in HBM are a copy, but the version cannot be read
        lk.lookup_ids_raw(np.zeros(1, dtype=np.uint32), ANY, 4)
    assert e.value.code == L.EINVAL
    lk.close()
