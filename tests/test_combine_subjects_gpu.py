"""Combined subject lists on the device (ketogpu_subjects_combine / _combine_page,
keto_amd/csrc/combine.hpp) against numpy set algebra over the host lists
(ketogpu_snapshot_subjects), which test_combine_host.py pins against the oracle.  The
comparisons are exact: lists are compared as sorted arrays."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import combine_cases as CC
from tests import lookup_cases as LC
from tests import subjects_cases as SC
from tests import test_subjects_gpu as TS

pytestmark = pytest.mark.gpu
ANY, IDS, NONE = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID, L.NODE_NONE
AND, ANDNOT, OR = lookup.OP_AND, lookup.OP_ANDNOT, lookup.OP_OR
S = CC.SubjectsSide


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["default", "tier2"])
def tiers(request, monkeypatch):
    """handles created while active: the default tiers, or every request through tier 2"""
    if request.param == "tier2":
        monkeypatch.setenv(S.tier_env, "2")
    return request.param


def tier_delta(h, call):
    """(tier-1, tier-2) requests that call() adds to the combined stats"""
    before = h.combine_stats()
    call()
    after = h.combine_stats()
    return (after["tier1_requests"] - before["tier1_requests"], after["tier2_requests"] - before["tier2_requests"])


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables_on_the_device(case, tiers):
    _, _, snap = LC.table(*case)
    a, b = CC.pair_sample(snap.stats()["num_nodes"], case[0])  # never-expanded roots included
    m = CC.Members(S, snap)
    skipped = CC.unlisted(S, snap, a, b)
    assert 0 < skipped < len(a)
    with S.Handle(snap) as h:
        plain = h.stats()
        for op in CC.OP_IDS:
            CC.assert_combined(h, a, b, op, ANY, m.want(a, b, op))
        CC.assert_combined(h, a, b, AND, IDS, m.want(a, b, AND, IDS))
        st = h.combine_stats()
        assert st["requests"] == 4 * len(a)
        assert st["tier1_requests"] + st["tier2_requests"] + 4 * skipped == st["requests"]
        if tiers == "tier2":
            assert st["tier1_requests"] == 0
        assert h.stats() == plain  # combined calls count in their own struct


@functools.lru_cache(maxsize=None)
def boundary():
    snap = Snapshot.from_rows(LC.NS1, CC.boundary_rows(S))
    return snap, {k: S.node(snap, k) for k in ("s1024", "s1025", "d512a", "d512b", "d513", "ov_a", "ov_b", "ov_c")}


def test_tier_boundary():
    snap, v = boundary()
    m = CC.Members(S, snap)
    assert [len(m(v[k])) for k in ("s1024", "s1025", "d512a", "d513", "ov_a", "ov_b", "ov_c")] == \
        [1024, 1025, 512, 513, 700, 700, 700]
    with S.Handle(snap) as h:
        assert h.stats()["set_capacity"] == 1024

        def one(x, y, op):
            a, b = np.array([v[x]], dtype=np.uint32), np.array([v[y]], dtype=np.uint32)
            want = m.want(a, b, op)
            return tier_delta(h, lambda: CC.assert_combined(h, a, b, op, ANY, want)), want[0]

        for op in CC.OP_IDS:
            assert one("s1024", "s1024", op)[0] == (1, 0), op
        for op in (AND, ANDNOT):  # the overflow is found on either side
            assert one("s1024", "s1025", op)[0] == (0, 1), op
            assert one("s1025", "s1024", op)[0] == (0, 1), op
        assert one("d512a", "d512b", OR)[0] == (1, 0)
        assert one("d512a", "d513", OR)[0] == (0, 1)
        t, want = one("ov_a", "ov_b", OR)  # the union decides, not the sum
        assert t == (1, 0) and len(want) == 1024
        t, want = one("ov_a", "ov_c", OR)
        assert t == (0, 1) and len(want) == 1025
        t, want = one("ov_a", "ov_b", AND)
        assert t == (1, 0) and len(want) == 376
        t, want = one("ov_a", "ov_b", ANDNOT)
        assert t == (1, 0) and len(want) == 324


@functools.lru_cache(maxsize=None)
def structure():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    return snap, S.structure(snap)


def test_structure_cases(tiers):
    snap, v = structure()
    m = CC.Members(S, snap)
    with S.Handle(snap) as h:
        one = lambda x, y, op: h.combine_ids([x], [y], op)[0]
        for name in ("cycle", "self"):  # a is a member of its own side
            x = v[name]
            assert x in m(x) and x in one(x, x, AND) and x in one(x, NONE, OR) and x not in one(x, x, ANDNOT)
        chain, mid = v["chain"], v["mid"]
        assert len(m(chain)) == v["chain_size"] and 0 < len(m(mid)) < len(m(chain))
        assert np.array_equal(one(chain, mid, AND), m(mid))  # the smaller closure
        rest = one(chain, mid, ANDNOT)
        assert len(rest) == len(m(chain)) - len(m(mid)) and np.array_equal(rest, np.setdiff1d(m(chain), m(mid)))
        assert np.array_equal(one(mid, chain, OR), m(chain))
        d = v["diamond"]  # ids arrive from two rows
        assert len(one(d, d, OR)) == v["diamond_size"] and len(one(d, chain, AND)) == 0
        assert np.array_equal(one(d, chain, OR), np.union1d(m(d), m(chain)))
        two = S.node(snap, "two")  # a document held through two groups that share half their members
        assert np.array_equal(one(two, two, AND), m(two)) and len(m(two)) == 42


def test_degenerate_pairs(tiers):
    snap, v = structure()
    n = snap.stats()["num_nodes"]
    m = CC.Members(S, snap)
    x, y = v["chain"], v["diamond"]
    leaf = int(lookup.resolve_subjects(snap, [rt.SubjectID("uc")])[0])  # a never-expanded root
    assert snap.stats()["num_expandable"] <= leaf < n
    a = np.array([x, x, NONE, NONE, x, n + 5, y, y, leaf, x, leaf, leaf], dtype=np.uint32)
    b = np.array([x, NONE, x, NONE, n + 5, y, x, y, x, leaf, leaf, NONE], dtype=np.uint32)
    valid = [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
    with S.Handle(snap) as h:
        for op in CC.OP_IDS:
            want = m.want(a[valid], b[valid], op)
            assert len(want[6]) == (len(m(x)) if op == OR else 0) and len(want[8]) == 0
            total = sum(len(w) for w in want)
            before = h.combine_stats()
            out, begin, count, needed = h.combine_ids_raw(a, b, op, ANY, total)
            assert needed == total
            assert (begin[[4, 5]] == lookup.INVALID).all() and not count[[4, 5]].any()
            got = CC.split(out, begin, count)
            for k, w in zip(valid, want):  # the other pairs of the batch are unaffected
                assert np.array_equal(got[k], w), (op, k)
            after = h.combine_stats()  # INVALID pairs and pairs without a row belong to neither tier
            assert after["tier1_requests"] + after["tier2_requests"] - before["tier1_requests"] \
                - before["tier2_requests"] == len(a) - 5
            _, returned, cnt, rem = h.combine_page_raw(a, b, op, None, ANY, 7)
            assert (returned[[4, 5]] == lookup.PAGE_INVALID).all() and not cnt[[4, 5]].any() and not rem[[4, 5]].any()
            assert [int(c) for c in cnt[valid]] == [len(w) for w in want]
            with pytest.raises(L.KetoError) as e:
                h.combine_ids(a, b, op)
            assert e.value.code == L.EINVAL
            for nothing in (lookup.TYPE_NONE, lookup.CLASS_UNTYPED_SET):
                out, begin, count, needed = h.combine_ids_raw(a[valid], b[valid], op, nothing, 16)
                assert needed == 0 and not count.any()
        assert np.array_equal(h.combine_ids([x], [x], AND)[0], m(x)) and len(h.combine_ids([x], [x], ANDNOT)[0]) == 0
        for call in (lambda: h.combine_ids_raw(a, b, 3, ANY, 0), lambda: h.combine_page_raw(a, b, 3, None, ANY, 7)):
            with pytest.raises(L.KetoError) as e:
                call()
            assert e.value.code == L.EINVAL
        out, begin, count, needed = h.combine_ids_raw(np.zeros(0, np.uint32), np.zeros(0, np.uint32), AND, ANY, 8)
        assert needed == 0 and len(begin) == 0


def test_slots_and_clearing(monkeypatch):
    """every exit path leaves both bitmaps of a slot all zero: whatever runs next on the handle,
    combined or plain (by list or by scan), answers as the host does"""
    monkeypatch.setenv(S.tier_env, "2")
    monkeypatch.setenv(S.slots_env, "2")
    snap, v = structure()
    m = CC.Members(S, snap)
    names = ["chain", "mid", "diamond", "cycle", "self"]
    a = np.array([v[k] for k in names], dtype=np.uint32)
    b = np.array([v[k] for k in names[1:] + names[:1]], dtype=np.uint32)
    plain = [m(x) for x in a]
    with S.Handle(snap) as h:
        TS.assert_call_matches(h, snap, a, ANY, plain)
        CC.assert_combined(h, a, b, AND, ANY, m.want(a, b, AND))
        st = h.combine_stats()
        assert st["tier2_requests"] == 5 and st["tier2_rounds"] == 3 and st["slots"] == 2
        want = m.want(a, b, ANDNOT)
        total = sum(len(w) for w in want)
        out, begin, count, needed = h.combine_ids_raw(a, b, ANDNOT, ANY, total - 1)
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert (begin == lookup.TRUNCATED).any()
        for g, w in zip(CC.split(out, begin, count), want):
            assert g is None or np.array_equal(g, w)
        CC.assert_pages(h, a, b, OR, None, ANY, 7, m.want(a, b, OR))
        CC.assert_pages(h, a, a, AND, None, ANY, 100, plain)
        out, returned, count, remaining = h.subject_page_raw(a, None, ANY, 100)
        for k, w in enumerate(plain):
            assert int(count[k]) == len(w) and np.array_equal(out[k, :int(returned[k])], w[:100])
        TS.assert_call_matches(h, snap, a, ANY, plain)
        assert h.combine_stats()["tier2_rounds"] == 12


def test_truncation_protocol(tiers):
    snap = TS.workload("rbac")
    rng = np.random.default_rng(11)
    n = S.sample_bound(snap)
    a, b = rng.integers(0, n, 100).astype(np.uint32), rng.integers(0, n, 100).astype(np.uint32)
    m = CC.Members(S, snap)
    want = m.want(a, b, AND, IDS)
    total = sum(len(w) for w in want)
    assert total > 0
    with S.Handle(snap) as h:
        out, begin, count, needed = h.combine_ids_raw(a, b, AND, IDS, 0)  # count only
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert all(bg == lookup.TRUNCATED for bg, w in zip(begin, want) if len(w))
        before = h.combine_stats()["truncated_lists"]
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = h.combine_ids_raw(a, b, AND, IDS, cap)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
            assert (begin == lookup.TRUNCATED).any()
            for g, w, bg in zip(CC.split(out, begin, count), want, begin):
                if g is not None:  # a list that was written is complete
                    assert np.array_equal(g, w) and int(bg) + len(w) <= cap
        assert h.combine_stats()["truncated_lists"] > before
        calls = h.combine_stats()["requests"]
        got = h.combine_ids(a, b, AND, IDS, capacity=1000)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert h.combine_stats()["requests"] - calls <= 2 * len(a)  # no list is asked for more than twice


def test_pages():
    snap, v = boundary()
    m = CC.Members(S, snap)
    n = snap.stats()["num_nodes"]
    a = np.array([v["s1025"], v["ov_a"]], dtype=np.uint32)  # an overflowing and a tier-1 pair
    b = np.array([v["ov_a"], v["ov_b"]], dtype=np.uint32)
    with S.Handle(snap) as h:
        assert tier_delta(h, lambda: h.combine_page_raw(a, b, OR, None, ANY, 1)) == (1, 1)
        for op in CC.OP_IDS:
            want = m.want(a, b, op)
            member, other = int(want[1][len(want[1]) // 2]), int(m(v["d513"])[0])
            assert other not in want[0] and other not in want[1]
            for limit in (1, 7, 100):
                for f in (0, member, other, n, 0xFFFFFFFF):
                    CC.assert_pages(h, a, b, op, np.full(2, f, dtype=np.uint32), ANY, limit, want)
        for x, y in (("s1025", "ov_a"), ("ov_a", "ov_b")):  # the page walk ends with ""
            ra, rb = ("n", x, "view"), ("n", y, "view")
            full = h.ListSubjectsCombined(ra, rb, "or")
            assert full == lookup.HostSubjects(snap).ListSubjectsCombined(ra, rb, "or") and len(full) >= 1024
            items, token, pages = [], "", 0
            while True:
                page, token, total = h.list_subjects_combined_page(ra, rb, "or", "ids", 700, token)
                items += page
                pages += 1
                assert total == len(full)
                if token == "":
                    break
            assert sorted(s.id for s in items) == [s.id for s in full] and pages == -(-len(full) // 700)


@pytest.mark.parametrize("kind", ["rbac", "folders"])
def test_synthetic_workloads_match_the_host(kind):
    snap = TS.workload(kind)
    m = CC.Members(S, snap)
    n = S.sample_bound(snap)
    ty = snap.type_id(*TS.WORKLOADS[kind][1])
    with S.Handle(snap) as h:
        cap = h.stats()["set_capacity"]
        for op in CC.OP_IDS:
            rng = np.random.default_rng(70 + op)
            a, b = rng.integers(0, n, 500).astype(np.uint32), rng.integers(0, n, 500).astype(np.uint32)
            want = m.want(a, b, op)
            if op == OR:  # a pair passes the LDS set exactly when the union does
                over = sum(len(w) > cap for w in want)
            else:  # ... or when either side does
                over = sum(len(m(x)) > cap or len(m(y)) > cap for x, y in zip(a, b))
            if kind == "folders":  # (no forward closure of this workload passes the set)
                assert over == 0, "the folders sample stays in tier 1"
            else:
                assert 0 < over < len(a), "the sample uses both tiers"
            assert tier_delta(h, lambda: CC.assert_combined(h, a, b, op, ANY, want)) == (len(a) - over, over)
            for filt in (IDS, ty):
                typed = m.want(a, b, op, filt)
                CC.assert_combined(h, a, b, op, filt, typed)
                assert sum(len(w) for w in typed) <= sum(len(w) for w in want)


def test_writes_are_seen_by_the_next_call(tiers):
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("doc1", "view", "bob"),
            LC.sid("doc2", "view", "bob"), LC.sset("doc2", "view", "h", "member")]
    rows += [LC.sid("h", "member", f"m{i}") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    d1, d2 = ("n", "doc1", "view"), ("n", "doc2", "view")
    ids = lambda subs: [s.id for s in subs]
    with S.Handle(snap) as h:
        assert ids(h.ListSubjectsCombined(d1, d2, "and")) == ["bob"]
        assert ids(h.ListSubjectsCombined(d1, d2, "andnot")) == ["alice"]
        assert snap.write([LC.sid("g", "member", "m7")])["applied"]
        assert ids(h.ListSubjectsCombined(d1, d2, "and")) == ["bob", "m7"]
        assert ids(h.ListSubjectsCombined(d2, d1, "andnot")) == sorted(f"m{i}" for i in range(40) if i != 7)
        assert len(h.ListSubjectsCombined(d1, d2, "or")) == 42
        assert h.stats()["uploads"] == 2
