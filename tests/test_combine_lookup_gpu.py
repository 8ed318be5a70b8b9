"""Combined object lists on the device (ketogpu_lookup_combine / _combine_page,
keto_amd/csrc/combine.hpp) against numpy set algebra over the host lists
(ketogpu_snapshot_lookup), which test_combine_host.py pins against the oracle.  The comparisons
are exact: lists are compared as sorted arrays."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import combine_cases as CC
from tests import lookup_cases as LC
from tests import test_lookup_gpu as TL

pytestmark = pytest.mark.gpu
ANY, NONE = lookup.TYPE_ANY, L.NODE_NONE
AND, ANDNOT, OR = lookup.OP_AND, lookup.OP_ANDNOT, lookup.OP_OR
S = CC.LookupSide


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
    a, b = CC.pair_sample(S.sample_bound(snap), case[0])
    m = CC.Members(S, snap)
    skipped = CC.unlisted(S, snap, a, b)
    with S.Handle(snap) as h:
        plain = h.stats()
        for op in CC.OP_IDS:
            CC.assert_combined(h, a, b, op, ANY, m.want(a, b, op))
        st = h.combine_stats()
        assert st["requests"] == 3 * len(a)
        assert st["tier1_requests"] + st["tier2_requests"] + 3 * skipped == st["requests"]
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
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows())
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


def test_degenerate_pairs(tiers):
    snap, v = structure()
    n = snap.stats()["num_nodes"]
    m = CC.Members(S, snap)
    x, y = v["chain"], v["diamond"]
    a = np.array([x, x, NONE, NONE, x, n + 5, y, y], dtype=np.uint32)
    b = np.array([x, NONE, x, NONE, n + 5, y, x, y], dtype=np.uint32)
    valid = [0, 1, 2, 3, 6, 7]
    with S.Handle(snap) as h:
        for op in CC.OP_IDS:
            want = m.want(a[valid], b[valid], op)
            total = sum(len(w) for w in want)
            before = h.combine_stats()
            out, begin, count, needed = h.combine_ids_raw(a, b, op, ANY, total)
            assert needed == total
            assert (begin[[4, 5]] == lookup.INVALID).all() and not count[[4, 5]].any()
            got = CC.split(out, begin, count)
            for k, w in zip(valid, want):  # the other pairs of the batch are unaffected
                assert np.array_equal(got[k], w), (op, k)
            after = h.combine_stats()  # INVALID pairs and NONE with NONE belong to neither tier
            assert after["tier1_requests"] + after["tier2_requests"] - before["tier1_requests"] \
                - before["tier2_requests"] == len(a) - 3
            _, returned, cnt, rem = h.combine_page_raw(a, b, op, None, ANY, 7)
            assert (returned[[4, 5]] == lookup.PAGE_INVALID).all() and not cnt[[4, 5]].any() and not rem[[4, 5]].any()
            assert [int(c) for c in cnt[valid]] == [len(w) for w in want]
            with pytest.raises(L.KetoError) as e:
                h.combine_ids(a, b, op)
            assert e.value.code == L.EINVAL
            out, begin, count, needed = h.combine_ids_raw(a[valid], b[valid], op, lookup.TYPE_NONE, 16)
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
    combined or plain, answers as the host does"""
    monkeypatch.setenv(S.tier_env, "2")
    monkeypatch.setenv(S.slots_env, "2")
    snap, v = structure()
    m = CC.Members(S, snap)
    names = ["chain", "mid", "diamond", "cycle", "self"]
    a = np.array([v[k] for k in names], dtype=np.uint32)
    b = np.array([v[k] for k in names[1:] + names[:1]], dtype=np.uint32)
    plain = [m(x) for x in a]
    with S.Handle(snap) as h:
        TL.assert_call_matches(h, snap, a, ANY, plain)
        CC.assert_combined(h, a, b, AND, ANY, m.want(a, b, AND))
        st = h.combine_stats()
        assert st["tier2_requests"] == 5 and st["tier2_rounds"] == 3 and st["slots"] == 2
        roots = np.array([m(x)[0] for x in a], dtype=np.uint32)  # a member of each list: an allowed pair
        for ids, r, t in zip(h.path_ids(roots, a), roots, a):
            assert len(ids) == len(lookup.host_path(snap, int(r), int(t))) >= 2
        want = m.want(a, b, ANDNOT)
        total = sum(len(w) for w in want)
        out, begin, count, needed = h.combine_ids_raw(a, b, ANDNOT, ANY, total - 1)
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert (begin == lookup.TRUNCATED).any()
        for g, w in zip(CC.split(out, begin, count), want):
            assert g is None or np.array_equal(g, w)
        CC.assert_pages(h, a, b, OR, None, ANY, 7, m.want(a, b, OR))
        CC.assert_pages(h, a, a, AND, None, ANY, 100, plain)
        out, returned, count, remaining = h.lookup_page_raw(a, None, ANY, 100)
        for k, w in enumerate(plain):
            assert int(count[k]) == len(w) and np.array_equal(out[k, :int(returned[k])], w[:100])
        TL.assert_call_matches(h, snap, a, ANY, plain)
        assert h.combine_stats()["tier2_rounds"] == 12


def test_truncation_protocol(tiers):
    snap = TL.workload("rbac")
    rng = np.random.default_rng(11)
    n = S.sample_bound(snap)
    a, b = rng.integers(0, n, 300).astype(np.uint32), rng.integers(0, n, 300).astype(np.uint32)
    m = CC.Members(S, snap)
    want = m.want(a, b, OR)
    total = sum(len(w) for w in want)
    with S.Handle(snap) as h:
        out, begin, count, needed = h.combine_ids_raw(a, b, OR, ANY, 0)  # count only
        assert needed == total and [int(c) for c in count] == [len(w) for w in want]
        assert all(bg == lookup.TRUNCATED for bg, w in zip(begin, want) if len(w))
        before = h.combine_stats()["truncated_lists"]
        for cap in (total - 1, total // 2, 1):
            out, begin, count, needed = h.combine_ids_raw(a, b, OR, ANY, cap)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
            assert (begin == lookup.TRUNCATED).any()
            for g, w, bg in zip(CC.split(out, begin, count), want, begin):
                if g is not None:  # a list that was written is complete
                    assert np.array_equal(g, w) and int(bg) + len(w) <= cap
        assert h.combine_stats()["truncated_lists"] > before
        calls = h.combine_stats()["requests"]
        got = h.combine_ids(a, b, OR, ANY, capacity=1000)
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
            sa, sb = rt.SubjectID(x), rt.SubjectID(y)
            full = h.ListObjectsCombined("n", "view", sa, sb, "or")
            assert full == lookup.HostLookup(snap).ListObjectsCombined("n", "view", sa, sb, "or") and len(full) >= 1024
            items, token, pages = [], "", 0
            while True:
                page, token, total = h.list_objects_combined_page("n", "view", sa, sb, "or", 700, token)
                items += page
                pages += 1
                assert total == len(full)
                if token == "":
                    break
            assert sorted(items) == full and pages == -(-len(full) // 700)


@pytest.mark.parametrize("kind", ["rbac", "folders"])
def test_synthetic_workloads_match_the_host(kind):
    snap = TL.workload(kind)
    m = CC.Members(S, snap)
    n = S.sample_bound(snap)
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
            assert 0 < over < len(a), "the sample uses both tiers"
            assert tier_delta(h, lambda: CC.assert_combined(h, a, b, op, ANY, want)) == (len(a) - over, over)
            for ns, rel in TL.WORKLOADS[kind][1]:
                ty = snap.type_id(ns, rel)
                typed = m.want(a, b, op, ty)
                CC.assert_combined(h, a, b, op, ty, typed)
                assert sum(len(w) for w in typed) <= sum(len(w) for w in want)


def test_writes_are_seen_by_the_next_call(tiers):
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
            LC.sid("doc3", "view", "bob")]
    rows += [LC.sset(f"h{i}", "view", "h", "member") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    alice, bob = rt.SubjectID("alice"), rt.SubjectID("bob")
    with S.Handle(snap) as h:
        assert h.ListObjectsCombined("n", "view", alice, bob, "and") == []
        assert h.ListObjectsCombined("n", "view", bob, alice, "andnot") == sorted(["doc3"] + [f"h{i}" for i in range(40)])
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert h.ListObjectsCombined("n", "view", alice, bob, "and") == sorted(f"h{i}" for i in range(40))
        assert h.ListObjectsCombined("n", "view", bob, alice, "andnot") == ["doc3"]
        assert h.ListObjectsCombined("n", "view", alice, bob, "or") == \
            sorted(["doc1", "doc3"] + [f"h{i}" for i in range(40)])
        assert h.stats()["uploads"] == 2
