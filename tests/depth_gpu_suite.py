"""The device tests of the depth-limited listings, written once for both handles:
test_depth_lookup_gpu.py and test_depth_subjects_gpu.py import every test here and supply the
fixture `side` (depth_cases.LookupSide / SubjectsSide).  The yardstick is depth_cases.Truth (the
plain host list restricted by one shortest-path call per member); the synthetic workloads use
the host twins, which test_depth_host.py pins against it.  The comparisons are exact: lists are
compared as sorted arrays, frontiers and tier counts as numbers."""
import ctypes as C

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd.snapshot import Snapshot
from tests import combine_cases as CC
from tests import depth_cases as DC
from tests import lookup_cases as LC

ANY, NONE, ALL = DC.ANY, DC.NONE, DC.ALL


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["default", "tier2"])
def tiers(request, side, monkeypatch):
    """handles created while active: the default tiers, or every request through tier 2"""
    if request.param == "tier2":
        monkeypatch.setenv(side.tier_env, "2")
    return request.param


def u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def assert_tiers(h, tiers, truth, ids, depth, call, unlisted=0):
    """call() moves the depth stats by the tiers the yardstick predicts (forced tier 2: all
    listed requests), and the plain stats not at all"""
    plain = h.stats()
    t1, t2 = DC.depth_tiers(truth, ids, depth, plain["set_capacity"])
    got = DC.tier_delta(h, call)
    listed = len(ids) - unlisted
    assert got == ((0, listed) if tiers == "tier2" else (t1 - unlisted, t2)), (got, t1, t2, unlisted)
    assert h.stats() == plain  # depth calls count in their own struct


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables_on_the_device(case, side, tiers):
    snap, truth = DC.table_truth(side.name, case)
    starts = np.arange(side.sample_bound(snap), dtype=np.uint32)
    ids, depth = np.repeat(starts, len(DC.DEPTHS)), u32(np.tile(DC.DEPTHS, len(starts)))
    want, wfr = truth.want(ids, depth)
    with side.Handle(snap) as h:
        assert_tiers(h, tiers, truth, ids, depth, lambda: DC.assert_depth(side, h, ids, depth, ANY, want, wfr))
        st = h.depth_stats()
        assert st["requests"] == len(ids) and st["cut_requests"] == sum(f > 0 for f in wfr) > 0
        assert st["ids_produced"] == sum(len(w) for w in want) and st["truncated_lists"] == 0
        # a null depth array is no limit for every request: the plain call's sets
        every = [side.host(snap, int(x), ANY) for x in starts]
        DC.assert_depth(side, h, starts, None, ANY, every, [0] * len(starts), null_depth=True)


def test_level_boundaries_in_tier_1(side, tiers):
    """the chain of 6 at k = 1 .. 7; start rows of 65 and 129 entries (the level ends inside and
    at the end of a 64-entry step); a level whose last row adds nothing; the cycle of 3; the
    last level without rows; and from the structure graph the diamond and the self-loop"""
    snap, truth, v = DC.levels(side.name)
    names = ["chain", "w65", "w129", "empty_last", "cycle", "leaf_level"]
    ids, depth = [], []
    for name in names:
        ks = list(range(1, truth.eccentricity(v[name]) + 2)) + [ALL]
        ids += [v[name]] * len(ks)
        depth += ks
    ids, depth = u32(ids), u32(depth)
    want, wfr = truth.want(ids, depth)
    with side.Handle(snap) as h:
        assert_tiers(h, tiers, truth, ids, depth, lambda: DC.assert_depth(side, h, ids, depth, ANY, want, wfr))
        one = lambda x, k: side.lists(h, [x], [k])
        chain = v["chain"]
        assert [len(one(chain, k)[0][0]) for k in range(1, 8)] == [1, 2, 3, 4, 5, 6, 6]
        cyc = v["cycle"]  # the start is a member only through a cycle of at most k hops
        assert cyc not in one(cyc, 2)[0][0] and cyc in one(cyc, 3)[0][0]
        for name in ("w65", "w129"):
            k = int(name[1:])
            assert [len(one(v[name], d)[0][0]) for d in (1, 2)] == [k, 2 * k]
            assert [int(one(v[name], d)[1][0]) for d in (1, 2)] == [k, 0]
    snap, _, truth, v = DC.structure(side.name)
    with side.Handle(snap) as h:
        x, d = v["self"], v["diamond"]
        lists, fr = side.lists(h, [x, d, d, d, d], [1, 1, 2, 3, ALL])
        assert x in lists[0]  # a self-loop: a member of its own list at one hop
        want, wfr = truth.want([x, d, d, d, d], [1, 1, 2, 3, ALL])
        assert all(np.array_equal(g, w) for g, w in zip(lists, want)) and [int(f) for f in fr] == wfr
        assert len(lists[2]) == 3 and len(lists[3]) == 4  # ids that arrive from two rows of one level


def test_frontier(side, tiers):
    snap, truth, v = DC.levels(side.name)
    with side.Handle(snap) as h:
        for name in ("chain", "w65", "empty_last", "cycle", "fan"):
            x, ecc = v[name], truth.eccentricity(v[name])
            lists, fr = side.lists(h, [x, x], [ecc, ecc - 1])
            assert np.array_equal(lists[0], truth.members(x, ALL)), name
            # the cycle's last level is the start itself, an interior member: its row is unread
            assert int(fr[0]) == truth.frontier(x, ecc) == (1 if name == "cycle" else 0), name
            assert int(fr[1]) == truth.frontier(x, ecc - 1) > 0, name
        leaf = v["leaf_level"]  # a last level made of members without a row: nothing is unread
        lists, fr = side.lists(h, [leaf, leaf], [2, 1])
        assert len(lists[0]) == 3 and [int(f) for f in fr] == [0, 1]
        assert h.depth_stats()["cut_requests"] == 7


def test_tier_rule(side):
    """a request goes to tier 2 exactly when its unfiltered M_k passes the set capacity"""
    snap, truth, v = DC.levels(side.name)
    with side.Handle(snap) as h:
        def one(name, k):
            x = u32([v[name]])
            want, wfr = truth.want(x, [k])
            before = h.depth_stats()
            DC.assert_depth(side, h, x, u32([k]), ANY, want, wfr)
            after = h.depth_stats()
            got = (after["tier1_requests"] - before["tier1_requests"], after["tier2_requests"] - before["tier2_requests"])
            assert got == DC.depth_tiers(truth, x, [k], h.stats()["set_capacity"])
            return got, len(want[0])

        assert one("s1024", 1) == ((1, 0), 1024)
        assert one("s1025", 1) == ((0, 1), 1025)
        assert one("s1024", ALL) == ((1, 0), 1024)
        # a star of 30 over a closure of 1050: the near part finishes in LDS
        assert one("fan", 1) == ((1, 0), 30)
        assert one("fan", 2) == ((0, 1), 1050)
        assert one("fan", ALL) == ((0, 1), 1050)
        plain = h.stats()
        assert plain["tier1_requests"] == plain["tier2_requests"] == 0
        out, begin, count, needed = side.plain_raw(h, u32([v["fan"]]), ANY, 1050)
        assert needed == 1050 and h.stats()["tier2_requests"] == 1  # the plain call goes to tier 2


def check_chain(side, h, finish=None):
    """the 3000-chain at k = 1, 2999, 3000, 3001 and no limit on handle h"""
    snap, _, truth, v = DC.structure(side.name)
    chain, size = v["chain"], v["chain_size"]
    depth = u32([1, size - 1, size, size + 1, ALL])
    ids = u32([chain] * len(depth))
    want, wfr = truth.want(ids, depth)
    assert [len(w) for w in want] == [1, size - 1, size, size, size] and wfr == [1, 1, 0, 0, 0]
    before = h.depth_stats()
    DC.assert_depth(side, h, ids, depth, ANY, want, wfr)
    DC.assert_pages(side, h, ids, depth, u32([0, 5, 2000, 0, 2990]), ANY, 100, want, wfr)
    after = h.depth_stats()
    if finish is not None:
        other = "scan_finishes" if finish == "list_finishes" else "list_finishes"
        assert after[finish] - before[finish] == after["tier2_requests"] - before["tier2_requests"] > 0
        assert after[other] == before[other]
    return after


def test_tier2_chain(side, tiers):
    snap = DC.structure(side.name)[0]
    with side.Handle(snap) as h:
        st = check_chain(side, h, "list_finishes" if side.list_cap_env else None)
        if side.list_cap_env is None:
            assert st["list_finishes"] == st["scan_finishes"] == 0
        # default tiers: k = 1 stays in LDS, the four longer lists pass the set
        assert st["tier1_requests"] == (0 if tiers == "tier2" else 2)


def raw_null_frontier(side, h, ids, depth, filt, cap):
    """the cursor call with frontier = NULL, as the ABI allows"""
    ids, depth = u32(ids), u32(depth)
    n = len(ids)
    out = np.empty(max(cap, 1), dtype=np.uint32)
    begin, count = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    needed = C.c_uint64()
    L.check(h._abi("ids_depth")(h.h, ids.ctypes.data, depth.ctypes.data, n, int(filt), out.ctypes.data, cap,
                                begin.ctypes.data, count.ctypes.data, None, C.byref(needed)))
    return out[:cap], begin, count, needed.value


def test_mixed_depths_in_one_call(side, tiers):
    """the same id at k = 1, 2 and no limit, next to NONE, a node without a row of its own (on
    the subjects handle: a never-expanded root) and an id outside the snapshot"""
    snap, truth, v = DC.levels(side.name)
    n = snap.stats()["num_nodes"]
    x = v["w65"]
    ids = u32([x, NONE, x, n - 1, x, n + 5, v["chain"]])
    depth = u32([1, 1, 2, 2, ALL, 1, 3])
    valid = [0, 1, 2, 3, 4, 6]
    want, wfr = truth.want(ids[valid], depth[valid])
    total = sum(len(w) for w in want)
    assert [len(w) for w in want][:3] == [65, 0, 130]
    unlisted = 2  # NONE and INVALID belong to neither tier, as in the plain call
    with side.Handle(snap) as h:
        before = h.depth_stats()
        out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, total)
        assert needed == total and begin[5] == lookup.INVALID and count[5] == 0 and frontier[5] == 0
        assert begin[1] == 0 and count[1] == 0 and frontier[1] == 0
        got = DC.split(out, begin, count)
        for k, w, f in zip(valid, want, wfr):
            assert np.array_equal(got[k], w) and int(frontier[k]) == f, k
        after = h.depth_stats()
        assert after["tier1_requests"] + after["tier2_requests"] - before["tier1_requests"] \
            - before["tier2_requests"] == len(ids) - unlisted
        assert after["cut_requests"] - before["cut_requests"] == sum(f > 0 for f in wfr)
        out, begin, count, needed = raw_null_frontier(side, h, ids, depth, ANY, total)  # frontier = NULL
        assert needed == total and begin[5] == lookup.INVALID
        assert all(np.array_equal(g, w) for g, w in zip([DC.split(out, begin, count)[k] for k in valid], want))
        assert h.depth_stats()["cut_requests"] - after["cut_requests"] == sum(f > 0 for f in wfr)
        _, returned, cnt, rem, fr = side.page(h, ids, depth, None, ANY, 7)
        assert returned[5] == lookup.PAGE_INVALID and not cnt[5] and not rem[5] and not fr[5]
        assert [int(c) for c in cnt[valid]] == [len(w) for w in want] and [int(f) for f in fr[valid]] == wfr
        with pytest.raises(L.KetoError) as e:
            side.lists(h, ids, depth)
        assert e.value.code == L.EINVAL
        # empty batches and the argument checks of the plain calls
        out, begin, count, frontier, needed = side.raw(h, u32([]), u32([]), ANY, 0)
        assert needed == 0 and len(begin) == 0
        with pytest.raises(L.KetoError):
            side.page(h, ids, depth, None, ANY, 0)
        with pytest.raises(L.KetoError):
            side.page(h, ids, depth, None, ANY, lookup.PAGE_LIMIT_MAX + 1)


def test_truncation_protocol_and_count_only(side, tiers):
    snap, truth, v = DC.levels(side.name)
    ids = u32([v["w129"], v["chain"], v["w65"], v["w129"], v["fan"]])
    depth = u32([1, 4, 2, ALL, 2])
    want, wfr = truth.want(ids, depth)
    sizes = [len(w) for w in want]
    total = sum(sizes)
    with side.Handle(snap) as h:
        out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, 0)  # capacity 0 counts only
        assert needed == total and [int(c) for c in count] == sizes and (begin == lookup.TRUNCATED).all()
        assert [int(f) for f in frontier] == wfr
        cap = total - 1  # whichever list reserves last does not fit, every other one does
        before = h.depth_stats()["truncated_lists"]
        out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, cap)
        assert needed == total and [int(c) for c in count] == sizes and [int(f) for f in frontier] == wfr
        trunc = begin == lookup.TRUNCATED
        assert trunc.sum() == 1
        assert h.depth_stats()["truncated_lists"] - before == int(trunc.sum())
        for k in np.nonzero(~trunc)[0]:  # a list is written completely or marked
            b = int(begin[k])
            assert b + sizes[k] <= cap and np.array_equal(np.sort(out[b:b + sizes[k]]), want[k])
        lists, fr = side.lists(h, ids, depth)  # the re-issue loop ends with every list
        assert all(np.array_equal(g, w) for g, w in zip(lists, want)) and [int(f) for f in fr] == wfr
        lists, fr = h.lookup_depth(ids, depth, ANY, capacity=1) if side.name == "lookup" else \
            h.subject_depth(ids, depth, ANY, capacity=1)
        assert all(np.array_equal(g, w) for g, w in zip(lists, want)) and [int(f) for f in fr] == wfr


def test_pages(side, tiers):
    """walking a depth-limited list to its end concatenates to the sorted M_k"""
    snap, truth, v = DC.levels(side.name)
    x = v["w129"]
    with side.Handle(snap) as h:
        for k in (1, 2):
            for limit in (1, 7, 100):
                if limit == 1 and k == 2:
                    continue  # (258 one-id calls show nothing that 129 do not)
                got, calls = DC.walk_pages(side, h, x, k, ANY, limit)
                assert np.array_equal(got, truth.members(x, k)), (k, limit)
                assert calls == -(-len(got) // limit)
        ids = u32([x, x, v["chain"], v["fan"], v["fan"], NONE])
        depth = u32([1, 2, 3, 1, 2, 1])
        want, wfr = truth.want(ids, depth)
        lo = u32([0, int(want[1][100]), 0, int(want[3][29]) + 1, int(want[4][1000]), 0])
        for limit in (1, 7, 100):
            DC.assert_pages(side, h, ids, depth, lo, ANY, limit, want, wfr)
        DC.assert_pages(side, h, ids, depth, None, ANY, 50, want, wfr)


def test_clean_slots(side, monkeypatch):
    """two slots, every request through tier 2: plain, depth, truncated depth, paged depth,
    combined and path calls on one handle, twice around.  A bitmap left dirty by a depth
    kernel's exit shows in the next answer."""
    monkeypatch.setenv(side.tier_env, "2")
    monkeypatch.setenv(side.slots_env, "2")
    snap, truth, v = DC.levels(side.name)
    ids = u32([v["w129"], v["fan"], v["chain"], v["cycle"], v["w65"]])
    depth = u32([1, 1, 3, 2, 2])
    want, wfr = truth.want(ids, depth)
    every = [truth.members(x, ALL) for x in ids]
    m = CC.Members(side, snap)
    with side.Handle(snap) as h:
        for _ in range(2):
            out, begin, count, needed = side.plain_raw(h, ids, ANY, sum(len(w) for w in every))
            assert all(np.array_equal(g, w) for g, w in zip(CC.split(out, begin, count), every))
            DC.assert_depth(side, h, ids, depth, ANY, want, wfr)
            cap = sum(len(w) for w in want) - 1  # the list that reserves last is truncated
            out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, cap)
            assert (begin == lookup.TRUNCATED).sum() == 1 and [int(f) for f in frontier] == wfr
            DC.assert_pages(side, h, ids, depth, None, ANY, 7, want, wfr)
            a, b = ids, ids[::-1].copy()
            for op in CC.OP_IDS:
                CC.assert_combined(h, a, b, op, ANY, m.want(a, b, op))
            if side.name == "lookup":
                roots = u32([int(w[-1]) for w in every])
                paths = h.path_ids(roots, ids)
                assert [len(p) - 1 for p in paths] == [side.hops(snap, int(t), int(r)) for r, t in zip(roots, ids)]
            DC.assert_depth(side, h, ids, depth, ANY, want, wfr)
        st = h.depth_stats()
        assert st["slots"] == 2 and st["tier1_requests"] == 0 and st["tier2_requests"] == st["requests"] == 8 * len(ids)
        assert st["tier2_rounds"] == 8 * 3


def test_writes_are_seen_by_the_next_call(side, tiers):
    """a write that adds a hop"""
    snap, x, add = DC.writable_chains(side)
    ks = [1, 2, 3, 4, 5, 6, ALL]
    with side.Handle(snap) as h:
        truth = DC.Truth(side, snap)
        before, bfr = side.lists(h, [x] * len(ks), ks)
        want, wfr = truth.want([x] * len(ks), ks)
        assert all(np.array_equal(g, w) for g, w in zip(before, want)) and [int(f) for f in bfr] == wfr
        assert [len(g) for g in before] == [1, 2, 3, 3, 3, 3, 3] and wfr == [1, 1, 0, 0, 0, 0, 0]
        assert snap.write(add)["applied"]
        truth = DC.Truth(side, snap)  # the host calls see the write
        after, afr = side.lists(h, [x] * len(ks), ks)
        want, wfr = truth.want([x] * len(ks), ks)
        assert all(np.array_equal(g, w) for g, w in zip(after, want)) and [int(f) for f in afr] == wfr
        assert [len(g) for g in after] == [1, 2, 4, 5, 6, 6, 6] and wfr == [1, 1, 1, 1, 0, 0, 0]


def check_workload(side, tiers, snap, filt):
    """2000 random starts (forced tier 2: 300) at k = 1, 2 and 3 against the host twins"""
    twin = DC.Twin(side, snap)
    rng = np.random.default_rng(7)
    starts = rng.integers(0, side.sample_bound(snap), 300 if tiers == "tier2" else 2000).astype(np.uint32)
    with side.Handle(snap) as h:
        sizes = {}
        for k in (1, 2, 3):
            depth = u32(np.full(len(starts), k))
            want, wfr = twin.want(starts, depth)
            unlisted = sum(not side.has_row(snap, int(x)) for x in starts)
            assert_tiers(h, tiers, twin, starts, depth,
                         lambda: DC.assert_depth(side, h, starts, depth, ANY, want, wfr), unlisted)
            sizes[k] = sum(len(w) for w in want)
            typed, _ = twin.want(starts, depth, filt)
            DC.assert_depth(side, h, starts, depth, filt, typed, wfr)
            assert sum(len(w) for w in typed) <= sizes[k]
        assert 0 < sizes[1] <= sizes[2] <= sizes[3] and sizes[1] < sizes[3]
        mixed = u32(rng.integers(0, 4, len(starts)))  # 0 .. 3 in one call: no limit next to limits
        want, wfr = twin.want(starts, mixed)
        DC.assert_depth(side, h, starts, mixed, ANY, want, wfr)
        DC.assert_pages(side, h, starts[:200], mixed[:200], None, ANY, 10, want[:200], wfr[:200])
        return h.depth_stats()
