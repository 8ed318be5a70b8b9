"""The device tests of the listings that say why, written once for both handles:
test_via_lookup_gpu.py and test_via_subjects_gpu.py import every test here and supply the fixture
`side` (via_cases.LookupSide / SubjectsSide).  The yardstick is via_cases.Checker over
depth_cases.Truth: hops and member sets exactly, every (via, member) edge by host_path, and under
ANY a complete tree.  via values are never compared with the host twins'."""
import ctypes as C

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from tests import combine_cases as CC
from tests import depth_cases as DC
from tests import lookup_cases as LC
from tests import via_cases as VC

ANY, NONE, ALL = VC.ANY, VC.NONE, VC.ALL
SENTINEL = 0xABCD1234


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
    """call() moves the via stats by the tiers the depth rule predicts (forced tier 2: all listed
    requests), and the plain, depth, combine (and path) stats not at all"""
    others = lambda: [h.stats(), h.depth_stats(), h.combine_stats()] + \
        ([h.path_stats()] if hasattr(h, "path_stats") else [])
    before = others()
    t1, t2 = DC.depth_tiers(truth, ids, depth, before[0]["set_capacity"])
    got = VC.tier_delta(h, call)
    listed = len(ids) - unlisted
    assert got == ((0, listed) if tiers == "tier2" else (t1 - unlisted, t2)), (got, t1, t2, unlisted)
    assert others() == before  # via calls count in their own struct


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables_on_the_device(case, side, tiers):
    snap, truth = DC.table_truth(side.name, case)
    chk = VC.Checker(side, snap, truth)
    starts = np.arange(side.sample_bound(snap), dtype=np.uint32)
    ids, depth = np.repeat(starts, len(DC.DEPTHS)), u32(np.tile(DC.DEPTHS, len(starts)))
    with side.Handle(snap) as h:
        lists = []
        assert_tiers(h, tiers, truth, ids, depth, lambda: lists.extend(VC.assert_via(side, h, chk, ids, depth)))
        # the member sets of the depth call on the same handle, word for word
        total = sum(len(m[0]) for m in lists)
        out, begin, count, frontier, needed = side.depth_raw(h, ids, depth, ANY, total)
        assert needed == total
        assert all(np.array_equal(g, m[0]) for g, m in zip(DC.split(out, begin, count), lists))
        st = h.via_stats()
        assert st["requests"] == len(ids) and st["ids_produced"] == total and st["truncated_lists"] == 0
        assert st["cut_requests"] > 0
        VC.assert_via(side, h, chk, starts, None)  # a null depth array is no limit for every request


def test_level_boundaries_and_the_cycle(side, tiers):
    """the chain of 6; start rows of 65 and 129 entries (a level ends inside and at the end of a
    64-entry step); a level whose last row adds nothing; the cycle of 3; a last level without
    rows"""
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    names = ["chain", "w65", "w129", "empty_last", "cycle", "leaf_level"]
    ids, depth = [], []
    for name in names:
        ks = list(range(1, truth.eccentricity(v[name]) + 2)) + [ALL]
        ids += [v[name]] * len(ks)
        depth += ks
    ids, depth = u32(ids), u32(depth)
    with side.Handle(snap) as h:
        assert_tiers(h, tiers, truth, ids, depth, lambda: VC.assert_via(side, h, chk, ids, depth))
        cyc = v["cycle"]  # the start is its own member at the cycle's length, and the via of level 1
        (m, via, hops), = side.lists(h, [cyc], [ALL])[0]
        at = int(np.searchsorted(m, cyc))
        assert m[at] == cyc and hops[at] == 3 and via[at] != cyc and hops[m == via[at]] == 2
        assert (hops == 1).sum() == 1 and (via[hops == 1] == cyc).all()
        assert cyc not in side.lists(h, [cyc], [2])[0][0][0]
        for name in ("w65", "w129"):
            (m, via, hops), = side.lists(h, [v[name]], [2])[0]
            k = int(name[1:])
            assert (hops == 1).sum() == (hops == 2).sum() == k and (via[hops == 1] == v[name]).all()
            assert np.array_equal(np.sort(via[hops == 2]), m[hops == 1])  # one document or user per group


def test_structure(side, tiers):
    """the diamond (either parent), the self-loop, and the 3000-chain through tier 2"""
    snap, _, truth, v = DC.structure(side.name)
    chk = VC.Checker(side, snap, truth)
    with side.Handle(snap) as h:
        x, d = v["self"], v["diamond"]
        lists = VC.assert_via(side, h, chk, [x, d, d, d, d], [1, 1, 2, 3, ALL])
        m, via, hops = lists[0]
        at = int(np.searchsorted(m, x))
        assert m[at] == x and via[at] == x and hops[at] == 1
        assert len(lists[2][0]) == 3 and len(lists[4][0]) == 4
        check_chain(side, h, chk, v)
        st = h.via_stats()
        assert st["tier2_requests"] == (5 + 5 if tiers == "tier2" else 4)  # default: k = 1 stays in LDS
        if side.list_cap_env is None:
            assert st["list_finishes"] == st["scan_finishes"] == 0
        else:
            assert st["list_finishes"] == st["tier2_requests"] and st["scan_finishes"] == 0


def check_chain(side, h, chk, v):
    """the 3000-chain at no limit, at k = 2999 and at k = 1: hops run 1 .. and via is the previous link"""
    chain, size = v["chain"], v["chain_size"]
    lists = VC.assert_via(side, h, chk, [chain, chain, chain], [ALL, size - 1, 1], chains=8, edges=32)
    for (m, via, hops), n in zip(lists, (size, size - 1, 1)):
        assert len(m) == n
        order = np.argsort(hops)
        assert np.array_equal(hops[order], np.arange(1, n + 1))
        assert via[order[0]] == chain and np.array_equal(via[order[1:]], m[order[:-1]])
    out, via, hops, returned, count, remaining, fr = side.page(h, [chain, chain], [ALL, size - 1], u32([2000, 0]),
                                                               ANY, 100)
    for k, (m, mv, mh) in enumerate(lists[:2]):
        rest = np.searchsorted(m, [2000, 0][k])
        r = int(returned[k])
        assert r == min(100, len(m) - rest) and np.array_equal(out[k, :r], m[rest:rest + r])
        assert np.array_equal(via[k, :r], mv[rest:rest + r]) and np.array_equal(hops[k, :r], mh[rest:rest + r])
    assert [int(f) for f in fr] == [0, 1]


def test_tier_rule(side):
    """a request goes to tier 2 exactly when its unfiltered M_k passes the set capacity"""
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    with side.Handle(snap) as h:
        def one(name, k):
            x = u32([v[name]])
            lists = []
            got = VC.tier_delta(h, lambda: lists.extend(VC.assert_via(side, h, chk, x, u32([k]), chains=64,
                                                                      edges=64)))
            assert got == DC.depth_tiers(truth, x, [k], h.stats()["set_capacity"])
            return got, lists[0]

        got, (m, via, hops) = one("s1024", 1)
        assert got == (1, 0) and len(m) == 1024 and (via == v["s1024"]).all() and (hops == 1).all()
        got, (m, via, hops) = one("s1025", 1)
        assert got == (0, 1) and len(m) == 1025 and (via == v["s1025"]).all() and (hops == 1).all()
        assert one("s1024", ALL)[0] == (1, 0)
        got, (m, via, hops) = one("fan", 1)  # the near part stays in LDS, every via the start
        assert got == (1, 0) and len(m) == 30 and (via == v["fan"]).all()
        groups = m
        got, (m, via, hops) = one("fan", 2)  # the closure of 1050 leaves it, via in the 30 groups
        assert got == (0, 1) and len(m) == 1050
        assert np.array_equal(np.unique(via[hops == 2]), groups) and (hops == 2).sum() == 1020
        assert one("fan", ALL)[0] == (0, 1)
        st = h.via_stats()
        assert st["slots"] >= 1 and h.stats()["tier1_requests"] == h.stats()["tier2_requests"] == 0


def test_concrete_filter(side, tiers):
    """hops equal the yardstick and via is valid against the ANY yardstick although the via node
    is not listed"""
    snap, truth = DC.table_truth(side.name, LC.TABLES[0])
    chk = VC.Checker(side, snap, truth)
    starts = np.arange(0, side.sample_bound(snap), 2, dtype=np.uint32)
    if side.name == "subjects":
        filters = [lookup.CLASS_SUBJECT_ID]
    else:
        filters = sorted({int(snap.node_info(int(u))["type"]) for x in starts[::5] for u in
                          side.host(snap, int(x), ANY)[:3]})[:2]
    unlisted = 0
    with side.Handle(snap) as h:
        for f in filters:
            assert f not in (ANY, lookup.TYPE_NONE)
            for k in (1, 2, ALL):
                lists = VC.assert_via(side, h, chk, starts, u32(np.full(len(starts), k)), f)
                unlisted += sum(int((~np.isin(via, m) & (via != x)).sum()) for x, (m, via, _) in zip(starts, lists))
    assert unlisted > 0


def raw_call(side, h, ids, depth, filt, cap, out, via, hops):
    """the cursor call over caller-owned arrays (None: NULL)"""
    ids, depth = u32(ids), u32(depth)
    n = len(ids)
    begin, count, frontier = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    needed = C.c_uint64()
    ptr = lambda a: None if a is None else a.ctypes.data
    L.check(h._abi("ids_via")(h.h, ids.ctypes.data, depth.ctypes.data, n, int(filt), ptr(out), ptr(via), ptr(hops),
                              cap, begin.ctypes.data, count.ctypes.data, frontier.ctypes.data, C.byref(needed)))
    return begin, count, frontier, needed.value


def test_truncation_protocol_count_only_and_null_arrays(side, tiers):
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    ids = u32([v["w129"], v["chain"], v["w65"], v["w129"], v["fan"]])
    depth = u32([1, 4, 2, ALL, 2])
    want, wfr = truth.want(ids, depth)
    sizes = [len(w) for w in want]
    total = sum(sizes)
    with side.Handle(snap) as h:
        begin, count, frontier, needed = raw_call(side, h, ids, depth, ANY, 0, None, None, None)  # counts only
        assert needed == total and [int(c) for c in count] == sizes and (begin == lookup.TRUNCATED).all()
        assert [int(f) for f in frontier] == wfr
        cap = total - 1  # whichever list reserves last does not fit, every other one does
        arrays = [np.full(total + 8, SENTINEL, dtype=np.uint32) for _ in range(3)]
        before = h.via_stats()["truncated_lists"]
        begin, count, frontier, needed = raw_call(side, h, ids, depth, ANY, cap, *arrays)
        assert needed == total and [int(c) for c in count] == sizes and [int(f) for f in frontier] == wfr
        trunc = begin == lookup.TRUNCATED
        assert trunc.sum() == 1 and h.via_stats()["truncated_lists"] - before == 1
        written = np.zeros(total + 8, dtype=bool)
        for k in np.nonzero(~trunc)[0]:  # a list is written completely or marked
            b = int(begin[k])
            assert b + sizes[k] <= cap
            written[b:b + sizes[k]] = True
            order = np.argsort(arrays[0][b:b + sizes[k]], kind="stable")
            chk.answer(ids[k], depth[k], ANY, *[a[b:b + sizes[k]][order] for a in arrays], chains=32, edges=32)
        for a in arrays:  # every word outside the written lists keeps the sentinel, in all three arrays
            assert (a[~written] == SENTINEL).all() and (a[written] != SENTINEL).all()
        for drop in (1, 2):  # via NULL, hops NULL, each on its own
            arrays = [np.full(total, SENTINEL, dtype=np.uint32) for _ in range(3)]
            given = [None if j == drop else a for j, a in enumerate(arrays)]
            begin, count, frontier, needed = raw_call(side, h, ids, depth, ANY, total, *given)
            assert needed == total and not (begin == lookup.TRUNCATED).any()
            assert (arrays[drop] == SENTINEL).all() and (arrays[3 - drop] != SENTINEL).all()
            for k in range(len(ids)):
                b = int(begin[k])
                order = np.argsort(arrays[0][b:b + sizes[k]], kind="stable")
                assert np.array_equal(arrays[0][b:b + sizes[k]][order], want[k])
                if drop == 1:  # the hops that came alone are the yardstick's
                    every, dist = truth.dist(ids[k])
                    assert np.array_equal(arrays[2][b:b + sizes[k]][order], dist[np.searchsorted(every, want[k])])
        out = side.raw(h, ids, depth, ANY, total, want_via=False)  # ... and through the Python call
        assert out[1] is None and out[2] is not None
        lists, fr = side.lists(h, ids, depth, capacity=1)  # the re-issue loop ends with every list
        chk.batch(ids, depth, ANY, lists, fr, chains=32, edges=32)


def test_pages(side, tiers):
    """walking to the end reproduces the full answer's (id, hops) pairs, with valid via values"""
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    with side.Handle(snap) as h:
        for name, k in (("w129", 1), ("w129", 2), ("chain", ALL), ("cycle", ALL)):
            x = v[name]
            (m, _, hops), = side.lists(h, [x], [k])[0]
            for limit in (1, 7, 100):
                if limit == 1 and len(m) > 129:
                    continue  # (258 one-id calls show nothing that 129 do not)
                pids, pvia, phops, calls = VC.walk_pages(side, h, x, k, ANY, limit)
                assert np.array_equal(pids, m) and np.array_equal(phops, hops), (name, k, limit)
                chk.answer(x, k, ANY, pids, pvia, phops)
                assert calls == -(-len(m) // limit)
        ids = u32([v["w129"], v["w129"], v["chain"], v["fan"], v["fan"], NONE])
        depth = u32([1, 2, 3, 1, 2, 1])
        want, wfr = truth.want(ids, depth)
        lo = u32([0, int(want[1][100]), 0, int(want[3][29]) + 1, int(want[4][1000]), 0])
        full, _ = side.lists(h, ids, depth)
        for limit in (1, 7, 100):
            for frm in (lo, None):
                out, via, hops, returned, count, remaining, fr = side.page(h, ids, depth, frm, ANY, limit)
                assert [int(f) for f in fr] == wfr
                for k, (m, mv, mh) in enumerate(full):
                    rest = int(np.searchsorted(m, 0 if frm is None else frm[k]))
                    r = int(returned[k])
                    assert int(count[k]) == len(m) and int(remaining[k]) == len(m) - rest
                    assert r == min(limit, len(m) - rest) and np.array_equal(out[k, :r], m[rest:rest + r])
                    assert np.array_equal(hops[k, :r], mh[rest:rest + r])
                    for j in range(0, r, 13):
                        assert chk.edge(via[k, j], out[k, j])


def test_clean_slots(side, monkeypatch):
    """two slots, every request through tier 2: plain, depth, path (lookup), combined and via
    calls on one handle, twice around.  A stale parent or hop word of the slot's previous request
    shows up as a wrong answer."""
    monkeypatch.setenv(side.tier_env, "2")
    monkeypatch.setenv(side.slots_env, "2")
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    ids = u32([v["w129"], v["fan"], v["chain"], v["cycle"], v["w65"]])
    other = ids[::-1].copy()  # the same slots serve other requests in between
    depth = u32([1, 2, 3, ALL, 2])
    want, wfr = truth.want(ids, depth)
    every = [truth.members(x, ALL) for x in ids]
    m = CC.Members(side, snap)
    with side.Handle(snap) as h:
        for _ in range(2):
            out, begin, count, needed = side.plain_raw(h, ids, ANY, sum(len(w) for w in every))
            assert all(np.array_equal(g, w) for g, w in zip(CC.split(out, begin, count), every))
            VC.assert_via(side, h, chk, ids, depth, chains=32, edges=32)
            DC.assert_depth(DC.SIDES[side.name], h, ids, depth, ANY, want, wfr)
            VC.assert_via(side, h, chk, other, depth, chains=32, edges=32)
            if side.name == "lookup":
                roots = u32([int(w[-1]) for w in every])
                paths = h.path_ids(roots, ids)
                assert [len(p) - 1 for p in paths] == [side.hops(snap, int(t), int(r)) for r, t in zip(roots, ids)]
            for op in CC.OP_IDS:
                CC.assert_combined(h, ids, other, op, ANY, m.want(ids, other, op))
            VC.assert_via(side, h, chk, ids, depth, chains=32, edges=32)
            out, via, hops, returned, count, remaining, fr = side.page(h, ids, depth, None, ANY, 7)
            for k, w in enumerate(want):
                assert np.array_equal(out[k, :int(returned[k])], w[:7])
                every_k, dist = truth.dist(ids[k])
                assert np.array_equal(hops[k, :int(returned[k])], dist[np.searchsorted(every_k, w[:7])])
        st = h.via_stats()
        assert st["slots"] == 2 and st["tier1_requests"] == 0 and st["tier2_requests"] == st["requests"] == 8 * len(ids)
        assert st["tier2_rounds"] == 8 * 3


def test_mixed_batch(side, tiers):
    """NONE, an id outside the snapshot and a node without a row next to valid ids; an empty
    batch; the plain calls' argument checks"""
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    n = snap.stats()["num_nodes"]
    x = v["w65"]
    ids = u32([x, NONE, x, n - 1, x, n + 5, v["chain"]])
    depth = u32([1, 1, 2, 2, ALL, 1, 3])
    valid = [0, 1, 2, 3, 4, 6]
    want, wfr = truth.want(ids[valid], depth[valid])
    total = sum(len(w) for w in want)
    with side.Handle(snap) as h:
        before = h.via_stats()
        out, via, hops, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, total)
        assert needed == total and begin[5] == lookup.INVALID and count[5] == 0 and frontier[5] == 0
        assert begin[1] == 0 and count[1] == 0 and frontier[1] == 0
        lists = VC.split3(out, via, hops, begin, count)
        chk.batch(ids[valid], depth[valid], ANY, [lists[k] for k in valid], frontier[valid])
        after = h.via_stats()
        assert after["tier1_requests"] + after["tier2_requests"] - before["tier1_requests"] \
            - before["tier2_requests"] == len(ids) - 2  # NONE and INVALID belong to neither tier
        _, _, _, returned, cnt, rem, fr = side.page(h, ids, depth, None, ANY, 7)
        assert returned[5] == lookup.PAGE_INVALID and not cnt[5] and not rem[5] and not fr[5]
        assert [int(c) for c in cnt[valid]] == [len(w) for w in want] and [int(f) for f in fr[valid]] == wfr
        with pytest.raises(L.KetoError) as e:
            side.lists(h, ids, depth)
        assert e.value.code == L.EINVAL
        out, via, hops, begin, count, frontier, needed = side.raw(h, u32([]), u32([]), ANY, 0)
        assert needed == 0 and len(begin) == 0
        for limit in (0, lookup.PAGE_LIMIT_MAX + 1):
            with pytest.raises(L.KetoError):
                side.page(h, ids, depth, None, ANY, limit)
        begin = np.empty(len(ids), dtype=np.uint64)
        assert h._abi("ids_via")(h.h, ids.ctypes.data, None, len(ids), ANY, None, None, None, 4, begin.ctypes.data,
                                 begin.ctypes.data, None, C.byref(C.c_uint64())) == L.EINVAL  # capacity without out
        assert h._abi("ids_via")(h.h, ids.ctypes.data, None, len(ids), ANY, None, None, None, 0, begin.ctypes.data,
                                 begin.ctypes.data, None, None) == L.EINVAL  # needed is required


def test_writes_are_seen_by_the_next_call(side, tiers):
    """after the write the next call's hops and via follow the new chain"""
    snap, x, add = DC.writable_chains(DC.SIDES[side.name])
    with side.Handle(snap) as h:
        chk = VC.Checker(side, snap, DC.Truth(side, snap))
        (m, via, hops), = VC.assert_via(side, h, chk, [x], [ALL])
        assert sorted(hops) == [1, 2, 3]
        assert snap.write(add)["applied"]
        chk = VC.Checker(side, snap, DC.Truth(side, snap))  # the host calls see the write
        (m, via, hops), = VC.assert_via(side, h, chk, [x], [ALL])
        assert sorted(hops) == [1, 2, 3, 3, 4, 5]  # the second chain hangs under the first
        (m, via, hops), = VC.assert_via(side, h, chk, [x], [4])
        assert sorted(hops) == [1, 2, 3, 3, 4]


def check_workload(side, tiers, snap, filt):
    """2000 random starts (forced tier 2: 300) at k = 1, 2, 3 and mixed: hops and member sets
    exactly against the host twins, the edge check on a fixed-seed sample of 500 members per k"""
    rng = np.random.default_rng(7)
    starts = rng.integers(0, side.sample_bound(snap), 300 if tiers == "tier2" else 2000).astype(np.uint32)
    pick = np.random.default_rng(11)
    twins = {}

    def twin(x, k, f):
        if (x, k, f) not in twins:
            twins[x, k, f] = (np.zeros(0, dtype=np.uint32),) * 3 + (0,) if x == NONE else side.host_via(snap, x, k, f)
        return twins[x, k, f]

    def check(depth, f, sample):
        want = [twin(int(x), int(k), f) for x, k in zip(starts, depth)]
        total = sum(len(w[0]) for w in want)
        out, via, hops, begin, count, frontier, needed = side.raw(h, starts, depth, f, total)
        assert needed == total and not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
        assert [int(fr) for fr in frontier] == [int(w[3]) for w in want]
        lists = VC.split3(out, via, hops, begin, count)
        for (m, _, hp), w in zip(lists, want):
            assert np.array_equal(m, w[0]) and np.array_equal(hp, w[2])
        if sample and total:
            where = np.repeat(np.arange(len(starts)), [len(m[0]) for m in lists])
            flat = [np.concatenate([m[j] for m in lists]) for j in range(3)]
            for j in pick.choice(total, min(sample, total), replace=False):
                u, w, hp = (int(a[j]) for a in flat)
                assert side.edge(snap, w, u), (int(starts[where[j]]), u, w)
                assert (w == int(starts[where[j]])) == (hp == 1)
        return total

    with side.Handle(snap) as h:
        sizes = {}
        for k in (1, 2, 3):
            depth = u32(np.full(len(starts), k))
            sizes[k] = check(depth, ANY, 500)
            assert check(depth, filt, 100) <= sizes[k]
        assert 0 < sizes[1] <= sizes[2] <= sizes[3] and sizes[1] < sizes[3]
        check(u32(rng.integers(0, 4, len(starts))), ANY, 500)  # 0 .. 3 in one call: no limit next to limits
        return h.via_stats()
