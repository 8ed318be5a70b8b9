"""Listings that say why, on the host (ketogpu_snapshot_lookup_via / _subjects_via, the CPU twins
HostLookup / HostSubjects and grant_chain), pinned against the yardstick of via_cases.py: hops
equal depth_cases.Truth.dist, member sets and frontier Truth.want, every (via, member) edge a
host_path of 2 nodes, and under ANY a complete tree.  Random tables, the level cases and the
structure graph, in both directions; no GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from tests import depth_cases as DC
from tests import lookup_cases as LC
from tests import via_cases as VC

ANY, NONE, ALL = VC.ANY, VC.NONE, VC.ALL
SIDE_NAMES = list(VC.SIDES)


@pytest.mark.parametrize("side_name", SIDE_NAMES)
@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_twins_match_the_yardstick_on_random_tables(case, side_name):
    side = VC.SIDES[side_name]
    snap, truth = DC.table_truth(side_name, case)
    chk = VC.Checker(side, snap, truth)
    deepest = 0
    for x in range(side.sample_bound(snap)):
        for k in DC.DEPTHS:
            ids, via, hops, fr = side.host_via(snap, x, k, ANY)
            assert fr == truth.frontier(x, k), (x, k)
            chk.answer(x, k, ANY, ids, via, hops)
            dids, dfr = side.host_depth(snap, x, k, ANY)  # the depth twin's set, word for word
            assert np.array_equal(ids, dids) and fr == dfr
            deepest = max(deepest, int(hops.max(initial=0)))
    assert deepest >= 3  # the tables are not vacuous


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_filters_keep_hops_and_name_unlisted_vias(side_name):
    side = VC.SIDES[side_name]
    snap, truth = DC.table_truth(side_name, LC.TABLES[0])
    chk = VC.Checker(side, snap, truth)
    unlisted = 0
    for x in range(0, side.sample_bound(snap), 3):
        every = side.host(snap, x, ANY)
        filters = {lookup.CLASS_SUBJECT_ID} if side_name == "subjects" else \
            {int(snap.node_info(int(u))["type"]) for u in every[:3]}
        for f in sorted(filters)[:3]:
            for k in (1, 2, ALL):
                ids, via, hops, fr = side.host_via(snap, x, k, f)
                assert fr == truth.frontier(x, k)  # the frontier does not depend on the filter
                chk.answer(x, k, f, ids, via, hops)
                unlisted += int((~np.isin(via, ids) & (via != x)).sum())
    assert unlisted > 0  # a via that is a node id whatever the filter says


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_level_cases_on_the_host(side_name):
    side = VC.SIDES[side_name]
    snap, truth, v = DC.levels(side_name)
    chk = VC.Checker(side, snap, truth)
    for name, x in v.items():
        big = name in ("s1024", "s1025", "fan")
        for k in list(range(1, truth.eccentricity(x) + 2)) + [ALL]:
            ids, via, hops, fr = side.host_via(snap, x, k, ANY)
            assert fr == truth.frontier(x, k), (name, k)
            chk.answer(x, k, ANY, ids, via, hops, chains=64 if big else None, edges=64 if big else None)
    cyc = v["cycle"]  # the start is its own member at the cycle's length, and the via of level 1
    ids, via, hops, _ = side.host_via(snap, cyc, ALL, ANY)
    at = int(np.searchsorted(ids, cyc))
    assert ids[at] == cyc and hops[at] == 3 and via[at] != cyc and hops[ids == via[at]] == 2
    assert (via[hops == 1] == cyc).all() and (hops == 1).sum() == 1
    assert lookup.grant_chain(ids, via, cyc, cyc)[0] == lookup.grant_chain(ids, via, cyc, cyc)[-1] == cyc
    ids, via, hops, _ = side.host_via(snap, v["fan"], 2, ANY)
    assert (hops == 1).sum() == 30 and set(via[hops == 2]) == set(ids[hops == 1])
    ids, via, hops, _ = side.host_via(snap, v["chain"], ALL, ANY)
    assert sorted(hops) == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_structure_cases_on_the_host(side_name):
    side = VC.SIDES[side_name]
    snap, _, truth, v = DC.structure(side_name)
    chk = VC.Checker(side, snap, truth)
    x = v["self"]
    ids, via, hops, _ = side.host_via(snap, x, ALL, ANY)
    at = int(np.searchsorted(ids, x))
    assert ids[at] == x and via[at] == x and hops[at] == 1  # a self-loop
    chk.answer(x, ALL, ANY, ids, via, hops)
    d = v["diamond"]
    for k in (1, 2, 3, ALL):
        chk.answer(d, k, ANY, *side.host_via(snap, d, k, ANY)[:3])  # either parent is accepted
    chain, size = v["chain"], v["chain_size"]
    ids, via, hops, fr = side.host_via(snap, chain, ALL, ANY)
    assert fr == 0 and sorted(hops) == list(range(1, size + 1))
    order = np.argsort(hops)
    assert via[order[0]] == chain and np.array_equal(via[order[1:]], ids[order[:-1]])  # the previous link
    chk.answer(chain, ALL, ANY, ids, via, hops, chains=16, edges=64)
    ids, via, hops, fr = side.host_via(snap, chain, 10, ANY)
    assert fr == 1 and sorted(hops) == list(range(1, 11))


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_host_handles_lay_their_results_out_like_the_device(side_name):
    side = VC.SIDES[side_name]
    snap, truth, v = DC.levels(side_name)
    chk = VC.Checker(side, snap, truth)
    h = side.Host(snap)
    n = snap.stats()["num_nodes"]
    ids = np.array([v["w65"], NONE, v["chain"], v["cycle"]], dtype=np.uint32)
    depth = np.array([2, 1, 3, ALL], dtype=np.uint32)
    lists = VC.assert_via(side, h, chk, ids, depth)
    assert [len(m[0]) for m in lists] == [130, 0, 3, 3]
    got, fr = side.lists(h, ids, depth, capacity=1)  # the re-issue loop
    chk.batch(ids, depth, ANY, got, fr)
    total = sum(len(m[0]) for m in lists)
    out, via, hops, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, total - 1)
    assert needed == total and (begin == lookup.TRUNCATED).sum() == 1
    out, via, hops, begin, count, frontier, needed = side.raw(h, np.array([n + 5], dtype=np.uint32), None, ANY, 8)
    assert begin[0] == lookup.INVALID and needed == 0
    with pytest.raises(L.KetoError):
        side.lists(h, [n + 5], None)
    for limit in (1, 7, 100):
        for x, k in ((v["w65"], 2), (v["chain"], ALL)):
            pids, pvia, phops, calls = VC.walk_pages(side, h, x, k, ANY, limit)
            chk.answer(x, k, ANY, pids, pvia, phops)
            assert calls == -(-len(pids) // limit)
    out, via, hops, returned, count, remaining, fr = side.page(h, [n + 5, NONE], None, None, ANY, 5)
    assert returned[0] == lookup.PAGE_INVALID and returned[1] == 0


def test_grant_chain():
    ids, via = np.array([3, 5, 9], dtype=np.uint32), np.array([7, 3, 5], dtype=np.uint32)
    assert lookup.grant_chain(ids, via, 7, 9) == [9, 5, 3, 7]
    assert lookup.grant_chain(ids, via, 7, 3) == [3, 7]
    with pytest.raises(KeyError):
        lookup.grant_chain(ids, via, 7, 4)  # no member
    with pytest.raises(KeyError):
        lookup.grant_chain(ids, np.array([8, 3, 5], dtype=np.uint32), 7, 9)  # a via that is not listed
    with pytest.raises(KeyError):
        lookup.grant_chain(ids, np.array([5, 3, 5], dtype=np.uint32), 7, 9)  # a loop that misses the start


def test_null_arrays_and_argument_checks():
    import ctypes as C
    snap, truth, v = DC.levels("lookup")
    lib = snap.L
    p, n = C.c_void_p(), C.c_uint64()
    L.check(lib.ketogpu_snapshot_lookup_via(snap.h, v["chain"], ANY, 2, C.byref(p), None, None, C.byref(n), None))
    assert n.value == 2
    lib.ketogpu_free(p)
    assert lib.ketogpu_snapshot_lookup_via(snap.h, v["chain"], ANY, 2, None, None, None, C.byref(n), None) == L.EINVAL
    with pytest.raises(L.KetoError):
        lookup.host_lookup_via(snap, snap.stats()["num_nodes"] + 1)
    with pytest.raises(L.KetoError):
        lookup.host_subjects_via(snap, snap.stats()["num_nodes"] + 1)
    ids, via, hops, fr = lookup.host_subjects_via(snap, NONE)
    assert len(ids) == len(via) == len(hops) == 0 and fr == 0


def test_named_calls_on_the_host():
    from keto_amd import relationtuple as rt
    snap, _, _ = DC.levels("lookup")
    uk = rt.SubjectID("uk")
    hl = lookup.HostLookup(snap)
    items, tok, total = hl.list_objects_page("n", "member", uk, 4, "", with_via=True)
    assert [(o, h) for o, _, h in items] == [("k0", 1), ("k1", 2), ("k2", 3), ("k3", 4)] and total == 6
    assert items[0][1] == uk and items[1][1] == rt.SubjectSet("n", "k0", "member")
    items, _, total, complete = hl.list_objects_page("n", "member", uk, 4, "", max_depth=2, with_via=True)
    assert [(o, h) for o, _, h in items] == [("k0", 1), ("k1", 2)] and total == 2 and complete is False
    assert hl.list_objects_page("n", "member", uk, 4, "") == (["k0", "k1", "k2", "k3"], tok, 6)  # unchanged
    assert hl.list_objects_via_batch("n", "member", [uk], 1) == [[("k0", uk, 1)]]
    snap, _, _ = DC.levels("subjects")
    hs = lookup.HostSubjects(snap)
    items, tok, total = hs.list_subjects_page("n", "k5", "member", "ids", 10, "", with_via=True)
    assert items == [(rt.SubjectID("uk"), rt.SubjectSet("n", "k0", "member"), 6)] and total == 1
    got = hs.list_subjects_via_batch([("n", "k5", "member")], "any", 2)
    assert got == [[(rt.SubjectSet("n", "k3", "member"), rt.SubjectSet("n", "k4", "member"), 2),
                    (rt.SubjectSet("n", "k4", "member"), rt.SubjectSet("n", "k5", "member"), 1)]]
