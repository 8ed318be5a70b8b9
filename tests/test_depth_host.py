"""Depth-limited listings on the host (ketogpu_snapshot_lookup_depth / _subjects_depth and the
CPU twins HostLookup / HostSubjects), pinned against the yardstick of depth_cases.py: the plain
host list restricted by one shortest-path call per member.  Random tables (wildcard subject sets
and page poisoning included) and the level cases, in both directions; no GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from tests import depth_cases as DC
from tests import lookup_cases as LC
from tests import subjects_cases as SC

ANY, NONE, ALL = DC.ANY, DC.NONE, DC.ALL
SIDE_NAMES = list(DC.SIDES)


def starts(side, snap, step=1):
    return range(0, side.sample_bound(snap), step)


@pytest.mark.parametrize("side_name", SIDE_NAMES)
@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_twins_match_the_yardstick_on_random_tables(case, side_name):
    side = DC.SIDES[side_name]
    snap, truth = DC.table_truth(side_name, case)
    cut = deepest = 0
    for x in starts(side, snap):
        plain = side.host(snap, x, ANY)
        ecc = truth.eccentricity(x)
        deepest = max(deepest, ecc)
        prev, grown_after_zero = np.zeros(0, dtype=np.uint32), False
        complete_at = None
        for k in DC.DEPTHS:
            ids, fr = side.host_depth(snap, x, k, ANY)
            assert np.array_equal(ids, truth.members(x, k)), (x, k)
            assert fr == truth.frontier(x, k), (x, k)
            if k == ALL:
                assert np.array_equal(ids, plain) and fr == 0  # unlimited: the plain host list
                continue
            assert np.isin(prev, ids).all() and len(ids) >= len(prev)  # monotone in k
            if complete_at is not None:  # M_k stops growing once the frontier read 0 ...
                grown_after_zero |= len(ids) != len(prev)
            elif fr == 0:
                complete_at = k
                assert np.array_equal(ids, plain), (x, k)  # ... and is then the whole closure
            else:
                cut += 1
                assert k < ecc or len(ids) == len(plain)
            prev = ids
        assert not grown_after_zero, x
    print(f"{side_name} seed{case[0]}: deepest member at {deepest} hops, {cut} cut requests")
    assert deepest >= 3 and cut > 0  # the tables are not vacuous


@pytest.mark.parametrize("side_name", SIDE_NAMES)
@pytest.mark.parametrize("case", LC.TABLES[:2], ids=lambda c: f"seed{c[0]}")
def test_filters_restrict_the_any_list(case, side_name):
    side = DC.SIDES[side_name]
    snap, truth = DC.table_truth(side_name, case)
    filters = sorted({int(f) for x in starts(side, snap, 7) for f in
                      ([snap.node_info(int(u))["type"] for u in side.host(snap, x, ANY)[:3]]
                       if side_name == "lookup" else [lookup.CLASS_SUBJECT_ID])})
    assert filters
    for x in starts(side, snap, 3):
        for f in filters[:3]:
            for k in (1, 2, ALL):
                ids, fr = side.host_depth(snap, x, k, f)
                assert np.array_equal(ids, truth.members(x, k, f)), (x, k, f)
                assert fr == truth.frontier(x, k)  # the frontier does not depend on the filter


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_unlimited_depth_ties_to_the_oracle(case):
    """a member at no limit <=> the check is allowed (the matrix of test_subjects_host.py)"""
    _, _, snap = LC.table(*case)
    want = SC.oracle_matrix(case)
    n, nx = want.shape
    for t in range(n):
        ids, fr = lookup.host_lookup_depth(snap, t, ALL)
        got = np.zeros(nx, dtype=bool)
        got[ids] = True
        assert fr == 0 and (got == want[t]).all(), t
    for r in range(nx):
        ids, fr = lookup.host_subjects_depth(snap, r, ALL)
        got = np.zeros(n, dtype=bool)
        got[ids] = True
        assert fr == 0 and (got == want[:, r]).all(), r


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_level_cases_on_the_host(side_name):
    side = DC.SIDES[side_name]
    snap, truth, v = DC.levels(side_name)
    for name, x in v.items():
        ecc = truth.eccentricity(x)
        for k in list(range(1, ecc + 2)) + [ALL]:
            ids, fr = side.host_depth(snap, x, k, ANY)
            assert np.array_equal(ids, truth.members(x, k)) and fr == truth.frontier(x, k), (name, k)
    chain = v["chain"]
    assert [len(truth.members(chain, k)) for k in range(1, 8)] == [1, 2, 3, 4, 5, 6, 6]
    assert [truth.frontier(chain, k) for k in range(1, 8)] == [1, 1, 1, 1, 1, 0, 0]
    cyc = v["cycle"]  # the start is a member only through a cycle of at most k hops
    assert cyc not in truth.members(cyc, 2) and cyc in truth.members(cyc, 3)
    assert truth.frontier(cyc, 3) == 1 and truth.frontier(cyc, 4) == 0
    assert [len(truth.members(v[s], 1)) for s in ("w65", "w129", "s1024", "s1025", "fan")] == [65, 129, 1024, 1025, 30]
    assert len(truth.members(v["fan"], 2)) == 1050
    leaf = v["leaf_level"]  # a last level of members without a row: nothing was left unread
    assert truth.eccentricity(leaf) == 2 and truth.frontier(leaf, 1) == 1 and truth.frontier(leaf, 2) == 0


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_structure_cases_on_the_host(side_name):
    side = DC.SIDES[side_name]
    snap, twin, truth, v = DC.structure(side_name)
    x = v["self"]  # a self-loop: the start is its own member at one hop
    assert x in truth.members(x, 1) and x in twin.members(x, 1)
    d = v["diamond"]  # a node reachable in 2 and in 3 hops belongs to level 2
    for k in (1, 2, 3, ALL):
        assert np.array_equal(twin.members(d, k), truth.members(d, k)) and twin.frontier(d, k) == truth.frontier(d, k)
    assert len(truth.members(d, ALL)) == v["diamond_size"]
    chain, size = v["chain"], v["chain_size"]
    for k in (1, size - 1, size, size + 1, ALL):
        assert np.array_equal(twin.members(chain, k), truth.members(chain, k)), k
        assert twin.frontier(chain, k) == truth.frontier(chain, k), k
        assert len(twin.members(chain, k)) == (size if k == ALL else min(k, size))


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_writable_snapshot_placeholders_are_no_frontier(side_name):
    """a writable snapshot pads its rows with placeholder nodes: interior ids, but members of no
    list, so the frontier does not count them; and a write that adds hops is seen"""
    side = DC.SIDES[side_name]
    snap, x, add = DC.writable_chains(side)
    g = snap.graph()
    placeholders = [v for v in range(g["Ni"]) if snap.subject_class(v) == lookup.TYPE_NONE]
    assert placeholders and any(v in g["rev_col"] for v in placeholders)
    ks = [1, 2, 3, 4, 5, 6, ALL]
    for written in (False, True):
        truth = DC.Truth(side, snap)
        for v in starts(side, snap):
            for k in ks:
                ids, fr = side.host_depth(snap, v, k, ANY)
                assert np.array_equal(ids, truth.members(v, k)) and fr == truth.frontier(v, k), (written, v, k)
        sizes = [len(truth.members(x, k)) for k in ks]
        assert sizes == ([1, 2, 4, 5, 6, 6, 6] if written else [1, 2, 3, 3, 3, 3, 3])
        if not written:
            assert snap.write(add)["applied"]


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_classification_and_errors(side_name):
    side = DC.SIDES[side_name]
    snap, truth, v = DC.levels(side_name)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    ids, fr = side.host_depth(snap, NONE, 2, ANY)
    assert len(ids) == 0 and fr == 0
    if side_name == "subjects":  # a never-expanded root: the empty list
        assert nx < n
        ids, fr = side.host_depth(snap, n - 1, 2, ANY)
        assert len(ids) == 0 and fr == 0
    with pytest.raises(L.KetoError) as e:
        side.host_depth(snap, n + 5, 2, ANY)
    assert e.value.code == L.EINVAL


@pytest.mark.parametrize("side_name", SIDE_NAMES)
def test_cpu_twin_handles(side_name):
    """HostLookup / HostSubjects: the cursor layout, the re-issue loop, the pages and the named
    calls over the host twins"""
    side = DC.SIDES[side_name]
    snap, truth, v = DC.levels(side_name)
    h = side.Host(snap)
    n = snap.stats()["num_nodes"]
    x = v["chain"]
    ids = np.array([x, x, x, NONE, n + 5, v["w65"]], dtype=np.uint32)
    depth = np.array([1, 2, ALL, 2, 2, 1], dtype=np.uint32)
    valid = [0, 1, 2, 3, 5]
    want, wfr = truth.want(ids[valid], depth[valid])
    total = sum(len(w) for w in want)
    out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, total)
    assert needed == total and begin[4] == lookup.INVALID and count[4] == 0 and frontier[4] == 0
    got = DC.split(out, begin, count)
    for k, w, f in zip(valid, want, wfr):
        assert np.array_equal(got[k], w) and frontier[k] == f, k
    out, begin, count, frontier, needed = side.raw(h, ids, depth, ANY, 3)  # a capacity that truncates
    assert needed == total and (begin == lookup.TRUNCATED).any() and [int(c) for c in count[valid]] == \
        [len(w) for w in want]
    _, _, count, frontier, needed = side.raw(h, ids[valid], None, ANY, 0)  # null depths: no limit, count only
    assert needed == sum(len(truth.members(y, ALL)) for y in ids[valid]) and not frontier.any()
    lists, frontier = side.lists(h, ids[valid], depth[valid])
    for g, w, f, wf in zip(lists, want, frontier, wfr):
        assert np.array_equal(g, w) and f == wf
    with pytest.raises(L.KetoError):
        side.lists(h, ids, depth)  # an id outside the snapshot
    with pytest.raises(L.KetoError):
        side.lists(h, ids[valid], [1, 2])  # one depth per request
    with pytest.raises(L.KetoError):
        side.lists(h, ids[valid], -1)
    # pages: walking a depth-limited list to its end concatenates to the sorted M_k
    w65 = v["w65"]
    for k in (1, 2, ALL):
        for limit in (1, 7, 100):
            got, calls = DC.walk_pages(side, h, w65, k, ANY, limit)
            assert np.array_equal(got, truth.members(w65, k)), (k, limit)
            assert calls == max(1, -(-len(got) // limit))
    DC.assert_pages(side, h, ids[valid], depth[valid], None, ANY, 7, want, wfr)
    _, returned, count, remaining, frontier = side.page(h, ids, depth, None, ANY, 7)
    assert returned[4] == lookup.PAGE_INVALID and not count[4] and not remaining[4] and not frontier[4]


def test_named_calls_on_the_cpu_twins():
    snap, truth, v = DC.levels("lookup")
    h = lookup.HostLookup(snap)
    uk = lookup.SubjectID("uk")
    lists, complete = h.list_objects_depth_batch("n", "member", [uk, uk, uk], [1, 6, ALL])
    assert lists == [["k0"], [f"k{i}" for i in range(6)], [f"k{i}" for i in range(6)]]
    assert complete == [False, True, True]
    items, tok, total, done = h.list_objects_page("n", "member", uk, 2, "", max_depth=3)
    assert items == ["k0", "k1"] and tok != "" and total == 3 and done is False
    items, tok, total = h.list_objects_page("n", "member", uk, 100, "")  # without a depth: as before
    assert len(items) == 6 and tok == "" and total == 6
    snap, truth, v = DC.levels("subjects")
    h = lookup.HostSubjects(snap)
    root = ("n", "k5", "member")
    lists, complete = h.list_subjects_depth_batch([root, root, root], [5, 6, ALL])
    assert lists == [[], [lookup.SubjectID("uk")], [lookup.SubjectID("uk")]] and complete == [False, True, True]
    lists, complete = h.list_subjects_depth_batch([root], 2, "any")
    assert [s.object for s in lists[0]] == ["k3", "k4"] and complete == [False]
    items, tok, total, done = h.list_subjects_page(*root, "any", 100, "", max_depth=6)
    assert total == 6 and tok == "" and done is True
