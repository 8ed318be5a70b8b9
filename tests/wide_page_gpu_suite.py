"""The checks of the wide paged and depth calls (ketogpu_*_page_wide / ketogpu_*_ids_depth_wide,
keto_amd/csrc/wide.hpp "depth", "page"), shared by test_wide_page_subjects_gpu.py and
test_wide_page_lookup_gpu.py.  Built on wide_gpu_suite.py's `Side`.

Two yardsticks, every field compared with both: the host (HostSubjects / HostLookup, which
test_depth_host.py and test_paged_lists_host.py pin against the oracle) and the plain device call
ketogpu_*_page_depth / ketogpu_*_ids_depth on the same handle.  Pages: out[:returned], returned,
count, remaining, frontier.  Full lists: the sorted lists, begin's markers, count, frontier, needed.

Routing is that of the depth calls: by default tier 1 answers what fits its LDS set and the wide
tier the rest; KETOGPU_<SIDE>_TIER=2 ("forced") sends every request that has a row to the wide tier."""
import ctypes as C
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import wide_gpu_suite as W

ANY, NONE_F = lookup.TYPE_ANY, lookup.TYPE_NONE
ALL = lookup.DEPTH_ALL
INVALID_PAGE = lookup.PAGE_INVALID


class PSide:
    """wide_gpu_suite's Side with the paged and depth calls of one handle and of its host twin"""

    def __init__(self, side, host, page, depth, plain_page, chain, diamond, member_row, member_name):
        self.__dict__.update(side.__dict__)
        self.side = side
        self.host_twin, self._page, self._depth, self._plain_page = host, page, depth, plain_page
        self.chain, self.diamond, self.member_row, self.member_name = chain, diamond, member_row, member_name

    def force(self, monkeypatch, slots=None):
        self.side.force(monkeypatch, slots)

    def page(self, h, ids, depth=None, lo=None, f=ANY, limit=100, wide=True):
        return getattr(h, self._page)(ids, depth, lo, f, limit, wide=wide)

    def ids_depth(self, h, ids, depth=None, f=ANY, cap=0, wide=True):
        return getattr(h, self._depth)(ids, depth, f, cap, wide=wide)

    def plain_page(self, h, ids, lo=None, f=ANY, limit=100, wide=False):
        return getattr(h, self._plain_page)(ids, lo, f, limit, wide=wide)


SUBJECTS = PSide(
    W.SUBJECTS, lookup.HostSubjects, "subject_depth_page_raw", "subject_depth_raw", "subject_page_raw",
    chain=("c2999", 3000), diamond=("top", 2, 1),  # (start, the k at which two rows reach one node, its frontier)
    member_row=lambda start, member: LC.sid(start, "view", member),
    member_name=lambda snap, v: snap.describe(int(v)).id)
SUBJECTS.chain_start = lambda snap: int(lookup.resolve_roots(snap, [("n", "c2999", "member")])[0])

LOOKUP = PSide(
    W.LOOKUP, lookup.HostLookup, "lookup_depth_page_raw", "lookup_depth_raw", "lookup_page_raw",
    chain=("uc", 3000), diamond=("ux", 3, None),  # (top#view is reached from g1 and g2 at level 3)
    member_row=lambda start, member: LC.sid(member, "view", start),
    member_name=lambda snap, v: snap.node_info(int(v))["id"])
LOOKUP.chain_start = lambda snap: W.LOOKUP.start(snap, "uc")

SIDES = {"subjects": SUBJECTS, "lookup": LOOKUP}


# ---------------------------------------------------------------------- the host's answers
def depth_key(depth):
    return None if depth is None else tuple(int(d) for d in depth)


_HOST = {}


def host_lists(S, snap, ids, f, depth):
    """(ascending lists, None for an id outside the snapshot; frontier) by the host twin, once
    per (snapshot, ids, filter, limits)"""
    key = (S.name, id(snap), tuple(int(x) for x in ids), int(f), depth_key(depth))
    if key not in _HOST:
        d = None if depth is None else np.asarray(depth, dtype=np.uint32)
        _HOST[key] = (snap, S.host_twin(snap)._depth_all(np.asarray(ids, dtype=np.uint32), d, f))
    return _HOST[key][1]


def host_page(S, snap, ids, depth, lo, f, limit):
    """what HostSubjects / HostLookup *_depth_page_raw answer (the lists are shared between limits)"""
    lists, frontier = host_lists(S, snap, ids, f, depth)
    return lookup._host_pages(lists, [m is None for m in lists], lo, limit) + (frontier,)


def assert_page_equal(got, want, what):
    out, returned, count, remaining, frontier = got
    wout, wret, wcount, wrem, wfr = want
    assert np.array_equal(returned, wret), (what, "returned")
    assert np.array_equal(count, wcount), (what, "count")
    assert np.array_equal(remaining, wrem), (what, "remaining")
    assert np.array_equal(frontier, wfr), (what, "frontier")
    for i, k in enumerate(returned):
        if k != INVALID_PAGE:
            assert np.array_equal(out[i, :int(k)], wout[i, :int(k)]), (what, "out", i)


def check_page(S, h, snap, ids, depth=None, lo=None, f=ANY, limit=100, what=""):
    """one wide page call against the host and against the plain depth page call -> the answer"""
    ids = np.asarray(ids, dtype=np.uint32)
    got = S.page(h, ids, depth, lo, f, limit, wide=True)
    assert_page_equal(got, host_page(S, snap, ids, depth, lo, f, limit), (what, "host"))
    assert_page_equal(got, S.page(h, ids, depth, lo, f, limit, wide=False), (what, "plain"))
    return got


def check_lists(S, h, snap, ids, depth=None, f=ANY, what=""):
    """one wide full-list depth call with exactly the capacity it needs, and one that only counts,
    against the host and the plain depth call -> the host's lists"""
    ids = np.asarray(ids, dtype=np.uint32)
    want, wfr = host_lists(S, snap, ids, f, depth)
    total = sum(len(w) for w in want if w is not None)
    for wide in (True, False):
        out, begin, count, frontier, needed = S.ids_depth(h, ids, depth, f, total, wide=wide)
        assert needed == total, (what, wide)
        assert np.array_equal(frontier, wfr), (what, wide, "frontier")
        assert [int(c) for c in count] == [0 if w is None else len(w) for w in want], (what, wide, "count")
        assert [b == lookup.INVALID for b in begin] == [w is None for w in want], (what, wide)
        assert not (begin == lookup.TRUNCATED).any()
        for k, (g, w) in enumerate(zip(W.split(out, begin, count), want)):
            if w is not None:
                assert np.array_equal(g, w), (what, wide, k, int(ids[k]))
        out, begin, count, frontier, needed = S.ids_depth(h, ids, depth, f, 0, wide=wide)  # count only
        assert needed == total and np.array_equal(frontier, wfr), (what, wide, "count only")
        assert [int(c) for c in count] == [0 if w is None else len(w) for w in want]
        assert all(b == lookup.TRUNCATED for b, w in zip(begin, want) if w is not None and len(w))
    return want


def other_stats_do_not_move(S, h, ids, depth, lo, f, limit):
    """the new calls count in wide_stats() only (uploads and the wall time aside): stats() and
    depth_stats() stand still under a wide page, a wide list and a wide count-only call"""
    before = {"stats": h.stats(), "depth": h.depth_stats()}
    wide = h.wide_stats()
    got = S.page(h, ids, depth, lo, f, limit, wide=True)
    needed = S.ids_depth(h, ids, depth, f, 0, wide=True)[4]
    assert S.ids_depth(h, ids, depth, f, needed, wide=True)[4] == needed
    after = {"stats": h.stats(), "depth": h.depth_stats()}
    for name in after:
        for k in after[name]:
            if k not in ("uploads", "last_call_ms"):
                assert after[name][k] == before[name][k], (name, k)
    now = h.wide_stats()
    assert now["requests"] - wide["requests"] == 3 * len(ids)
    returned = int(got[1][got[1] != INVALID_PAGE].sum())
    assert now["ids_produced"] - wide["ids_produced"] == returned + 2 * needed


def mid_from(lists, n_nodes):
    """a lower bound in the middle of each list (an empty list: some id)"""
    return np.array([int(m[len(m) // 2]) if m is not None and len(m) else n_nodes // 2 for m in lists],
                    dtype=np.uint32)


# ---------------------------------------------------------------------- truth tables
def check_truth_table(S, case, forced, monkeypatch):
    if forced:
        S.force(monkeypatch)
    _, _, snap = LC.table(*case)
    st = snap.stats()
    n, n_nodes = S.starts(st), st["num_nodes"]
    ids = np.arange(n, dtype=np.uint32)
    mix = (np.arange(n) % 4).astype(np.uint32)  # ALL, 1, 2, 3, ...
    past = np.where(np.arange(n) % 2 == 0, n_nodes, 0xFFFFFFFF).astype(np.uint32)
    with S.handle(snap) as h:
        calls = returned_sum = listed = 0
        for f in (ANY, S.second_filter(snap), NONE_F):
            for depth in (None, 1, 2, 3, mix):
                d = None if depth is None else np.broadcast_to(np.uint32(depth), (n,)) if np.ndim(depth) == 0 else depth
                lists, _ = host_lists(S, snap, ids, f, d)
                for lo in (None, mid_from(lists, n_nodes), past):
                    for limit in (1, 7, 4096):
                        got = check_page(S, h, snap, ids, d, lo, f, limit, (case[0], f, depth_key(d), limit))
                        calls += 1
                        returned_sum += int(got[1].sum())
                        if lo is past:
                            assert not got[1].any() and not got[3].any()
                        if f == NONE_F:
                            assert not got[2].any()
                want = check_lists(S, h, snap, ids, d, f, (case[0], f, depth_key(d)))
                calls += 2  # (the list and its count-only twin)
                listed += 2 * sum(len(w) for w in want)
        assert any(len(w) for w in host_lists(S, snap, ids, ANY, None)[0])
        ws = h.wide_stats()
        assert ws["requests"] == calls * n and ws["requests"] == ws["tier1_requests"] + ws["wide_requests"]
        assert ws["ids_produced"] == returned_sum + listed
        if forced:  # (every one of these ids can have a row)
            assert ws["wide_requests"] == calls * n and ws["wide_rounds"] >= calls and ws["levels"] >= calls
        else:  # the largest closure of the tables has 246 nodes
            assert ws["wide_requests"] == 0 and ws["wide_rounds"] == 0 and ws["levels"] == 0 and ws["items"] == 0
        other_stats_do_not_move(S, h, ids, mix, None, ANY, 7)


# ---------------------------------------------------------------------- structure
def structure(S):
    return W.structure(S.name)[0]


def check_chain_levels(S, monkeypatch):
    """level L is launch L: a limit of k hops costs exactly k level launches"""
    S.force(monkeypatch)
    snap = structure(S)
    r = np.array([S.chain_start(snap)], dtype=np.uint32)
    with S.handle(snap) as h:
        for k in (1, 2, 64, 2999):
            before = h.wide_stats()["levels"]
            got = check_page(S, h, snap, r, np.array([k], dtype=np.uint32), None, ANY, 4096, ("chain", k))
            # (check_page issues the wide call once)
            assert h.wide_stats()["levels"] - before == k, k
            assert got[2][0] == k and got[4][0] == 1  # k members within k hops, one interior node cut off
            before = h.wide_stats()["levels"]
            check_lists(S, h, snap, r, np.array([k], dtype=np.uint32), ANY, ("chain list", k))
            assert h.wide_stats()["levels"] - before == 2 * k, k  # (the list and its count-only twin)
        before = h.wide_stats()["levels"]
        W.assert_call_matches(S.side, h, r, ANY, S.host(snap, r))  # ketogpu_*_ids_wide
        full = h.wide_stats()["levels"] - before
        assert full >= 2999
        for depth in (None, np.array([ALL], dtype=np.uint32)):
            before = h.wide_stats()["levels"]
            got = check_page(S, h, snap, r, depth, None, ANY, 4096, ("chain", "unlimited"))
            assert h.wide_stats()["levels"] - before == full
            assert got[2][0] == S.chain[1] and got[4][0] == 0 and got[1][0] == S.chain[1]


def check_structure_cases(S, monkeypatch):
    """the 2-cycle, the self-loop, the diamond and the stars of 65 and 129, and every node of the
    graph as a start at 1, 2 and 3 hops"""
    S.force(monkeypatch)
    snap = structure(S)
    n = snap.stats()["num_nodes"]
    one = lambda k, m: np.full(m, k, dtype=np.uint32)
    with S.handle(snap) as h:
        cyc = S.cycle_starts(snap)  # ya, yb, self
        at1 = check_page(S, h, snap, cyc, one(1, 3), None, ANY, 100, "cycles at 1")
        at2 = check_page(S, h, snap, cyc, one(2, 3), None, ANY, 100, "cycles at 2")
        listed = lambda got, i: int(cyc[i]) in [int(v) for v in got[0][i, :int(got[1][i])]]
        assert not listed(at1, 0) and not listed(at1, 1) and listed(at1, 2)  # the self-loop: at one hop
        assert listed(at2, 0) and listed(at2, 1) and listed(at2, 2)          # the 2-cycle: at two
        name, k, front = S.diamond
        r = np.array([S.start(snap, name)], dtype=np.uint32)
        for kk in (1, 2, 3, 4):
            got = check_page(S, h, snap, r, one(kk, 1), None, ANY, 100, ("diamond", kk))
            check_lists(S, h, snap, r, one(kk, 1), ANY, ("diamond list", kk))
            if kk == k and front is not None:
                assert got[4][0] == front  # reached from two rows of one level, counted once
        stars = S.structure_starts(snap)[[2, 0]]  # 65 and 129 entries
        for depth in (None, one(1, 2)):
            for limit in (64, 65, 128, 129, 130):
                got = check_page(S, h, snap, stars, depth, None, ANY, limit, ("stars", limit))
                assert [int(c) for c in got[2]] == [65, 129]
            lists, _ = host_lists(S, snap, stars, ANY, depth)
            check_page(S, h, snap, stars, depth, mid_from(lists, n), ANY, 100, "stars from the middle")
            check_lists(S, h, snap, stars, depth, ANY, "stars")
        every = np.arange(n, dtype=np.uint32)
        for kk in (1, 2, 3):
            lists, _ = host_lists(S, snap, every, ANY, one(kk, n))
            check_page(S, h, snap, every, one(kk, n), None, ANY, 7, ("every node", kk))
            check_page(S, h, snap, every, one(kk, n), mid_from(lists, n), S.second_filter(snap), 2,
                       ("every node, filtered", kk))
            check_lists(S, h, snap, every, one(kk, n), ANY, ("every node", kk))
        ws = h.wide_stats()
        assert ws["wide_requests"] > 0 and ws["requests"] == ws["tier1_requests"] + ws["wide_requests"]


def check_mixed_round(S, monkeypatch):
    """one round holds limits of 1, 2 and none side by side: a slot whose limit is reached
    produces no more items, the others go on"""
    S.force(monkeypatch, 4)
    snap = structure(S)
    c = S.chain_start(snap)
    ids = np.array([c, c, c, int(S.structure_starts(snap)[0])], dtype=np.uint32)
    depth = np.array([1, 2, ALL, 1], dtype=np.uint32)
    with S.handle(snap) as h:
        before = h.wide_stats()
        got = check_page(S, h, snap, ids, depth, None, ANY, 4096, "mixed round")
        after = h.wide_stats()
        assert after["slots"] == 4 and after["wide_rounds"] - before["wide_rounds"] == 1
        assert after["wide_requests"] - before["wide_requests"] == 4
        assert [int(x) for x in got[2]] == [1, 2, S.chain[1], 129]
        assert [int(x) for x in got[4]] == [1, 1, 0, 0]
        assert after["levels"] - before["levels"] >= 2999  # the unlimited slot ran to its end
        check_lists(S, h, snap, ids, depth, ANY, "mixed round, lists")


def check_rounds(S, slots, monkeypatch):
    """more wide requests than slots, and one start twice in a call under different `from` and depth"""
    S.force(monkeypatch, slots)
    snap = structure(S)
    c, star = S.chain_start(snap), int(S.structure_starts(snap)[0])
    ids = np.array([star, c, star, c], dtype=np.uint32)
    depth = np.array([1, 5, ALL, 70], dtype=np.uint32)
    lists, _ = host_lists(S, snap, ids, ANY, depth)
    lo = np.array([0, int(lists[1][2]), int(lists[2][100]), int(lists[3][69]) + 1], dtype=np.uint32)
    with S.handle(snap) as h:
        for _ in range(2):  # (the second call finds every bitmap clean)
            before = h.wide_stats()
            got = check_page(S, h, snap, ids, depth, lo, ANY, 50, ("rounds", slots))
            after = h.wide_stats()
            assert after["slots"] == slots and after["wide_rounds"] - before["wide_rounds"] == 4 // slots
            assert [int(x) for x in got[1]] == [50, 3, 29, 0] and [int(x) for x in got[3]] == [129, 3, 29, 0]
        check_lists(S, h, snap, ids, depth, ANY, ("rounds, lists", slots))


# ---------------------------------------------------------------------- finish boundaries
@functools.lru_cache(maxsize=None)
def boundary_graph(side):
    """one start with 2T + 130 direct members, which the wide tier takes by its size, and one that
    holds every 1000th of them in id order, counted down from the largest: the third tile holds
    only the 130 largest members, so counting up from the smallest would leave it empty.
    T: the ids one workgroup of the clear kernel covers"""
    S = SIDES[side]
    T = int(L.lib().ketogpu_wide_clear_tile_ids())
    k = 2 * T + 130
    rows = S.star("big", k, "m")
    alone = Snapshot.from_rows(LC.NS1, rows)  # (ids follow the names: a further start keeps the members' order)
    picked = S.host(alone, [S.start(alone, "big")])[0][::-1][::1000]
    rows = rows + [S.member_row("sparse", S.member_name(alone, v)) for v in picked]
    snap = Snapshot.from_rows(LC.NS1, rows)
    big, sparse = (np.array([S.start(snap, x)], dtype=np.uint32) for x in ("big", "sparse"))
    members = S.host(snap, big)[0]
    few = S.host(snap, sparse)[0]
    assert len(members) == k and len(few) == -(-k // 1000)
    assert members[0] < T and members[-1] >= 2 * T and few[0] < T and few[-1] >= 2 * T  # three tiles each
    return T, snap, big, sparse, members, few


def boundary_froms(T, ms):
    """`from` at a member, one below it and one above it, next to a 32-id word boundary, each
    tile boundary, the smallest member and the largest member + 1"""
    places = [32 * 100, T, 2 * T, int(ms[0]), int(ms[-1]) + 1]
    los = set()
    for p in places:
        j = int(np.searchsorted(ms, p))
        near = [p] + ([int(ms[j])] if j < len(ms) else []) + ([int(ms[j - 1])] if j else [])
        for m in near:
            los.update(x for x in (m - 1, m, m + 1) if 0 <= x <= 0xFFFFFFFF)
    return np.array(sorted(los), dtype=np.uint32)


def check_boundaries_big(S):
    """unforced: the start's size alone routes it to the wide tier"""
    T, snap, big, sparse, ms, few = boundary_graph(S.name)
    with S.handle(snap) as h:
        lo = boundary_froms(T, ms)
        before = h.wide_stats()
        got = check_page(S, h, snap, np.repeat(big, len(lo)), None, lo, ANY, 7, "from at the boundaries")
        after = h.wide_stats()
        assert after["wide_requests"] - before["wide_requests"] == len(lo)
        assert after["ids_produced"] - before["ids_produced"] == int(got[1].sum())
        assert (got[2] == len(ms)).all()
        j = int(np.searchsorted(ms, T)) - 1  # the last member of tile 0
        cases = [(int(ms[j - 99]), 100, int(ms[j - 99]), int(ms[j])),          # ends on the last member of a tile
                 (int(ms[j + 1]), 100, int(ms[j + 1]), int(ms[j + 100])),       # starts on the first of the next
                 (int(ms[j - 10]), T + 100, int(ms[j - 10]), int(ms[j - 10 + T + 99])),  # spans three tiles
                 (int(ms[-1]), 1, int(ms[-1]), int(ms[-1]))]
        assert T + 100 <= lookup.PAGE_LIMIT_MAX and ms[j] < T <= ms[j + 1] and ms[j - 10 + T + 99] >= 2 * T
        for lo1, limit, first, last in cases:
            got = check_page(S, h, snap, big, None, np.array([lo1], dtype=np.uint32), ANY, limit, ("page", lo1, limit))
            k = int(got[1][0])
            assert k == limit and got[0][0, 0] == first and got[0][0, k - 1] == last
        check_page(S, h, snap, big, np.array([1], dtype=np.uint32), np.array([T], dtype=np.uint32),
                   S.view_filter(snap), 300, "one hop, filtered, from the tile boundary")
        check_lists(S, h, snap, big, np.array([1], dtype=np.uint32), ANY, "the big list")
        other_stats_do_not_move(S, h, np.concatenate([big, sparse]), None, np.array([T, 0], dtype=np.uint32), ANY, 50)


def check_boundaries_sparse(S, monkeypatch):
    S.force(monkeypatch)
    T, snap, big, sparse, ms, few = boundary_graph(S.name)
    with S.handle(snap) as h:
        lo = boundary_froms(T, few)
        check_page(S, h, snap, np.repeat(sparse, len(lo)), None, lo, ANY, 3, "sparse, from at the boundaries")
        check_page(S, h, snap, sparse, None, None, ANY, 64, "sparse, the first page of 64")
        token = np.array([int(few[len(few) - 64])], dtype=np.uint32)  # the page of 64 that ends at the largest member
        got = check_page(S, h, snap, sparse, None, token, ANY, 64, "sparse, a page of 64 over every tile")
        page = got[0][0, :int(got[1][0])]
        assert len(page) == 64 and page[0] < T and ((page >= T) & (page < 2 * T)).any() and page[-1] >= 2 * T
        walked, token = [], 0
        for _ in range(len(few)):  # the whole list by tokens
            got = S.page(h, sparse, None, np.array([token], dtype=np.uint32), ANY, 7)
            k = int(got[1][0])
            walked += [int(v) for v in got[0][0, :k]]
            if got[3][0] == k:
                break
            token = walked[-1] + 1
        assert walked == [int(v) for v in few]
        both = np.concatenate([big, sparse, big])
        check_page(S, h, snap, both, None, np.array([T - 1, 2 * T, 2 * T + 1], dtype=np.uint32), ANY, 33,
                   "big and sparse in one round")


# ---------------------------------------------------------------------- bitmaps are left zero
def check_bitmaps_left_zero(S, monkeypatch):
    """tier 2 and both wide finishes share the slots' bitmaps: each finds them all zero behind the
    others, also behind a page shorter than its list and behind a truncated full-list call"""
    S.force(monkeypatch)
    snap = structure(S)
    r = S.structure_starts(snap)
    w = S.host(snap, r)
    two = np.full(len(r), 2, dtype=np.uint32)

    def every_call(h):
        W.assert_call_matches(S.side, h, r, ANY, w, wide=False)            # plain ids
        check_page(S, h, snap, r, None, None, ANY, 4096, "wide page")       # wide page
        got = S.plain_page(h, r, None, ANY, 4096)                           # plain page
        assert_page_equal(got + (np.zeros(len(r), dtype=np.uint64),), host_page(S, snap, r, None, None, ANY, 4096),
                          "plain page")
        check_lists(S, h, snap, r, two, ANY, "wide depth list")            # wide depth list
        W.assert_call_matches(S.side, h, r, ANY, w, wide=True)             # wide ids

    with S.handle(snap) as h:
        every_call(h)
        check_page(S, h, snap, r, None, None, ANY, 1, "a page shorter than its list")
        every_call(h)
        want, _ = host_lists(S, snap, r, ANY, None)
        total = sum(len(x) for x in want)
        before = h.wide_stats()["truncated_lists"]
        out, begin, count, frontier, needed = S.ids_depth(h, r, None, ANY, total // 2)
        assert needed == total and (begin == lookup.TRUNCATED).any()
        assert h.wide_stats()["truncated_lists"] > before
        for g, x in zip(W.split(out, begin, count), want):
            assert g is None or np.array_equal(g, x)  # a list that was written is complete
        out, begin, count, frontier, needed = S.ids_depth(h, r, None, ANY, needed)  # the re-issue
        assert not (begin == lookup.TRUNCATED).any()
        assert all(np.array_equal(g, x) for g, x in zip(W.split(out, begin, count), want))
        every_call(h)
        before = h.wide_stats()["truncated_lists"]
        check_page(S, h, snap, r, None, None, ANY, 1, "pages truncate nothing")
        assert h.wide_stats()["truncated_lists"] == before


# ---------------------------------------------------------------------- contracts
def check_contracts(S, forced, monkeypatch):
    """limit 0, limit > MAX and null arrays: EINVAL; n = 0; ids outside the snapshot, NODE_NONE,
    starts without a row; frontier NULL and from NULL"""
    if forced:
        S.force(monkeypatch)
    snap = structure(S)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    abi = L.lib()
    page = getattr(abi, f"ketogpu_{S.name}_page_wide")
    ids_depth = getattr(abi, f"ketogpu_{S.name}_ids_depth_wide")
    with S.handle(snap) as h:
        for limit in (0, lookup.PAGE_LIMIT_MAX + 1):
            try:
                S.page(h, np.array([5], dtype=np.uint32), None, None, ANY, limit)
                raise AssertionError(f"limit {limit} was accepted")
            except L.KetoError as e:
                assert e.code == L.EINVAL
        one = np.array([5], dtype=np.uint32)
        buf32, buf64 = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        p32, p64 = buf32.ctypes.data, buf64.ctypes.data
        needed = C.c_uint64()
        assert page(h.h, None, None, None, 1, ANY, 4, p32, p32, p64, p64, None) == L.EINVAL
        assert page(h.h, one.ctypes.data, None, None, 1, ANY, 4, None, p32, p64, p64, None) == L.EINVAL
        assert page(h.h, one.ctypes.data, None, None, 1, ANY, 4, p32, None, p64, p64, None) == L.EINVAL
        assert page(h.h, one.ctypes.data, None, None, 1, ANY, 4, p32, p32, None, p64, None) == L.EINVAL
        assert page(h.h, one.ctypes.data, None, None, 1, ANY, 4, p32, p32, p64, None, None) == L.EINVAL
        assert page(None, one.ctypes.data, None, None, 1, ANY, 4, p32, p32, p64, p64, None) == L.EINVAL
        assert ids_depth(h.h, None, None, 1, ANY, None, 0, p64, p64, None, C.byref(needed)) == L.EINVAL
        assert ids_depth(h.h, one.ctypes.data, None, 1, ANY, None, 0, None, p64, None, C.byref(needed)) == L.EINVAL
        assert ids_depth(h.h, one.ctypes.data, None, 1, ANY, None, 0, p64, p64, None, None) == L.EINVAL
        assert ids_depth(h.h, one.ctypes.data, None, 1, ANY, None, 4, p64, p64, None, C.byref(needed)) == L.EINVAL
        # n = 0: OK, with every array null
        assert page(h.h, None, None, None, 0, ANY, 4, None, None, None, None, None) == L.OK
        assert ids_depth(h.h, None, None, 0, ANY, None, 0, None, None, None, C.byref(needed)) == L.OK
        assert needed.value == 0
        got = S.page(h, np.zeros(0, dtype=np.uint32), None, None, ANY, 4)
        assert len(got[1]) == 0
        # frontier NULL and from NULL, max_depth given: the other fields as with them
        r = np.array([S.chain_start(snap)], dtype=np.uint32)
        two = np.array([2], dtype=np.uint32)
        out, ret, cnt, rem = (np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64),
                              np.zeros(1, dtype=np.uint64))
        assert page(h.h, r.ctypes.data, two.ctypes.data, None, 1, ANY, 4, out.ctypes.data, ret.ctypes.data,
                    cnt.ctypes.data, rem.ctypes.data, None) == L.OK
        want = host_page(S, snap, r, two, None, ANY, 4)
        assert ret[0] == want[1][0] == 2 and cnt[0] == 2 and rem[0] == 2 and np.array_equal(out[:2], want[0][0, :2])
        b, c = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        assert ids_depth(h.h, r.ctypes.data, two.ctypes.data, 1, ANY, out.ctypes.data, 4, b.ctypes.data, c.ctypes.data,
                         None, C.byref(needed)) == L.OK
        assert needed.value == 2 and c[0] == 2 and b[0] == 0 and np.array_equal(np.sort(out[:2]), want[0][0, :2])
        # ids outside the snapshot, NODE_NONE, starts without a row
        ids = np.array([7, L.NODE_NONE, n, 9, 0xFFFFFFFE, n - 1, nx, nx - 1], dtype=np.uint32)
        valid = (0, 3, 5, 6, 7)
        for depth in (None, np.full(len(ids), 2, dtype=np.uint32)):
            before = h.wide_stats()
            got = check_page(S, h, snap, ids, depth, None, ANY, 9, "starts")
            assert got[1][2] == INVALID_PAGE and got[1][4] == INVALID_PAGE and got[1][1] == 0 and got[2][1] == 0
            after = h.wide_stats()
            assert after["requests"] - before["requests"] == len(ids)
            assert (after["tier1_requests"] - before["tier1_requests"]) + (after["wide_requests"]
                                                                           - before["wide_requests"]) == len(valid)
            if forced:
                rowed = sum(1 for k in valid if int(ids[k]) < S.starts(st))
                assert after["wide_requests"] - before["wide_requests"] == rowed
            want = check_lists(S, h, snap, ids, depth, ANY, "starts, lists")
            assert want[2] is None and want[4] is None and want[1] is not None and not len(want[1])


# ---------------------------------------------------------------------- writes
def check_writes(S, monkeypatch):
    """an in-place write adds a member below a page's first id: the next wide page call lists it
    first, and a page from the old first id on is what it was, with one more in `count`"""
    S.force(monkeypatch)
    rows = S.star("pa", 50, "a_") + S.star("pb", 50, "b_") + S.star("bulk", 3000, "f_")
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    a, b = S.start(snap, "pa"), S.start(snap, "pb")
    ma, mb = S.host(snap, [a])[0], S.host(snap, [b])[0]
    # the start whose members lie above the other's smallest gains that one
    start, name, new = (a, "pa", int(mb[0])) if mb[0] < ma[0] else (b, "pb", int(ma[0]))
    r = np.array([start], dtype=np.uint32)
    with S.handle(snap) as h:
        first = check_page(S, h, snap, r, None, None, ANY, 10, "before the write")
        p0 = int(first[0][0, 0])
        assert new < p0 and first[2][0] == 50
        from_p0 = check_page(S, h, snap, r, None, np.array([p0], dtype=np.uint32), ANY, 10, "from p0, before")
        assert snap.write([S.member_row(name, S.member_name(snap, new))])["applied"]
        _HOST.clear()  # (the host's lists are cached per snapshot object)
        got = check_page(S, h, snap, r, None, None, ANY, 10, "after the write")
        assert got[0][0, 0] == new and got[0][0, 1] == p0 and got[2][0] == 51 and got[3][0] == 51
        again = check_page(S, h, snap, r, None, np.array([p0], dtype=np.uint32), ANY, 10, "from p0, after")
        assert np.array_equal(again[0][0, :10], from_p0[0][0, :10])
        assert again[2][0] == 51 and again[3][0] == from_p0[3][0] == 50
        one = check_page(S, h, snap, r, np.array([1], dtype=np.uint32), None, ANY, 100, "one hop, after")
        assert one[1][0] == 51
        assert h.stats()["uploads"] == 2 and h.wide_stats()["wide_requests"] > 0
