"""The checks shared by the via tests (test_via_host.py on the CPU, via_gpu_suite.py on the
device).  Next to depth_cases.py, whose graphs and yardstick they use.

The yardstick is older code only: `hops` must equal depth_cases.Truth.dist (the plain host list
with one host_path call per member), the member sets and the frontier Truth.want, and an edge is
checked with host_path: (via, u) on the subjects side and (u, via) on the lookup side must be a
path of exactly 2 nodes.  `via` values are never compared between two implementations, only
against the definition in include/ketogpu.h."""
import numpy as np

from keto_amd import lookup
from tests import combine_cases as CC
from tests import depth_cases as DC

ANY, NONE, ALL = DC.ANY, DC.NONE, DC.ALL


class LookupSide(DC.LookupSide):
    host_via = staticmethod(lookup.host_lookup_via)
    depth_raw = staticmethod(DC.LookupSide.raw)

    @staticmethod
    def edge(snap, via, u):  # via is an entry of row(u): u holds via
        return len(lookup.host_path(snap, int(u), int(via))) == 2

    @staticmethod
    def raw(h, ids, depth, filt, cap, **want):
        return h.lookup_via_raw(ids, depth, filt, cap, **want)

    @staticmethod
    def page(h, ids, depth, lo, filt, limit):
        return h.lookup_via_page_raw(ids, depth, lo, filt, limit)

    @staticmethod
    def lists(h, ids, depth, filt=ANY, capacity=None):
        return h.lookup_via(ids, depth, filt, capacity)


class SubjectsSide(DC.SubjectsSide):
    host_via = staticmethod(lookup.host_subjects_via)
    depth_raw = staticmethod(DC.SubjectsSide.raw)

    @staticmethod
    def edge(snap, via, u):  # u is an entry of row(via): via holds u
        return len(lookup.host_path(snap, int(via), int(u))) == 2

    @staticmethod
    def raw(h, ids, depth, filt, cap, **want):
        return h.subject_via_raw(ids, depth, filt, cap, **want)

    @staticmethod
    def page(h, ids, depth, lo, filt, limit):
        return h.subject_via_page_raw(ids, depth, lo, filt, limit)

    @staticmethod
    def lists(h, ids, depth, filt=ANY, capacity=None):
        return h.subject_via(ids, depth, filt, capacity)


SIDES = {"lookup": LookupSide, "subjects": SubjectsSide}


class Checker:
    """the definition of include/ketogpu.h "listings that say why" over one snapshot and side,
    against a depth_cases.Truth; edges are checked once per (via, member) pair"""

    def __init__(self, side, snap, truth):
        self.side, self.snap, self.truth, self.edges = side, snap, truth, {}

    def edge(self, via, u):
        key = (int(via), int(u))
        if key not in self.edges:
            self.edges[key] = self.side.edge(self.snap, *key)
        return self.edges[key]

    def answer(self, x, k, filt, ids, via, hops, chains=None, edges=None):
        """one request's (ids ascending, via, hops) against the definition.  chains / edges: how
        many members (evenly spread) get their grant_chain walked / their edge checked (None:
        all of them)"""
        x, k = int(x), int(k)
        ids, via, hops = np.asarray(ids), np.asarray(via), np.asarray(hops)
        assert np.array_equal(ids, self.truth.members(x, k, filt)), (x, k, filt, len(ids))
        every, dist = self.truth.dist(x)  # the ANY yardstick, whatever the filter
        at = np.searchsorted(every, ids)
        assert np.array_equal(hops, dist[at]), (x, k, filt)
        assert (hops >= 1).all() and (k == ALL or (hops <= k).all())
        near = hops == 1
        assert (via[near] == x).all(), (x, k)  # level 1 is the start's own row
        far = ~near
        # otherwise an interior member of the unfiltered closure, one hop nearer the start
        assert np.isin(via[far], every).all() and (via[far] < self.truth.ni).all(), (x, k)
        assert np.array_equal(dist[np.searchsorted(every, via[far])], hops[far] - 1), (x, k)
        pick = lambda n: range(len(ids)) if n is None or n >= len(ids) else \
            np.unique(np.linspace(0, len(ids) - 1, n).astype(int))
        for j in pick(edges):
            assert self.edge(via[j], ids[j]), (x, k, int(via[j]), int(ids[j]))
        if filt == ANY:  # a complete tree: every chain ends at the start after `hops` steps
            for j in pick(chains):
                chain = lookup.grant_chain(ids, via, x, ids[j])
                assert len(chain) == int(hops[j]) + 1 and chain[0] == ids[j] and chain[-1] == x, (x, k, int(ids[j]))

    def batch(self, ids, depth, filt, lists, frontier, **kw):
        depth = np.broadcast_to(np.asarray(ALL if depth is None else depth), (len(ids),))
        _, wfr = self.truth.want(ids, depth)
        assert [int(f) for f in frontier] == wfr, (depth[:8], ids[:8])
        for x, k, (m, v, h) in zip(ids, depth, lists):
            self.answer(x, k, filt, m, v, h, **kw)


def split3(out, via, hops, begin, count):
    """the lists of a cursor call, each sorted by id -> [(ids, via, hops)]"""
    res = []
    for b, c in zip(begin, count):
        b, c = int(b), int(c)
        order = np.argsort(out[b:b + c], kind="stable")
        res.append((out[b:b + c][order], via[b:b + c][order], hops[b:b + c][order]))
    return res


def assert_via(side, h, chk, ids, depth, filt=ANY, **kw):
    """one via cursor call with exactly the capacity needed: needed = the sum, counts exact,
    nothing TRUNCATED or INVALID, the segments tile [0, needed), and every list meets the
    definition -> the lists"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    want, _ = chk.truth.want(ids, ALL if depth is None else depth, filt)
    total = sum(len(w) for w in want)
    out, via, hops, begin, count, frontier, needed = side.raw(h, ids, depth, filt, total)
    assert needed == total, (needed, total)
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    used = np.zeros(total + 1, dtype=np.int32)
    for bg, c in zip(begin, count):
        used[int(bg):int(bg) + int(c)] += 1
    assert (used[:total] == 1).all()
    lists = split3(out, via, hops, begin, count)
    chk.batch(ids, depth, filt, lists, frontier, **kw)
    return lists


def walk_pages(side, h, x, k, filt, limit):
    """every page of one list, by the token rule -> (ids, via, hops concatenated, calls)"""
    got, lo, calls = [], 0, 0
    while True:
        out, via, hops, returned, count, remaining, _ = side.page(h, [x], [k], np.array([lo], dtype=np.uint32), filt,
                                                                  limit)
        calls += 1
        r = int(returned[0])
        got.append((out[0, :r].copy(), via[0, :r].copy(), hops[0, :r].copy()))
        tok = lookup.next_page_token(out[0], r, remaining[0])
        if tok == "":
            return tuple(np.concatenate([g[j] for g in got]) for j in range(3)) + (calls,)
        lo = lookup.parse_page_token(tok)


def tier_delta(h, call):
    before = h.via_stats()
    call()
    after = h.via_stats()
    return (after["tier1_requests"] - before["tier1_requests"], after["tier2_requests"] - before["tier2_requests"])


split = CC.split
