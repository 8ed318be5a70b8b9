"""The yardstick and the graphs shared by the depth tests (test_depth_host.py on the CPU,
test_depth_lookup_gpu.py / test_depth_subjects_gpu.py on the device).  Next to path_cases.py.

The yardstick is built from calls that are older than the depth calls and share no code with
them: the member set within k hops is

    { u in host_lookup / host_subjects : len(host_path(...)) - 1 <= k }

and the frontier is the number of those members at exactly k hops with an id below
num_interior.  `Truth` computes it per start node, once.  The host twins
(ketogpu_snapshot_*_depth) are pinned against it on the CPU; after that they serve as the
device's reference where one path call per member would take too long (`twin`)."""
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd.snapshot import Snapshot
from tests import combine_cases as CC
from tests import lookup_cases as LC
from tests import subjects_cases as SC

ANY, NONE, ALL = lookup.TYPE_ANY, L.NODE_NONE, lookup.DEPTH_ALL
DEPTHS = [1, 2, 3, 4, 5, 6, ALL]


class LookupSide(CC.LookupSide):
    host_depth = staticmethod(lookup.host_lookup_depth)
    list_cap_env = None

    @staticmethod
    def hops(snap, x, u):  # u reaches the target x
        return len(lookup.host_path(snap, u, x)) - 1

    @staticmethod
    def raw(h, ids, depth, filt, cap):
        return h.lookup_depth_raw(ids, depth, filt, cap)

    @staticmethod
    def page(h, ids, depth, lo, filt, limit):
        return h.lookup_depth_page_raw(ids, depth, lo, filt, limit)

    @staticmethod
    def lists(h, ids, depth, filt=ANY):
        return h.lookup_depth(ids, depth, filt)

    @staticmethod
    def set_node(snap, obj, rel="member"):
        return int(lookup.resolve_subjects(snap, [lookup.SubjectSet("n", obj, rel)])[0])

    @staticmethod
    def chain(prefix, n, user):
        """`user` is held by {prefix}0, which is held by {prefix}1, ...: from the user, group
        {prefix}{d-1} is d hops away -> rows"""
        return [LC.sid(f"{prefix}0", "member", user)] + \
            [LC.sset(f"{prefix}{i + 1}", "member", f"{prefix}{i}", "member") for i in range(n - 1)]

    @staticmethod
    def fan(name, mids, per):
        """user `name` is held by the groups `mids`, and every group by `per` documents of its
        own: level 1 is the groups, level 2 the documents"""
        return [LC.sid(m, "member", name) for m in mids] + \
            [LC.sset(f"{m}_d{i}", "view", m, "member") for m in mids for i in range(per)]


class SubjectsSide(CC.SubjectsSide):
    host_depth = staticmethod(lookup.host_subjects_depth)
    list_cap_env = "KETOGPU_SUBJECTS_LIST_CAP"

    @staticmethod
    def hops(snap, x, u):  # the root x reaches u
        return len(lookup.host_path(snap, x, u)) - 1

    @staticmethod
    def raw(h, ids, depth, filt, cap):
        return h.subject_depth_raw(ids, depth, filt, cap)

    @staticmethod
    def page(h, ids, depth, lo, filt, limit):
        return h.subject_depth_page_raw(ids, depth, lo, filt, limit)

    @staticmethod
    def lists(h, ids, depth, filt=ANY):
        return h.subject_depth(ids, depth, filt)

    @staticmethod
    def set_node(snap, obj, rel="member"):
        return int(lookup.resolve_roots(snap, [("n", obj, rel)])[0])

    @staticmethod
    def fan(name, mids, per):
        """document `name` is held by the groups `mids`, and every group holds `per` users of
        its own: level 1 is the groups, level 2 the users"""
        return [LC.sset(name, "view", m, "member") for m in mids] + \
            [LC.sid(m, "member", f"{m}_u{i}") for m in mids for i in range(per)]


SIDES = {"lookup": LookupSide, "subjects": SubjectsSide}


class Truth:
    """the yardstick of one snapshot and side: per start node x the hop distance of every member
    of the plain host list (under ANY), from one host_path call per member, memoized"""

    def __init__(self, side, snap):
        self.side, self.snap, self.memo = side, snap, {}
        # (the graph view, not the build-time statistics: a writable snapshot treats every
        # expandable node as interior)
        self.n, self.ni = snap.stats()["num_nodes"], int(snap.graph()["Ni"])

    def dist(self, x):
        """-> (members under ANY, ascending; their hop distances)"""
        x = int(x)
        if x not in self.memo:
            ids = np.zeros(0, dtype=np.uint32) if x == NONE else self.side.host(self.snap, x, ANY)
            d = np.array([self.side.hops(self.snap, x, int(u)) for u in ids], dtype=np.int64)
            assert (d >= 1).all()
            self.memo[x] = (ids, d)
        return self.memo[x]

    def members(self, x, k, filt=ANY):
        """M_k(x) under the filter, ascending"""
        ids, d = self.dist(x)
        near = ids if k == ALL else ids[d <= k]
        if filt == ANY:
            return near
        return np.intersect1d(near, self.side.host(self.snap, int(x), filt)).astype(np.uint32)

    def frontier(self, x, k):
        ids, d = self.dist(x)
        return 0 if k == ALL else int(((d == k) & (ids < self.ni)).sum())

    def eccentricity(self, x):
        """the largest distance of a member (0: no members)"""
        return int(self.dist(x)[1].max(initial=0))

    def want(self, ids, depth, filt=ANY):
        """-> (lists, frontier) of a batch, depth one number or one per request"""
        depth = np.broadcast_to(np.asarray(depth), (len(ids),))
        return ([self.members(x, int(k), filt) for x, k in zip(ids, depth)],
                [self.frontier(x, int(k)) for x, k in zip(ids, depth)])


class Twin:
    """Truth's interface over the host twins, for the workloads where one path call per member
    takes too long.  test_depth_host.py pins the twins against Truth."""

    def __init__(self, side, snap):
        self.side, self.snap, self.memo = side, snap, {}

    def _get(self, x, k, filt):
        key = (int(x), int(k), filt)
        if key not in self.memo:
            self.memo[key] = (np.zeros(0, dtype=np.uint32), 0) if key[0] == NONE else \
                self.side.host_depth(self.snap, key[0], key[1], filt)
        return self.memo[key]

    def members(self, x, k, filt=ANY):
        return self._get(x, k, filt)[0]

    def frontier(self, x, k):
        return int(self._get(x, k, ANY)[1])

    def want(self, ids, depth, filt=ANY):
        depth = np.broadcast_to(np.asarray(depth), (len(ids),))
        return ([self.members(x, int(k), filt) for x, k in zip(ids, depth)],
                [self.frontier(x, int(k)) for x, k in zip(ids, depth)])


@functools.lru_cache(maxsize=None)
def table_truth(side_name, case):
    """one of lookup_cases.TABLES -> (snapshot, Truth); every start node's distances are computed
    on first use and shared"""
    _, _, snap = LC.table(*case)
    return snap, Truth(SIDES[side_name], snap)


# ---- the level cases: one snapshot per side with a part per mechanism (names do not overlap)
def level_rows(side):
    """a chain of 6; start rows of 65 and 129 entries; a level whose last row adds nothing (its
    entries were all seen in the row before: the worklist tail stands still where the level
    ends); a cycle of 3 back to the start; stars of 1024 and 1025; a star of 30 over a closure
    of 30 + 30 x 34 = 1050; a last level of members without a row of their own.  For the lookup
    side a start is a user and levels climb through the groups and documents that hold it; for
    the subjects side a start is a document and levels descend to the subjects it is held by."""
    s, ss = LC.sid, LC.sset
    ids = lambda p, k: [f"{p}{i}" for i in range(k)]
    rows = []
    # ed#view holds ea and eb, both hold ec only, ec holds ef, ef holds the user ue.  From ed
    # level 1 is {ea, eb} and whichever row is read last adds nothing; from ue the same holds for
    # level 3
    empty_last = [ss("ed", "view", "ea", "member"), ss("ed", "view", "eb", "member"), ss("ea", "member", "ec", "member"),
                  ss("eb", "member", "ec", "member"), ss("ec", "member", "ef", "member"), s("ef", "member", "ue")]
    if side is LookupSide:
        rows += side.chain("k", 6, "uk")  # uk <- k0 <- k1 ... <- k5
        # 65 / 129 groups hold the user, each group is held by one document
        for k in (65, 129):
            rows += [s(f"w{k}_{i}", "member", f"uw{k}") for i in range(k)]
            rows += [ss(f"wd{k}_{i}", "view", f"w{k}_{i}", "member") for i in range(k)]
        rows += empty_last
        # a cycle of 3 through the start: the start is the subject set y0#member
        rows += [ss("y1", "member", "y0", "member"), ss("y2", "member", "y1", "member"),
                 ss("y0", "member", "y2", "member")]
        rows += side.star("s1024", ids("m1024_", 1024)) + side.star("s1025", ids("m1025_", 1025))
        rows += side.fan("ufan", ids("fg", 30), 34)
        # a last level of non-interior members: documents held by nobody
        rows += [s("lg", "member", "ul"), ss("ld0", "view", "lg", "member"), ss("ld1", "view", "lg", "member")]
    else:
        # k5#member holds k4#member ... holds k0#member holds the user uk: from k5, uk is 6 hops away
        rows += LookupSide.chain("k", 6, "uk")
        for k in (65, 129):
            rows += [ss(f"wd{k}", "view", f"w{k}_{i}", "member") for i in range(k)]
            rows += [s(f"w{k}_{i}", "member", f"wu{k}_{i}") for i in range(k)]
        rows += empty_last
        rows += [ss("y1", "member", "y0", "member"), ss("y2", "member", "y1", "member"),
                 ss("y0", "member", "y2", "member")]
        rows += side.star("s1024", ids("m1024_", 1024)) + side.star("s1025", ids("m1025_", 1025))
        rows += side.fan("dfan", ids("fg", 30), 34)
        rows += [ss("ldoc", "view", "lg", "member"), s("lg", "member", "lu0"), s("lg", "member", "lu1")]
    return rows


@functools.lru_cache(maxsize=None)
def levels(side_name):
    """-> (snapshot, Truth, {name: start node})"""
    side = SIDES[side_name]
    snap = Snapshot.from_rows(LC.NS1, level_rows(side))
    if side is LookupSide:
        u = lambda n: side.node(snap, n)
        v = {"chain": u("uk"), "w65": u("uw65"), "w129": u("uw129"), "empty_last": u("ue"),
             "cycle": side.set_node(snap, "y0"), "s1024": u("s1024"), "s1025": u("s1025"), "fan": u("ufan"),
             "leaf_level": u("ul")}
    else:
        d = lambda n: side.node(snap, n)
        v = {"chain": side.set_node(snap, "k5"), "w65": d("wd65"), "w129": d("wd129"), "empty_last": d("ed"),
             "cycle": side.set_node(snap, "y0"), "s1024": d("s1024"), "s1025": d("s1025"), "fan": d("dfan"),
             "leaf_level": d("ldoc")}
    assert all(x != NONE for x in v.values()), v
    return snap, Truth(side, snap), v


@functools.lru_cache(maxsize=None)
def structure(side_name):
    """the structure graph of the side's plain tests -> (snapshot, Twin, Truth, named nodes)"""
    side = SIDES[side_name]
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows() if side is LookupSide else SC.structure_rows())
    return snap, Twin(side, snap), Truth(side, snap), side.structure(snap)


def writable_chain_rows():
    """two chains, u0 <- a0 <- a1 <- spare and u1 <- b0 <- b1 <- b2"""
    s, ss = LC.sid, LC.sset
    return [s("a0", "member", "u0"), ss("a1", "member", "a0", "member"), ss("spare", "member", "a1", "member"),
            s("b0", "member", "u1"), ss("b1", "member", "b0", "member"), ss("b2", "member", "b1", "member")]


def writable_chains(side):
    """a writable snapshot with two chains, u0 <- a0 <- a1 <- spare and u1 <- b0 <- b1 <- b2, and
    a write that hangs the second under the first (b0 now holds a1#member): a start's deepest
    member moves from 3 to 5 hops -> (snapshot, start, rows to write).  A writable snapshot pads
    its rows with placeholder nodes, which are interior ids but no members."""
    ss = LC.sset
    rows = writable_chain_rows()
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    x = side.node(snap, "u0") if side is LookupSide else side.set_node(snap, "b2")
    return snap, x, [ss("b0", "member", "a1", "member")]


# ---- checks of one device (or CPU twin) call
def split(out, begin, count):
    return CC.split(out, begin, count)


def assert_depth(side, h, ids, depth, filt, want, want_frontier, null_depth=False):
    """one depth cursor call with exactly the capacity needed: needed = the sum, counts exact,
    nothing TRUNCATED or INVALID, every list equal to `want`, the frontier equal, the segments
    tile [0, needed)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    total = sum(len(w) for w in want)
    out, begin, count, frontier, needed = side.raw(h, ids, None if null_depth else depth, filt, total)
    assert needed == total, (needed, total)
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    for k, (g, w) in enumerate(zip(split(out, begin, count), want)):
        assert np.array_equal(g, w), (k, int(ids[k]), depth, len(g), len(w))
    assert [int(f) for f in frontier] == [int(f) for f in want_frontier], (depth, ids[:8])
    used = np.zeros(total + 1, dtype=np.int32)
    for bg, c in zip(begin, count):
        used[int(bg):int(bg) + int(c)] += 1
    assert (used[:total] == 1).all()


def assert_pages(side, h, ids, depth, lo, filt, limit, want, want_frontier):
    """one depth paged call against the slices of the sorted lists `want`"""
    out, returned, count, remaining, frontier = side.page(h, ids, depth, lo, filt, limit)
    for k, w in enumerate(want):
        f = 0 if lo is None else int(lo[k])
        rest = w[np.searchsorted(w, f, side="left"):]
        assert int(count[k]) == len(w) and int(remaining[k]) == len(rest), (k, f, limit)
        assert int(returned[k]) == min(limit, len(rest))
        assert np.array_equal(out[k, :int(returned[k])], rest[:limit]), (k, f, limit)
    assert [int(f) for f in frontier] == [int(f) for f in want_frontier]


def walk_pages(side, h, x, k, filt, limit):
    """every page of one depth-limited list, by the token rule -> (concatenated ids, calls)"""
    got, lo, calls = [], 0, 0
    while True:
        out, returned, count, remaining, _ = side.page(h, [x], [k], np.array([lo], dtype=np.uint32), filt, limit)
        calls += 1
        r = int(returned[0])
        got.append(out[0, :r].copy())
        tok = lookup.next_page_token(out[0], r, remaining[0])
        if tok == "":
            return np.concatenate(got), calls
        lo = lookup.parse_page_token(tok)


def depth_tiers(truth, ids, depth, cap=1024):
    """(tier-1, tier-2) requests predicted from the unfiltered sets of the yardstick: a request
    goes to tier 2 exactly when its unfiltered M_k passes the set capacity"""
    lists, _ = truth.want(ids, depth, ANY)
    t2 = sum(len(m) > cap for m in lists)
    return len(lists) - t2, t2


def tier_delta(h, call):
    before = h.depth_stats()
    call()
    after = h.depth_stats()
    return (after["tier1_requests"] - before["tier1_requests"], after["tier2_requests"] - before["tier2_requests"])
