"""Pairs, expectations and checks shared by the combined-listing tests (test_combine_host.py on
the CPU, test_combine_lookup_gpu.py / test_combine_subjects_gpu.py on the device).  A `Side`
says what differs between the two handles: which class, which host list, how a named star is
spelled in rows and resolved to a node.  The yardstick is numpy set algebra over the host lists
(ketogpu_snapshot_lookup / ketogpu_snapshot_subjects), which the host tests pin against the
oracle."""
import numpy as np

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import lookup_cases as LC

ANY, NONE = lookup.TYPE_ANY, L.NODE_NONE
OPS = {lookup.OP_AND: np.intersect1d, lookup.OP_ANDNOT: np.setdiff1d, lookup.OP_OR: np.union1d}
OP_IDS = list(OPS)
OP_NAMES = {lookup.OP_AND: "and", lookup.OP_ANDNOT: "andnot", lookup.OP_OR: "or"}


class LookupSide:
    name = "lookup"
    Handle, Host = lookup.Lookup, lookup.HostLookup
    tier_env, slots_env = "KETOGPU_LOOKUP_TIER", "KETOGPU_LOOKUP_SLOTS"
    host = staticmethod(lookup.host_lookup)

    @staticmethod
    def has_row(snap, x):  # every node has a reverse row
        return x < snap.stats()["num_nodes"]

    @staticmethod
    def sample_bound(snap):
        return snap.stats()["num_nodes"]

    @staticmethod
    def star(name, members):
        """user `name` is held directly by the documents `members`: M(name) is exactly these"""
        return [LC.sid(m, "view", name) for m in members]

    @staticmethod
    def node(snap, name):
        return int(lookup.resolve_subjects(snap, [rt.SubjectID(name)])[0])

    @staticmethod
    def plain_raw(h, ids, filt, cap):
        return h.lookup_ids_raw(ids, filt, cap)

    @staticmethod
    def plain_page(h, ids, lo, filt, limit):
        return h.lookup_page_raw(ids, lo, filt, limit)

    @staticmethod
    def structure(snap):
        """the named nodes of LC.structure_rows(): M(mid) is a subset of M(chain)"""
        s = lambda o, r="member": int(lookup.resolve_subjects(snap, [rt.SubjectSet("n", o, r)])[0])
        u = lambda n: LookupSide.node(snap, n)
        return {"chain": u("uc"), "mid": s("c1500"), "cycle": s("ya"), "self": s("self"), "diamond": u("ux"),
                "diamond_size": 4, "chain_size": 3000}


class SubjectsSide:
    name = "subjects"
    Handle, Host = lookup.Subjects, lookup.HostSubjects
    tier_env, slots_env = "KETOGPU_SUBJECTS_TIER", "KETOGPU_SUBJECTS_SLOTS"
    host = staticmethod(lookup.host_subjects)

    @staticmethod
    def has_row(snap, x):  # only the expandable nodes have a forward row
        return x < snap.stats()["num_expandable"]

    @staticmethod
    def sample_bound(snap):
        return snap.stats()["num_expandable"]

    @staticmethod
    def star(name, members):
        """document `name` is held directly by the users `members`: M(name#view) is exactly these"""
        return [LC.sid(name, "view", m) for m in members]

    @staticmethod
    def node(snap, name):
        return int(lookup.resolve_roots(snap, [("n", name, "view")])[0])

    @staticmethod
    def plain_raw(h, ids, filt, cap):
        return h.subject_ids_raw(ids, filt, cap)

    @staticmethod
    def plain_page(h, ids, lo, filt, limit):
        return h.subject_page_raw(ids, lo, filt, limit)

    @staticmethod
    def structure(snap):
        s = lambda o, r="member": int(lookup.resolve_roots(snap, [("n", o, r)])[0])
        return {"chain": s("c2999"), "mid": s("c1500"), "cycle": s("ya"), "self": s("self"),
                "diamond": s("top", "view"), "diamond_size": 4, "chain_size": 3000}


def pair_sample(n, seed):
    """every node paired with itself, with NONE on either side, and with 6 partners from a
    seeded rng -> (a, b)"""
    ids = np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    a = [ids, ids, np.full(n, NONE, dtype=np.uint32)] + [ids] * 6
    b = [ids, np.full(n, NONE, dtype=np.uint32), ids] + [rng.integers(0, n, n).astype(np.uint32) for _ in range(6)]
    return np.concatenate(a), np.concatenate(b)


class Members:
    """M(x) under a filter from the host list, memoized per (x, filter); NONE is the empty set"""

    def __init__(self, side, snap):
        self.side, self.snap, self.memo = side, snap, {}

    def __call__(self, x, filt=ANY):
        x = int(x)
        if x == NONE:
            return np.zeros(0, dtype=np.uint32)
        if (x, filt) not in self.memo:
            self.memo[(x, filt)] = self.side.host(self.snap, x, filt)
        return self.memo[(x, filt)]

    def want(self, a, b, op, filt=ANY):
        return [OPS[op](self(x, filt), self(y, filt)).astype(np.uint32) for x, y in zip(a, b)]


def unlisted(side, snap, a, b):
    """pairs neither side of which has a row to read (the ids are valid or NONE)"""
    return sum(not side.has_row(snap, int(x)) and not side.has_row(snap, int(y)) for x, y in zip(a, b))


def split(out, begin, count):
    """the lists of one raw call, each sorted; a truncated list is None"""
    return [None if b == lookup.TRUNCATED else np.sort(out[int(b):int(b) + int(c)]) for b, c in zip(begin, count)]


def assert_combined(h, a, b, op, filt, want):
    """one combined call with exactly the capacity needed: needed = the sum, counts exact,
    nothing TRUNCATED or INVALID, every list equal to `want`, the segments tile [0, needed)"""
    total = sum(len(w) for w in want)
    out, begin, count, needed = h.combine_ids_raw(a, b, op, filt, total)
    assert needed == total
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    for k, (g, w) in enumerate(zip(split(out, begin, count), want)):
        assert np.array_equal(g, w), (k, int(a[k]), int(b[k]), op, len(g), len(w))
    used = np.zeros(total + 1, dtype=np.int32)
    for bg, c in zip(begin, count):
        used[int(bg):int(bg) + int(c)] += 1
    assert (used[:total] == 1).all()


def assert_pages(h, a, b, op, lo, filt, limit, want):
    """one combined paged call against the slices of the sorted lists `want`"""
    out, returned, count, remaining = h.combine_page_raw(a, b, op, lo, filt, limit)
    for k, w in enumerate(want):
        f = 0 if lo is None else int(lo[k])
        rest = w[np.searchsorted(w, f, side="left"):]
        assert int(count[k]) == len(w) and int(remaining[k]) == len(rest), (k, f, limit)
        assert int(returned[k]) == min(limit, len(rest))
        assert np.array_equal(out[k, :int(returned[k])], rest[:limit]), (k, f, limit)


def boundary_rows(side):
    """stars around set_capacity = 1024 in one snapshot: 1024 and 1025; disjoint 512 / 512 / 513;
    700 + 700 that share 376 (a union of 1024) and 700 + 700 that share 375 (1025)"""
    ids = lambda p, lo, hi: [f"{p}{i}" for i in range(lo, hi)]
    rows = side.star("s1024", ids("m1024_", 0, 1024)) + side.star("s1025", ids("m1025_", 0, 1025))
    rows += side.star("d512a", ids("da_", 0, 512)) + side.star("d512b", ids("db_", 0, 512))
    rows += side.star("d513", ids("dc_", 0, 513))
    rows += side.star("ov_a", ids("oa_", 0, 700))
    rows += side.star("ov_b", ids("oa_", 324, 700) + ids("ob_", 0, 324))  # 376 shared
    rows += side.star("ov_c", ids("oa_", 325, 700) + ids("oc_", 0, 325))  # 375 shared
    return rows
