"""The yardstick shared by the path tests (test_paths_host.py on the CPU, test_paths_gpu.py on
the device): what makes a path valid and shortest, judged from the snapshot's reverse rows in
plain Python.  Equality of paths is never asserted: any path with the fewest hops is right."""
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import lookup
from tests import lookup_cases as LC

NONE = L.NODE_NONE


class Rows:
    """the reverse rows of a snapshot's current version (snapshot.graph(), copied once)"""

    def __init__(self, snap):
        g = snap.graph()
        self.ro, self.rc = g["rev_off"], g["rev_col"]
        self.n, self.nx, self.ni = int(g["N"]), int(g["Nx"]), int(g["Ni"])

    def row(self, v):
        return self.rc[int(self.ro[v]):int(self.ro[v + 1])]

    def distances(self, target):
        """{node: hops} of a level BFS from `target` over the rows: the fewest hops of a path
        node ... target (>= 1; the target itself appears only through a cycle)"""
        dist, level, d = {}, [int(target)], 0
        while level:
            d += 1
            nxt = []
            for v in level:
                for u in self.row(v).tolist():
                    if u < self.nx and u not in dist:
                        dist[u] = d
                        if u < self.ni:
                            nxt.append(u)
            level = nxt
        return dist

    def assert_valid(self, path, root, target):
        """starts at root, ends at target, >= 2 nodes, and every hop v(i) -> v(i+1) has v(i)
        in the row of v(i+1)"""
        path = [int(v) for v in path]
        assert len(path) >= 2, path
        assert path[0] == int(root) and path[-1] == int(target), (path[:3], path[-3:], root, target)
        for a, b in zip(path, path[1:]):
            assert b < self.n and a in self.row(b), (a, b)

    def assert_shortest(self, path, root, target, dist=None):
        self.assert_valid(path, root, target)
        dist = self.distances(target) if dist is None else dist
        assert len(path) - 1 == dist[int(root)], (len(path) - 1, dist[int(root)], int(root), int(target))


@functools.lru_cache(maxsize=None)
def table_truth(case):
    """one of lookup_cases.TABLES -> (snapshot, rows, roots, targets, want, dists): every
    expandable node as root x every node as target, want[i] the host call's path (computed
    once, shared, never changed), dists[t] the BFS levels of target t"""
    _, _, snap = LC.table(*case)
    rows = Rows(snap)
    targets = np.repeat(np.arange(rows.n, dtype=np.uint32), rows.nx)
    roots = np.tile(np.arange(rows.nx, dtype=np.uint32), rows.n)
    want = [lookup.host_path(snap, int(r), int(t)) for r, t in zip(roots, targets)]
    dists = [rows.distances(t) for t in range(rows.n)]
    return snap, rows, roots, targets, want, dists


def split_paths(out, begin, count):
    """the paths of one raw call; a truncated path is None"""
    return [None if b == lookup.TRUNCATED else out[int(b):int(b) + int(c)] for b, c in zip(begin, count)]


def check_raw(rows, roots, targets, want, raw, dists=None):
    """one raw call with capacity >= needed against the host's paths: the same counts, nothing
    truncated or invalid, every path valid and shortest, the segments disjoint"""
    out, begin, count, needed = raw
    total = sum(len(w) for w in want)
    assert needed == total
    assert [int(c) for c in count] == [len(w) for w in want]
    assert not (begin == lookup.TRUNCATED).any() and not (begin == lookup.INVALID).any()
    used = np.zeros(total + 1, dtype=np.int32)
    for k, (p, w) in enumerate(zip(split_paths(out, begin, count), want)):
        if not len(w):
            continue
        r, t = int(roots[k]), int(targets[k])
        rows.assert_shortest(p, r, t, None if dists is None else dists[t])
        used[int(begin[k]):int(begin[k]) + len(p)] += 1
    assert (used[:total] == 1).all()
