"""Graphs and the yardstick shared by the expand tests (test_expand_gpu.py on the device; the
shapes are checked against the host on the CPU in test_expand_cases_host.py).  Rows are raw
keto_relation_tuples rows as in randgraph; the backend orders a query's rows by the subject's
object name here, so the names fix each row's order."""
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests.lookup_cases import NS1, sid, sset, structure_rows

ALL = L.EXPAND_DEPTH_ALL
SET_CAP = 1024  # closure.hpp kSetCap (the stats' set_capacity)


def member(name):
    return rt.SubjectSet("n", name, "member")


def node_of(snap, subject):
    v = int(lookup.resolve_subjects(snap, [subject])[0])
    assert v != L.NODE_NONE, subject
    return v


def twin(ex, root, depth):
    """what ketogpu_subjects_expand owes for (root, depth), from the host twin ->
    (status, nodes, num_children, invalid)"""
    empty = np.zeros(0, np.uint32)
    n = ex.snapshot.stats()["num_nodes"]
    if int(root) >= n:
        return L.EXPAND_NIL, empty, empty, int(root) != L.NODE_NONE
    try:
        nodes, kids, flags = ex.expand_ids(int(root), int(depth))
    except expand.NotFound as e:
        assert e.flags & L.EXPAND_NEEDS_HOST
        return L.EXPAND_HOST, empty, empty, False
    if flags & L.EXPAND_NEEDS_HOST:
        return L.EXPAND_HOST, empty, empty, False
    return (L.EXPAND_OK if len(nodes) else L.EXPAND_NIL), nodes, kids, False


def assert_device(dev, ex, roots, depths):
    """one count-only call and one exact call of the device against the twin, word for word
    -> the statuses"""
    roots = np.asarray(roots, dtype=np.uint32)
    depths = np.broadcast_to(np.asarray(depths, dtype=np.uint32), roots.shape)
    want = [twin(ex, r, d) for r, d in zip(roots, depths)]
    total = sum(len(w[1]) for w in want)
    _, _, begin0, count0, status0, needed0 = dev.expand_ids_raw(roots, depths, 0)
    nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, total)
    assert needed0 == needed == total
    for i, (st, wn, wk, invalid) in enumerate(want):
        where = (i, int(roots[i]), int(depths[i]))
        assert status[i] == status0[i] == st, where
        assert count[i] == count0[i] == len(wn), where
        if invalid:
            assert begin[i] == begin0[i] == L.LOOKUP_INVALID, where
        elif len(wn):
            assert begin0[i] == L.LOOKUP_TRUNCATED, where
            b = int(begin[i])
            assert b + len(wn) <= total, where
            assert (nodes[b:b + len(wn)] == wn).all() and (kids[b:b + len(wn)] == wk).all(), where
    return status


def row_with_sets_at(k, at, prefix):
    """root `<prefix>r#view` whose row has k subject sets x000 .. in name order; the ones at the
    positions `at` have a row of their own (one user), the others none"""
    rows = [sset(f"{prefix}r", "view", f"{prefix}x{i:03d}", "member") for i in range(k)]
    rows += [sid(f"{prefix}x{i:03d}", "member", f"{prefix}u{i}") for i in at]
    return rows


def shape_rows():
    """one graph with a part per structural case of the walk (names do not overlap)"""
    rows = structure_rows()
    for k in (63, 64, 65, 129, 257):  # leaf-only rows around the 64- and 256-entry windows
        rows += row_with_sets_at(k, (), f"L{k}_")
    for p in (0, 63, 64):  # one child that opens, at these positions of a row of 66
        rows += row_with_sets_at(66, (p,), f"P{p}_")
    rows += row_with_sets_at(40, (3, 10), "two_")  # two fresh children in one window
    # the row [g, u, g] of the wildcard node n:o# (every relation of o, in relation order)
    rows += [sset("dup", "view", "o", ""), sset("o", "a", "g", "member"), sid("o", "b", "u"),
             sset("o", "c", "g", "member"), sid("g", "member", "ug")]
    # [h, g] with g inside h's subtree, and the mirror [g, h]
    rows += [sset("hg", "view", "hg_a_h", "member"), sset("hg", "view", "hg_b_g", "member"),
             sset("hg_a_h", "member", "hg_b_g", "member"), sid("hg_b_g", "member", "uhg")]
    rows += [sset("gh", "view", "gh_a_g", "member"), sset("gh", "view", "gh_b_h", "member"),
             sset("gh_b_h", "member", "gh_a_g", "member"), sid("gh_a_g", "member", "ugh")]
    # depth marking: R -> [a, b], a -> [b], b -> [u]
    rows += [sset("dm", "view", "dm_a", "member"), sset("dm", "view", "dm_b", "member"),
             sset("dm_a", "member", "dm_b", "member"), sid("dm_b", "member", "udm")]
    # a 3-cycle
    rows += [sset("t1", "member", "t2", "member"), sset("t2", "member", "t3", "member"),
             sset("t3", "member", "t1", "member"), sid("t1", "member", "ut")]
    # a subject set that is named but has no rows
    rows += [sset("named", "view", "norows", "member")]
    return rows


@functools.lru_cache(maxsize=None)
def shapes():
    snap = Snapshot.from_rows(NS1, shape_rows())
    return snap


def fan_rows(k, prefix):
    """root -> k groups with one user each: a walk without a depth limit opens k + 1 nodes"""
    rows = [sset(f"{prefix}top", "view", f"{prefix}f{i:04d}", "member") for i in range(k)]
    rows += [sid(f"{prefix}f{i:04d}", "member", f"{prefix}u") for i in range(k)]
    return rows


@functools.lru_cache(maxsize=None)
def fans():
    """the fans that open exactly SET_CAP nodes and one more"""
    return Snapshot.from_rows(NS1, fan_rows(SET_CAP - 1, "A") + fan_rows(SET_CAP, "B"))


def children_of_root(nodes, kids):
    """the positions in the arrays of the root's children"""
    out, k = [], 1
    for _ in range(int(kids[0])):
        out.append(k)
        open_ = 1
        while open_:
            open_ += int(kids[k]) - 1
            k += 1
    return out
