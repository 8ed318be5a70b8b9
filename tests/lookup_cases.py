"""Graphs and helpers shared by the reverse-lookup tests (test_lookup_host.py on the CPU,
test_lookup_gpu.py on the device).  Rows are raw keto_relation_tuples rows as in randgraph."""
import functools

import numpy as np

from keto_amd.snapshot import Snapshot
from tests import randgraph

# (seed, n_rows, n_obj, page_size, poison): 31 is dense (most roots reach most targets), 41-43
# are sparse; 42 and 43 truncate pages at rows of unconfigured namespaces (R7)
TABLES = [(31, 600, 30, 100, False), (41, 260, 60, 100, False), (42, 260, 60, 3, True), (43, 400, 80, 2, True)]


@functools.lru_cache(maxsize=None)
def table(seed, n_rows, n_obj, page_size, poison):
    """-> (namespaces, rows, snapshot) of one random table (wildcard subject sets included)"""
    namespaces, rows = randgraph.make_graph(seed, n_rows=n_rows, n_obj=n_obj, n_users=40, poison=poison,
                                            collide=False, empty_ns=False)
    return namespaces, rows, Snapshot.from_rows(namespaces, rows, page_size=page_size, sort=True)


def sid(obj, rel, user, ns=1):
    return (ns, obj, rel, user, None, None, None)


def sset(obj, rel, sobj, srel, ns=1, sns=1):
    return (ns, obj, rel, None, sns, sobj, srel)


def star_rows(user, k, prefix):
    """`user` is held directly by k documents: rev(user) has exactly k entries"""
    return [sid(f"{prefix}{i}", "view", user) for i in range(k)]


def split_star_rows(user, k, prefix):
    """B(user) has exactly k nodes: two groups that hold the user, and k - 2 documents of which
    half are held through both groups, so their ids arrive from two rows"""
    ga, gb = f"{prefix}ga", f"{prefix}gb"
    rows = [sid(ga, "member", user), sid(gb, "member", user)]
    nd = k - 2
    shared = nd // 2
    only_a = (nd - shared) // 2
    for i in range(nd):
        if i < only_a or i >= nd - shared:
            rows.append(sset(f"{prefix}d{i}", "view", ga, "member"))
        if i >= only_a:
            rows.append(sset(f"{prefix}d{i}", "view", gb, "member"))
    return rows


def structure_rows():
    """one graph with a part per structural case (names do not overlap):
    chains of 3000 and 1000 groups under users uc / ud, a 2-cycle and a self-loop, a diamond,
    stars of 65 and 129 documents, a document nobody holds"""
    rows = [sid("c0", "member", "uc"), sid("e0", "member", "ud")]
    rows += [sset(f"c{i + 1}", "member", f"c{i}", "member") for i in range(2999)]
    rows += [sset(f"e{i + 1}", "member", f"e{i}", "member") for i in range(999)]
    rows += [sset("ya", "member", "yb", "member"), sset("yb", "member", "ya", "member"), sid("ya", "member", "uy")]
    rows += [sset("self", "member", "self", "member"), sid("self", "member", "us")]
    rows += [sid("g0", "member", "ux"), sset("g1", "member", "g0", "member"), sset("g2", "member", "g0", "member"),
             sset("top", "view", "g1", "member"), sset("top", "view", "g2", "member")]
    rows += star_rows("u65", 65, "s65_") + star_rows("u129", 129, "s129_")
    rows += [sid("lonely", "view", "ul")]
    return rows


NS1 = [("n", 1)]


def closure(snap, target):
    """B(target) from the snapshot's reverse rows, in plain Python (a second implementation
    for the structure cases)"""
    g = snap.graph()
    ro, rc = g["rev_off"], g["rev_col"]
    seen, stack = set(), [int(target)]
    while stack:
        v = stack.pop()
        for u in rc[int(ro[v]):int(ro[v + 1])]:
            u = int(u)
            if u not in seen:
                seen.add(u)
                if u < g["Ni"]:
                    stack.append(u)
    return np.array(sorted(seen), dtype=np.uint32)
