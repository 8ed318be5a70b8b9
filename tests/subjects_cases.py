"""Graphs and helpers shared by the subject-listing tests (test_subjects_host.py on the CPU,
test_subjects_gpu.py on the device).  Rows are raw keto_relation_tuples rows as in randgraph."""
import functools

import numpy as np

from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import lookup_cases as LC
from tests import randgraph

ANY, IDS = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID


def fwd_star_rows(doc, k, prefix):
    """`doc` is held directly by k users: its row has exactly k entries"""
    return [LC.sid(doc, "view", f"{prefix}{i}") for i in range(k)]


def fwd_split_rows(doc, k, prefix):
    """F(doc#view) has exactly k nodes: two groups that hold the document, and k - 2 users of
    whom half are members of both groups, so their ids arrive from two rows"""
    ga, gb = f"{prefix}ga", f"{prefix}gb"
    rows = [LC.sset(doc, "view", ga, "member"), LC.sset(doc, "view", gb, "member")]
    nu = k - 2
    shared = nu // 2
    only_a = (nu - shared) // 2
    for i in range(nu):
        if i < only_a or i >= nu - shared:
            rows.append(LC.sid(ga, "member", f"{prefix}u{i}"))
        if i >= only_a:
            rows.append(LC.sid(gb, "member", f"{prefix}u{i}"))
    return rows


def structure_rows():
    """LC.structure_rows() plus documents held directly by 65 and 129 users (forward rows that
    cross the 64-entry read step) and a document held through two groups that share half their
    members (one id arrives from two rows)"""
    return (LC.structure_rows() + fwd_star_rows("f65", 65, "f65_") + fwd_star_rows("f129", 129, "f129_")
            + fwd_split_rows("two", 42, "two_"))


@functools.lru_cache(maxsize=None)
def oracle_matrix(case):
    """want[t][r] = Check(r, t) for every node t and every expandable node r of one LC.TABLES
    entry, by the CPU oracle (the matrix of test_lookup_host.py)"""
    seed, n_rows, n_obj, page_size, poison = case
    namespaces, rows, snap = LC.table(*case)
    st = snap.stats()
    assert st["num_ambiguous_nodes"] == 0
    n, nx = st["num_nodes"], st["num_expandable"]
    orc = randgraph.oracle_store(namespaces, rows, page_size)
    roots = [snap.describe(r) for r in range(nx)]
    assert all(isinstance(r, rt.SubjectSet) for r in roots)
    subjects = [snap.describe(t).to_dict() for t in range(n)]
    reqs = [(r.namespace, r.object, r.relation, s) for s in subjects for r in roots]
    return np.asarray(orc.check_batch(reqs, nthreads=4)).reshape(n, nx)


def forward_closure(snap, root):
    """F(root) from the transpose of the snapshot's reverse rows, in plain Python (a second
    implementation for the structure cases)"""
    g = snap.graph()
    ro, rc = g["rev_off"], g["rev_col"]
    succ = {}
    for t in range(g["N"]):
        for r in rc[int(ro[t]):int(ro[t + 1])]:
            succ.setdefault(int(r), []).append(t)
    seen, stack = set(), [int(root)]
    while stack:
        v = stack.pop()
        for u in succ.get(v, ()):
            if u not in seen:
                seen.add(u)
                if u < g["Ni"]:
                    stack.append(u)
    return np.array(sorted(seen), dtype=np.uint32)


def host_lists(snap, roots, cls=ANY):
    return [lookup.host_subjects(snap, int(r), cls) for r in roots]
