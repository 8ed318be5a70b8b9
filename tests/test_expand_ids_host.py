"""CPU tests of expand as id arrays: ketogpu_snapshot_expand_ids, the host twin of
ketogpu_expand over a root that is a snapshot node, and ketogpu_tree_from_ids, which turns
its arrays back into a ketogpu_tree.  The yardstick is ketogpu_expand itself (checked against
the oracle in test_host.py): the flattened tree node for node, the same ENOTFOUND, the same
JSON.  No GPU work is launched here."""
import ctypes as C
import json

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import expand, lookup, persistence
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot, subject_struct
from tests import randgraph

DEPTHS = (0, 1, 2, 3, 100, L.EXPAND_DEPTH_ALL)
NOT_FOUND = "not_found"


def flat_expand(ex, subject, depth):
    """ketogpu_expand's tree as ketogpu_tree_nodes lists it: [(type, num_children, Subject)],
    [] for the nil tree, NOT_FOUND"""
    lib, h = ex.L, C.c_void_p()
    subj = subject_struct(subject)
    rc = lib.ketogpu_expand(ex.snapshot.h, C.byref(subj), expand._depth(min(depth, 2**31 - 1)), C.byref(h))
    if rc == L.ENOTFOUND:
        return NOT_FOUND
    L.check(rc)
    if not h.value:
        return []
    try:
        nodes, n = C.POINTER(L.TreeNode)(), C.c_size_t()
        L.check(lib.ketogpu_tree_nodes(h, C.byref(nodes), C.byref(n)))
        return [(nodes[k].type, nodes[k].num_children, expand._subject(nodes[k].subject)) for k in range(n.value)]
    finally:
        lib.ketogpu_tree_free(h)


def flat_twin(ex, node, depth):
    """the twin's tree in the same form, and its flags"""
    try:
        nodes, kids, flags = ex.expand_ids(int(node), depth)
    except expand.NotFound as e:
        return NOT_FOUND, e.flags
    return [(L.NODE_UNION if k else L.NODE_LEAF, int(k), ex.snapshot.describe(int(v)))
            for v, k in zip(nodes, kids)], flags


def check_subjects(snap, subjects, depths=DEPTHS):
    """twin == ketogpu_expand for every subject that is a snapshot node -> (compared, failed,
    flagged)"""
    ex = expand.Engine(snap)
    ids = lookup.resolve_subjects(snap, subjects)
    compared = failed = flagged = 0
    for s, v in zip(subjects, ids):
        if int(v) == L.NODE_NONE:
            continue
        for d in depths:
            want = flat_expand(ex, s, d)
            got, flags = flat_twin(ex, v, d)
            assert got == want, (s, d)
            if want is NOT_FOUND:
                failed += 1
                assert flags & L.EXPAND_NEEDS_HOST, (s, d)  # set for every request that fails
            else:
                for t, k, _ in want:  # Union iff it has children
                    assert (t == L.NODE_UNION) == (k > 0)
                a, b, _ = ex.expand_ids(int(v), d)
                assert json.loads(ex.json_from_ids(a, b)) == json.loads(ex.build_tree_json(s, min(d, 2**31 - 1)))
                if len(a):
                    assert ex.json_from_ids(a, b) == ex.build_tree_json(s, min(d, 2**31 - 1))
                t = ex.tree_from_ids(a, b)
                bt = ex.BuildTree(s, min(d, 2**31 - 1))
                assert (t.to_node() if t else None) == (bt.to_node() if bt else None)
            flagged += bool(flags & L.EXPAND_NEEDS_HOST)
            compared += 1
    return compared, failed, flagged


def _snapshot_from_case(c):
    ns = [(n["name"], n["id"]) for n in c["namespaces"]]
    store = persistence.TupleStore(ns, page_size=c["page_size"])
    for t in c["tuples"]:
        store.insert(rt.InternalRelationTuple.from_dict(t))
    return Snapshot.from_store(store, batch_rows=2)


def test_twin_matches_expand_on_golden_cases(golden_cases):
    compared = 0
    for c in golden_cases:
        if not c["expands"]:
            continue
        snap = _snapshot_from_case(c)
        subjects = [rt.subject_from_dict(e) for e in c["expands"]]
        depths = sorted(set(DEPTHS) | {max(e["max_depth"], 0) for e in c["expands"]})
        compared += check_subjects(snap, subjects, depths)[0]
    assert compared > 0


@pytest.mark.parametrize("seed,page_size,poison,collide", [(21, 100, False, False), (22, 2, True, False),
                                                            (23, 3, True, True), (24, 1, False, True)])
def test_twin_matches_expand_on_random_tables(seed, page_size, poison, collide):
    namespaces, rows = randgraph.make_graph(seed, n_rows=200, poison=poison, collide=collide)
    snap = Snapshot.from_rows(namespaces, rows, page_size=page_size, sort=True)
    subjects = []
    for (ns, o, r, subj) in randgraph.make_requests(seed, namespaces, rows, n=80):
        subjects += [rt.subject_from_dict(subj), rt.SubjectSet(ns, o, r)]
    compared, failed, flagged = check_subjects(snap, subjects)
    assert compared > 200
    if poison:
        assert failed > 0 and flagged >= failed
    else:
        assert failed == 0 and flagged == 0  # never set on tables without poison


def test_every_node_as_root_equals_expand():
    """all N nodes, not only the ones requests name"""
    namespaces, rows = randgraph.make_graph(22, n_rows=200, poison=True)
    snap = Snapshot.from_rows(namespaces, rows, page_size=2, sort=True)
    subjects = [snap.describe(v) for v in range(snap.stats()["num_nodes"])]
    compared, failed, _ = check_subjects(snap, subjects, depths=(1, 2, 3, L.EXPAND_DEPTH_ALL))
    assert compared >= 4 * len(subjects) - 8 and failed > 0


def test_root_outside_the_snapshot_and_bad_arrays():
    snap = Snapshot.from_rows([("n", 1)], [(1, "doc", "view", "alice", None, None, None)])
    ex = expand.Engine(snap)
    for bad in (snap.stats()["num_nodes"], L.NODE_NONE):
        with pytest.raises(L.KetoError) as e:
            ex.expand_ids(bad, 3)
        assert e.value.code == L.EINVAL
    a, b, flags = ex.expand_ids(rt.SubjectSet("n", "doc", "view"), 3)
    assert list(b) == [1, 0] and flags == 0
    assert ex.json_from_ids(a[:0], b[:0]) == "null"
    for nodes, kids in (([a[0]], [1]), ([a[0], a[1], a[1]], [1, 0, 0]), ([snap.stats()["num_nodes"]], [0])):
        with pytest.raises(L.KetoError) as e:
            ex.json_from_ids(nodes, kids)
        assert e.value.code == L.EINVAL


def test_host_batch_equals_build_tree():
    namespaces, rows = randgraph.make_graph(22, n_rows=200, poison=True)
    snap = Snapshot.from_rows(namespaces, rows, page_size=2, sort=True)
    ex = expand.Engine(snap)
    subjects, depths = [], []
    for k, (ns, o, r, subj) in enumerate(randgraph.make_requests(22, namespaces, rows, n=60)):
        subjects += [rt.subject_from_dict(subj), rt.SubjectSet(ns, o, r), rt.SubjectSet("", o, "")]
        depths += [k % 5, 3, 2]
    got = ex.build_trees_batch(subjects, depths)
    errors = 0
    for s, d, t in zip(subjects, depths, got):
        try:
            want = ex.BuildTree(s, d)
            assert not isinstance(t, expand.NotFound)
            assert (t.to_node() if t else None) == (want.to_node() if want else None), (s, d)
        except expand.NotFound as e:
            assert isinstance(t, expand.NotFound) and str(t) == str(e), (s, d)
            errors += 1
    assert errors > 0
