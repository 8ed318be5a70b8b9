"""The graphs of tests/expand_cases.py have the shapes their names promise, by the host walk
alone (no GPU): test_expand_gpu.py runs the device over them."""
from keto_amd import _lib as L
from keto_amd import expand
from keto_amd import relationtuple as rt
from tests import expand_cases as EC


def _tree(ex, subject, depth=EC.ALL):
    a, b, flags = ex.expand_ids(EC.node_of(ex.snapshot, subject), depth)
    assert flags == 0
    return a, b


def test_shapes():
    snap = EC.shapes()
    ex = expand.Engine(snap)
    view = lambda x: rt.SubjectSet("n", x, "view")
    for k in (63, 64, 65, 129, 257):
        a, b = _tree(ex, view(f"L{k}_r"))
        assert len(a) == k + 1 and b[0] == k and not b[1:].any()
    for p in (0, 63, 64):
        a, b = _tree(ex, view(f"P{p}_r"))
        assert [i for i, c in enumerate(EC.children_of_root(a, b)) if b[c]] == [p] and len(a) == 68
    a, b = _tree(ex, view("two_r"))
    assert [i for i, c in enumerate(EC.children_of_root(a, b)) if b[c]] == [3, 10]
    a, b = _tree(ex, view("dup"))
    assert list(b) == [1, 3, 1, 0, 0, 0] and a[2] == a[5]
    assert list(_tree(ex, view("hg"))[1]) == [2, 1, 1, 0, 0] and list(_tree(ex, view("gh"))[1]) == [2, 1, 0, 1, 0]
    assert list(_tree(ex, view("dm"), 3)[1]) == [2, 1, 0, 0] and list(_tree(ex, view("dm"), 4)[1]) == [2, 1, 1, 0, 0]
    assert list(_tree(ex, EC.member("t1"))[1]) == [2, 1, 1, 0, 0] and list(_tree(ex, EC.member("self"))[1]) == [2, 0, 0]
    assert len(_tree(ex, EC.member("c2999"))[0]) == 3001 and len(_tree(ex, EC.member("e999"))[0]) == 1001
    assert len(_tree(ex, EC.member("norows"))[0]) == 0
    assert EC.twin(ex, L.NODE_NONE, 3)[0] == L.EXPAND_NIL and EC.twin(ex, snap.stats()["num_nodes"], 3)[3]


def test_fans_open_the_set_capacity_and_one_more():
    snap = EC.fans()
    ex = expand.Engine(snap)
    for prefix, opened in (("A", EC.SET_CAP), ("B", EC.SET_CAP + 1)):
        a, b = _tree(ex, rt.SubjectSet("n", f"{prefix}top", "view"))
        assert int((b > 0).sum()) == opened and len(a) == 2 * opened - 1


def test_truth_tables_split_between_host_and_device():
    """tables 31 and 41 never need the host; on 42 and 43 some requests do and some do not"""
    from tests import lookup_cases as LC
    for t in LC.TABLES:
        snap = LC.table(*t)[2]
        ex = expand.Engine(snap)
        st = [EC.twin(ex, v, d)[0] for v in range(snap.stats()["num_nodes"]) for d in (1, 2, 3, EC.ALL)]
        host = sum(s == L.EXPAND_HOST for s in st)
        assert (0 < host < len(st)) if t[4] else host == 0
