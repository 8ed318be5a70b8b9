"""Why a check is allowed, on the host (ketogpu_snapshot_path, lookup.host_path, HostLookup):
one path root ... target with the fewest hops over the reverse rows.  Pinned against
ketogpu_snapshot_lookup (itself pinned against the oracle) and the oracle's check as full truth
tables, and against a plain-Python level BFS for validity and length (tests/path_cases.py);
no GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import path_cases as PC
from tests import randgraph


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_table_paths_are_valid_and_shortest(case):
    snap, rows, roots, targets, want, dists = PC.table_truth(case)
    longest, allowed = 0, 0
    for t in range(rows.n):
        members = set(lookup.host_lookup(snap, t, lookup.TYPE_ANY).tolist())
        assert members == set(dists[t])  # the BFS of the yardstick reaches B(t)
        for r in range(rows.nx):
            p = want[t * rows.nx + r]
            assert (len(p) > 0) == (r in members), (r, t)
            if len(p):
                rows.assert_shortest(p, r, t, dists[t])
                longest = max(longest, len(p))
                allowed += 1
    assert allowed > 50 and longest >= 4  # the tables are not vacuous: chains of three hops and more


def test_allowed_matches_the_oracle_check():
    case = LC.TABLES[1]
    namespaces, table_rows, _ = LC.table(*case)
    snap, rows, roots, targets, want, _ = PC.table_truth(case)
    orc = randgraph.oracle_store(namespaces, table_rows, case[3])
    described = [snap.describe(r) for r in range(rows.nx)]
    subjects = [snap.describe(t).to_dict() for t in range(rows.n)]
    reqs = [(r.namespace, r.object, r.relation, s) for s in subjects for r in described]
    allowed = np.asarray(orc.check_batch(reqs, nthreads=4), dtype=bool)
    got = np.array([len(p) > 0 for p in want])
    assert (got == allowed).all(), np.nonzero(got != allowed)[0][:5]
    assert 0 < got.sum() < len(got)


@pytest.fixture(scope="module")
def structure():
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows())
    return snap, PC.Rows(snap)


def root_of(snap, obj, rel):
    return int(lookup.resolve_roots(snap, [("n", obj, rel)])[0])


def target_of(snap, subject):
    return int(lookup.resolve_subjects(snap, [subject])[0])


def test_structure_cases_on_the_host(structure):
    snap, rows = structure
    user = lambda u: target_of(snap, rt.SubjectID(u))
    path = lambda r, t: lookup.host_path(snap, r, t)
    p = path(root_of(snap, "c2999", "member"), user("uc"))  # no depth cutoff (R2)
    assert len(p) == 3001
    rows.assert_valid(p, p[0], user("uc"))
    assert len(set(p.tolist())) == 3001
    ya = root_of(snap, "ya", "member")
    assert ya == target_of(snap, rt.SubjectSet("n", "ya", "member"))
    p = path(ya, ya)  # root = target is answered through the cycle
    assert len(p) == 3 and p[1] == root_of(snap, "yb", "member")
    rows.assert_shortest(p, ya, ya)
    me = root_of(snap, "self", "member")
    assert path(me, me).tolist() == [me, me]
    g0 = root_of(snap, "g0", "member")
    assert len(path(g0, g0)) == 0  # no cycle: a node does not reach itself
    top = root_of(snap, "top", "view")
    p = path(top, user("ux"))  # the diamond: through either branch
    assert len(p) == 4 and p[1] in (root_of(snap, "g1", "member"), root_of(snap, "g2", "member")) and p[2] == g0
    rows.assert_shortest(p, top, user("ux"))
    lonely = root_of(snap, "lonely", "view")
    assert len(path(top, lonely)) == 0 and len(path(lonely, user("ux"))) == 0
    assert len(path(top, user("uc"))) == 0 and len(path(root_of(snap, "c5", "member"), user("ud"))) == 0  # cross-part
    assert len(path(lonely, user("ul"))) == 2
    # NONE in either field and never-expanded roots: the empty path
    assert len(path(PC.NONE, user("ux"))) == 0 and len(path(top, PC.NONE)) == 0 and len(path(PC.NONE, PC.NONE)) == 0
    assert user("ux") >= rows.nx and len(path(user("ux"), user("ux"))) == 0 and len(path(user("uc"), g0)) == 0
    for bad in (rows.n, rows.n + 7, 0xFFFFFFFE):
        for pair in ((bad, user("ux")), (top, bad), (bad, PC.NONE), (PC.NONE, bad)):
            with pytest.raises(L.KetoError) as e:
                path(*pair)
            assert e.value.code == L.EINVAL


def test_ambiguous_keys_are_refused():
    namespaces, table_rows = randgraph.make_graph(23, n_rows=200, poison=True, collide=True)
    snap = Snapshot.from_rows(namespaces, table_rows, page_size=3, sort=True)
    assert snap.stats()["num_ambiguous_nodes"] > 0
    with pytest.raises(L.KetoError) as e:
        lookup.host_path(snap, 0, 1)
    assert e.value.code == L.EINVAL


def test_explain_names_round_trip(structure):
    snap, rows = structure
    hl = lookup.HostLookup(snap)
    got = hl.Explain("n", "top", "view", rt.SubjectID("ux"))
    assert got[0] == rt.SubjectSet("n", "top", "view") and got[-1] == rt.SubjectID("ux")
    assert got[1] in (rt.SubjectSet("n", "g1", "member"), rt.SubjectSet("n", "g2", "member"))
    assert got[2] == rt.SubjectSet("n", "g0", "member") and len(got) == 4
    # a subject set as the subject, in both forms resolve_subjects takes
    for subject in (rt.SubjectSet("n", "g0", "member"), rt.SubjectSet("n", "g0", "member").to_dict()):
        assert hl.Explain("n", "top", "view", subject)[-1] == rt.SubjectSet("n", "g0", "member")
    tuples = [("n", "top", "view", rt.SubjectID("ux")), ("n", "top", "view", rt.SubjectID("uc")),
              ("n", "self", "member", rt.SubjectSet("n", "self", "member")), ("nowhere", "top", "view", rt.SubjectID("ux")),
              ("n", "c40", "member", rt.SubjectID("uc")), ("n", "top", "view", rt.SubjectID("nobody"))]
    batch = hl.explain_batch(tuples)
    assert batch[0] == got and batch[1] == [] and batch[3] == [] and batch[5] == []
    assert batch[2] == [rt.SubjectSet("n", "self", "member")] * 2
    assert len(batch[4]) == 42 and batch[4][1] == rt.SubjectSet("n", "c39", "member")
    # the names resolve back to the ids of the path
    ids = hl.path_ids([root_of(snap, "c40", "member")], [target_of(snap, rt.SubjectID("uc"))])[0]
    back = [root_of(snap, s.object, s.relation) for s in batch[4][:-1]] + [target_of(snap, batch[4][-1])]
    assert back == ids.tolist()
    assert hl.explain_batch([]) == []
    with pytest.raises(L.KetoError) as e:  # a nil subject, as in check
        hl.Explain("n", "top", "view", None)
    assert e.value.code == L.EINVAL


def test_host_twin_follows_the_truncation_protocol(structure):
    snap, rows = structure
    hl = lookup.HostLookup(snap)
    top, ux = root_of(snap, "top", "view"), target_of(snap, rt.SubjectID("ux"))
    roots = np.array([top, top, rows.n + 1, PC.NONE, top], dtype=np.uint32)
    targets = np.array([ux, target_of(snap, rt.SubjectID("uc")), ux, ux, ux], dtype=np.uint32)
    out, begin, count, needed = hl.path_ids_raw(roots, targets, 0)  # count only
    assert needed == 8 and count.tolist() == [4, 0, 0, 0, 4]
    assert begin[0] == lookup.TRUNCATED and begin[4] == lookup.TRUNCATED and begin[2] == lookup.INVALID
    out, begin, count, needed = hl.path_ids_raw(roots, targets, 5)
    assert needed == 8 and begin[0] == 0 and begin[4] == lookup.TRUNCATED
    rows.assert_shortest(out[:4], top, ux)
    with pytest.raises(L.KetoError) as e:
        hl.path_ids(roots, targets)
    assert e.value.code == L.EINVAL
    keep = [0, 1, 3, 4]
    got = hl.path_ids(roots[keep], targets[keep])
    assert [len(p) for p in got] == [4, 0, 0, 4]
