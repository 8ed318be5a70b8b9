"""Subject listing on the host (ketogpu_snapshot_subjects, _subject_class): subjects(r, C) lists
the nodes t of class C with SubjectIsAllowed(r, t).  Pinned against the CPU oracle as full truth
tables on random tables (wildcard subject sets and page poisoning included), against the
reverse lookup as its transpose, and on structure cases; no GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import randgraph
from tests import subjects_cases as SC

ANY, IDS, UNTYPED = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID, lookup.CLASS_UNTYPED_SET


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_table_matches_oracle(case):
    _, _, snap = LC.table(*case)
    want = SC.oracle_matrix(case)
    n, nx = want.shape
    sizes = []
    for r in range(nx):
        ids = lookup.host_subjects(snap, r, ANY)
        assert (np.diff(ids.astype(np.int64)) > 0).all()  # ascending, no duplicates
        got = np.zeros(n, dtype=bool)
        got[ids] = True
        assert (got == want[:, r]).all(), (r, snap.describe(r), np.nonzero(got != want[:, r])[0][:5])
        sizes.append(len(ids))
    print("largest forward closure:", max(sizes))
    assert max(sizes) > 50  # the tables are not vacuous


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_class_filter_is_the_any_list_restricted(case):
    namespaces, rows, snap = LC.table(*case)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    info = [snap.node_info(t) for t in range(n)]
    cls = [snap.subject_class(t) for t in range(n)]
    for t in range(n):  # the class extends the type: equal below Nx, never NONE from there on
        if t < nx:
            assert cls[t] == info[t]["type"] != lookup.TYPE_NONE
        elif info[t]["kind"] == L.SUBJECT_ID:
            assert cls[t] == IDS
        else:
            assert cls[t] not in (IDS, lookup.TYPE_NONE, ANY)
    pairs = sorted({(ns, r[2]) for ns, _ in namespaces for r in rows})
    used = {p: snap.type_id(*p) for p in pairs}
    used = {p: t for p, t in used.items() if t != lookup.TYPE_NONE}
    assert len(used) >= 3
    leaf_sets = [t for t in range(nx, n) if info[t]["kind"] == L.SUBJECT_SET]
    print("non-expandable subject-set nodes:", len(leaf_sets))
    assert leaf_sets
    typed = lambda t, ns, rel: (info[t]["kind"] == L.SUBJECT_SET and info[t]["ns"] == ns and info[t]["rel"] == rel
                                and info[t]["id"] != "")
    # a never-expanded subject set with a concrete pair that some expandable node defines has
    # that pair's type; any other (a wildcard, a pair only named as a subject) is UNTYPED
    # unless it shares a wildcard type
    wild_types = {info[r]["type"] for r in range(nx) if info[r]["id"] == "" or info[r]["rel"] == ""}
    for t in leaf_sets:
        match = [ty for (ns, rel), ty in used.items() if typed(t, ns, rel)]
        if match:
            assert cls[t] == match[0]
        else:
            assert cls[t] == UNTYPED or cls[t] in wild_types
    untyped = {t for t in leaf_sets if cls[t] == UNTYPED}
    leaf_typed = leaf_untyped = 0
    for r in range(nx):
        every = lookup.host_subjects(snap, r, ANY)
        assert len(lookup.host_subjects(snap, r, lookup.TYPE_NONE)) == 0
        assert len(lookup.host_subjects(snap, r, UNTYPED)) == 0  # UNTYPED as a filter lists nothing
        assert list(lookup.host_subjects(snap, r, IDS)) == [t for t in every if info[t]["kind"] == L.SUBJECT_ID]
        for (ns, rel), ty in used.items():
            want = [t for t in every if typed(t, ns, rel)]
            assert list(lookup.host_subjects(snap, r, ty)) == want, (r, ns, rel)
            leaf_typed += sum(t >= nx for t in want)
            assert not untyped & set(want)
        leaf_untyped += len(untyped & set(int(t) for t in every))
    assert leaf_typed > 0  # never-expanded subject sets are listed under a concrete type
    # the UNTYPED rule: exercised (listed under ANY and under no concrete class), or no node has the class
    assert leaf_untyped > 0 or not untyped
    print("untyped nodes:", len(untyped), "listings of them under ANY:", leaf_untyped)


def test_subjects_is_the_transpose_of_lookup():
    _, _, snap = LC.table(*LC.TABLES[0])
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    fwd = np.zeros((n, nx), dtype=bool)
    rev = np.zeros((n, nx), dtype=bool)
    for r in range(nx):
        fwd[lookup.host_subjects(snap, r, ANY), r] = True
    for t in range(n):
        rev[t, lookup.host_lookup(snap, t, ANY)] = True
    assert fwd.any() and (fwd == rev).all()


def test_structure_cases_on_the_host():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    root = lambda obj, rel: int(lookup.resolve_roots(snap, [("n", obj, rel)])[0])
    assert len(lookup.host_subjects(snap, root("c2999", "member"))) == 3000  # no depth cutoff (R2)
    for name in ("ya", "yb", "self"):  # r is listed when a cycle leads back to it
        r = root(name, "member")
        assert r in lookup.host_subjects(snap, r)
    r = root("g0", "member")
    assert r not in lookup.host_subjects(snap, r)
    names = lambda ids: sorted(getattr(s, "id", None) or s.object for s in map(snap.describe, ids))
    assert names(lookup.host_subjects(snap, root("top", "view"))) == ["g0", "g1", "g2", "ux"]  # the diamond: g0 once
    assert len(lookup.host_subjects(snap, root("f65", "view"), IDS)) == 65
    assert len(lookup.host_subjects(snap, root("f129", "view"), IDS)) == 129
    assert len(lookup.host_subjects(snap, root("two", "view"))) == 42
    assert len(lookup.host_subjects(snap, root("two", "view"), IDS)) == 40
    assert lookup.host_list_subjects(snap, "n", "top", "view") == [rt.SubjectID("ux")]
    assert lookup.host_list_subjects(snap, "n", "top", "view", "any") == [
        rt.SubjectID("ux")] + [rt.SubjectSet("n", g, "member") for g in ("g0", "g1", "g2")]
    assert lookup.host_list_subjects(snap, "n", "top", "view", ("n", "member")) == [
        rt.SubjectSet("n", g, "member") for g in ("g0", "g1", "g2")]
    assert lookup.host_list_subjects(snap, "n", "top", "view", ("n", "nothing")) == []
    assert lookup.host_list_subjects(snap, "nowhere", "top", "view") == []  # check says false there
    assert lookup.host_list_subjects(snap, "n", "nothing", "view") == []
    # roots without rows and the root no tuple matches: the empty list; ids outside: EINVAL
    assert nx < n
    for leaf in (nx, n - 1):
        assert len(lookup.host_subjects(snap, leaf)) == 0
    assert len(lookup.host_subjects(snap, L.NODE_NONE)) == 0
    for bad in (n, n + 7, 0xFFFFFFFE):
        with pytest.raises(L.KetoError) as e:
            lookup.host_subjects(snap, bad)
        assert e.value.code == L.EINVAL
        with pytest.raises(L.KetoError) as e:
            snap.subject_class(bad)
        assert e.value.code == L.EINVAL
    for r in list(range(0, nx, 97)) + [root("two", "view"), root("f129", "view")]:
        assert np.array_equal(lookup.host_subjects(snap, r), SC.forward_closure(snap, r))


def test_untyped_sets_are_listed_under_any_only():
    # ghost#owner is named as a subject, has no rows, and no expandable node has the pair
    # (n, owner); band#member has no rows either, but g#member defines its type
    rows = [LC.sset("doc", "view", "ghost", "owner"), LC.sset("doc", "view", "band", "member"),
            LC.sset("doc", "view", "g", "member"), LC.sid("g", "member", "alice")]
    snap = Snapshot.from_rows(LC.NS1, rows)
    nx = snap.stats()["num_expandable"]
    node = lambda s: int(lookup.resolve_subjects(snap, [s])[0])
    ghost, band, g = (node(rt.SubjectSet("n", o, r)) for o, r in (("ghost", "owner"), ("band", "member"),
                                                                  ("g", "member")))
    assert ghost >= nx and band >= nx and g < nx
    member = snap.type_id("n", "member")
    assert snap.type_id("n", "owner") == lookup.TYPE_NONE
    assert snap.subject_class(ghost) == UNTYPED
    assert snap.subject_class(band) == member == snap.subject_class(g)
    assert snap.node_info(band)["type"] == lookup.TYPE_NONE  # the reverse lookup's type is unchanged
    doc = int(lookup.resolve_roots(snap, [("n", "doc", "view")])[0])
    assert sorted(lookup.host_subjects(snap, doc, ANY)) == sorted([ghost, band, g, node(rt.SubjectID("alice"))])
    assert sorted(lookup.host_subjects(snap, doc, member)) == sorted([band, g])
    assert len(lookup.host_subjects(snap, doc, UNTYPED)) == 0
    assert lookup.host_list_subjects(snap, "n", "doc", "view", ("n", "owner")) == []
    assert rt.SubjectSet("n", "ghost", "owner") in lookup.host_list_subjects(snap, "n", "doc", "view", "any")


def test_dynamic_wildcard_roots_are_not_listed():
    _, rows, snap = LC.table(*LC.TABLES[1])
    obj, rel = rows[0][1], rows[0][2]
    assert obj and rel
    # no namespace is named "": a query over every namespace has no node of its own
    with pytest.raises(L.KetoError) as e:
        lookup.resolve_roots(snap, [("", obj, rel)])
    assert e.value.code == L.EINVAL
    with pytest.raises(L.KetoError) as e:
        lookup.host_list_subjects(snap, "", obj, rel)
    assert e.value.code == L.EINVAL
    assert lookup.resolve_roots(snap, [("", "no such object anywhere", rel)])[0] == L.NODE_NONE  # matches nothing
    with pytest.raises(ValueError):
        lookup.host_list_subjects(snap, "n", "o", "r", kind="users")


def test_ambiguous_keys_are_refused():
    namespaces, rows = randgraph.make_graph(23, n_rows=200, poison=True, collide=True)
    snap = Snapshot.from_rows(namespaces, rows, page_size=3, sort=True)
    assert snap.stats()["num_ambiguous_nodes"] > 0
    with pytest.raises(L.KetoError) as e:
        lookup.host_subjects(snap, 0)
    assert e.value.code == L.EINVAL


def test_written_row_shows_in_the_next_listing_and_placeholders_never_do():
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"),
            LC.sset("doc2", "view", "h", "member"), LC.sid("h", "member", "bob"), LC.sid("doc3", "view", "bob")]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    st = snap.stats()
    placeholders = []
    for v in range(st["num_nodes"]):
        try:
            snap.describe(v)
        except L.KetoError as e:
            assert e.code == L.EINVAL
            placeholders.append(v)
    assert len(placeholders) == 3
    assert all(snap.subject_class(v) == lookup.TYPE_NONE for v in placeholders)
    users = lambda d: [s.id for s in lookup.host_list_subjects(snap, "n", d, "view")]

    def no_placeholders():
        for r in range(snap.stats()["num_nodes"]):
            assert not set(lookup.host_subjects(snap, r)) & set(placeholders)

    assert users("doc1") == ["alice"] and users("doc2") == ["bob"] and users("doc3") == ["bob"]
    no_placeholders()
    res = snap.write([LC.sid("h", "member", "alice")])
    assert res["applied"], res
    assert users("doc2") == ["alice", "bob"]
    res = snap.write([LC.sid("h", "member", "carol")])  # a new subject: a reserved id
    assert res["applied"] and res["new_nodes"] == 1, res
    assert users("doc2") == ["alice", "bob", "carol"]
    assert snap.subject_class(snap.stats()["num_nodes"] - 1) == IDS
    assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]
    assert users("doc1") == [] and users("doc2") == ["alice", "bob", "carol"]
    no_placeholders()
