"""Reverse lookup on the host (ketogpu_snapshot_lookup, _type, _node): lookup(t, T) lists the
expandable nodes r of type T with SubjectIsAllowed(r, t).  Pinned against the CPU oracle as
full truth tables on random tables (wildcard subject sets and page poisoning included) and on
the RBAC shape; no GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup, synth
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import randgraph


@pytest.mark.parametrize("seed,n_rows,n_obj,page_size,poison", LC.TABLES)
def test_truth_table_matches_oracle(seed, n_rows, n_obj, page_size, poison):
    namespaces, rows, snap = LC.table(seed, n_rows, n_obj, page_size, poison)
    st = snap.stats()
    assert st["num_ambiguous_nodes"] == 0
    n, nx = st["num_nodes"], st["num_expandable"]
    orc = randgraph.oracle_store(namespaces, rows, page_size)
    roots = [snap.describe(r) for r in range(nx)]
    assert all(isinstance(r, rt.SubjectSet) for r in roots)
    subjects = [snap.describe(t).to_dict() for t in range(n)]
    reqs = [(r.namespace, r.object, r.relation, s) for s in subjects for r in roots]
    want = np.asarray(orc.check_batch(reqs, nthreads=4)).reshape(n, nx)
    sizes = []
    for t in range(n):
        got = np.zeros(nx, dtype=bool)
        ids = lookup.host_lookup(snap, t, lookup.TYPE_ANY)
        assert (np.diff(ids.astype(np.int64)) > 0).all()  # ascending, no duplicates
        got[ids] = True
        assert (got == want[t]).all(), (t, subjects[t], np.nonzero(got != want[t])[0][:5])
        sizes.append(len(ids))
    assert max(sizes) > (100 if seed == 31 else 3)  # the tables are not vacuous


@pytest.mark.parametrize("seed,n_rows,n_obj,page_size,poison", LC.TABLES)
def test_type_filter_is_the_any_list_restricted(seed, n_rows, n_obj, page_size, poison):
    namespaces, rows, snap = LC.table(seed, n_rows, n_obj, page_size, poison)
    st = snap.stats()
    info = [snap.node_info(r) for r in range(st["num_expandable"])]
    pairs = sorted({(ns, r[2]) for ns, _ in namespaces for r in rows})
    types = {p: snap.type_id(*p) for p in pairs}
    used = {p: t for p, t in types.items() if t != lookup.TYPE_NONE}
    assert len(used) >= 3 and len(set(used.values())) == len(used)
    wild = [i for i, d in enumerate(info) if d["id"] == "" or d["rel"] == ""]
    assert wild, "the table has wildcard subject-set nodes"
    # a wildcard node's type is its own: no (namespace, relation) pair resolves to it
    assert not {info[i]["type"] for i in wild} & set(used.values())
    assert snap.type_id("unknown", "r0") == lookup.TYPE_NONE
    assert snap.type_id(namespaces[0][0], "no such relation") == lookup.TYPE_NONE
    assert snap.type_id(namespaces[0][0], "") == lookup.TYPE_NONE
    seen_typed = 0
    for t in range(st["num_nodes"]):
        every = lookup.host_lookup(snap, t, lookup.TYPE_ANY)
        assert len(lookup.host_lookup(snap, t, lookup.TYPE_NONE)) == 0
        for (ns, rel), ty in used.items():
            want = [r for r in every if info[r]["ns"] == ns and info[r]["rel"] == rel and info[r]["id"] != ""]
            got = lookup.host_lookup(snap, t, ty)
            assert list(got) == want, (t, ns, rel)
            seen_typed += len(want)
    assert seen_typed > 50


@pytest.mark.slow
def test_rbac_list_objects_match_oracle():
    w = synth.rbac(users=20000, groups=2000, docs=4000, tuples=150000, checks=6000, seed=41)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    orc = randgraph.oracle_store_columns(w.namespaces, w.columns)
    users = [f"u{u}" for u in sorted(set(int(x) for x in w.chk_user[w.chk_pos != 0]))[:30]]
    assert len(users) == 30
    docs = [f"d{i}" for i in range(4000)]
    groups = [f"g{i}" for i in range(2000)]
    reqs = [("docs", d, "viewer", {"subject_id": u}) for u in users for d in docs]
    reqs += [("groups", g, "member", {"subject_id": u}) for u in users for g in groups]
    want = np.asarray(orc.check_batch(reqs, nthreads=8))
    wd = want[:30 * 4000].reshape(30, 4000)
    wg = want[30 * 4000:].reshape(30, 2000)
    sizes = []
    for k, u in enumerate(users):
        got = lookup.host_list_objects(snap, "docs", "viewer", rt.SubjectID(u))
        assert got == sorted(d for d, a in zip(docs, wd[k]) if a), u
        gotg = lookup.host_list_objects(snap, "groups", "member", rt.SubjectID(u))
        assert gotg == sorted(g for g, a in zip(groups, wg[k]) if a), u
        sizes.append(len(got))
    assert max(sizes) > 50
    assert lookup.host_list_objects(snap, "docs", "viewer", rt.SubjectID("nobody")) == []
    assert lookup.host_list_objects(snap, "nowhere", "viewer", rt.SubjectID(users[0])) == []
    assert lookup.host_list_objects(snap, "docs", "member", rt.SubjectID(users[0])) == []  # an unused pair


def test_ambiguous_keys_are_refused():
    namespaces, rows = randgraph.make_graph(23, n_rows=200, poison=True, collide=True)
    snap = Snapshot.from_rows(namespaces, rows, page_size=3, sort=True)
    assert snap.stats()["num_ambiguous_nodes"] > 0
    with pytest.raises(L.KetoError) as e:
        lookup.host_lookup(snap, 0)
    assert e.value.code == L.EINVAL


def test_describe_and_lookup_reject_ids_outside_the_snapshot():
    _, _, snap = LC.table(*LC.TABLES[1])
    n = snap.stats()["num_nodes"]
    snap.describe(n - 1)
    for bad in (n, n + 7, 0xFFFFFFFE):
        with pytest.raises(L.KetoError) as e:
            snap.describe(bad)
        assert e.value.code == L.EINVAL
        with pytest.raises(L.KetoError) as e:
            lookup.host_lookup(snap, bad)
        assert e.value.code == L.EINVAL
    assert len(lookup.host_lookup(snap, L.NODE_NONE)) == 0  # a subject no tuple names


def test_structure_cases_on_the_host():
    snap = Snapshot.from_rows(LC.NS1, LC.structure_rows())
    tgt = lambda s: int(lookup.resolve_subjects(snap, [s])[0])
    assert len(lookup.host_lookup(snap, tgt(rt.SubjectID("uc")))) == 3000  # no depth cutoff (R2)
    for name in ("ya", "yb", "self"):  # t is listed when a cycle leads back to it
        t = tgt(rt.SubjectSet("n", name, "member"))
        assert t in lookup.host_lookup(snap, t)
    t = tgt(rt.SubjectSet("n", "g0", "member"))
    assert t not in lookup.host_lookup(snap, t)
    names = lambda u: sorted(snap.describe(v).object for v in lookup.host_lookup(snap, tgt(rt.SubjectID(u))))
    assert names("ux") == ["g0", "g1", "g2", "top"]  # the diamond: top once
    assert len(names("u65")) == 65 and len(names("u129")) == 129
    assert len(lookup.host_lookup(snap, tgt(rt.SubjectSet("n", "lonely", "view")))) == 0
    for t in range(0, snap.stats()["num_nodes"], 97):
        assert (lookup.host_lookup(snap, t) == LC.closure(snap, t)).all()


def test_written_row_shows_in_the_next_lookup_and_placeholders_never_do():
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
    objs = lambda u: lookup.host_list_objects(snap, "n", "view", rt.SubjectID(u))
    assert objs("alice") == ["doc1"] and objs("bob") == ["doc2", "doc3"]
    for t in range(st["num_nodes"]):
        if t not in placeholders:
            assert not set(lookup.host_lookup(snap, t)) & set(placeholders)
    res = snap.write([LC.sid("h", "member", "alice")])
    assert res["applied"], res
    assert objs("alice") == ["doc1", "doc2"]
    res = snap.write([LC.sid("h", "member", "carol")])  # a new subject: a reserved id
    assert res["applied"] and res["new_nodes"] == 1, res
    assert objs("carol") == ["doc2"]
    assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]
    assert objs("alice") == ["doc2"]
    for t in range(snap.stats()["num_nodes"]):
        if t not in placeholders:
            assert not set(lookup.host_lookup(snap, t)) & set(placeholders)
