"""The CPU twins of the paged list calls (lookup.HostLookup / lookup.HostSubjects): pages are
slices of the ascending host lists, tokens are the decimal next lower bound.  No GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC

ANY = lookup.TYPE_ANY


def graphs():
    for case in LC.TABLES:
        yield f"seed{case[0]}", LC.table(*case)[2]
    yield "structure", Snapshot.from_rows(LC.NS1, SC.structure_rows())


def pages_of(raw, ids, limit):
    """walk one raw method to the end -> the concatenated lists, with the contract checked"""
    ids = np.asarray(ids, dtype=np.uint32)
    lo = np.zeros(len(ids), dtype=np.uint32)
    acc = [[] for _ in ids]
    active = np.arange(len(ids))
    while len(active):
        out, ret, cnt, rem = raw(ids[active], lo[active], ANY, limit)
        assert out.shape == (len(active), limit)
        for j, i in enumerate(active):
            k = int(ret[j])
            assert k == min(limit, int(rem[j])) and int(rem[j]) + len(acc[i]) == int(cnt[j])
            acc[i].extend(int(v) for v in out[j, :k])
            if k:
                lo[i] = int(out[j, k - 1]) + 1
        active = active[rem > ret]
    return [np.array(a, dtype=np.uint32) for a in acc]


@pytest.mark.parametrize("limit", [1, 7, 64, 4096])
def test_host_pages_are_slices_of_the_host_lists(limit):
    for name, snap in graphs():
        st = snap.stats()
        step = 1 if limit > 1 else 37  # (limit 1: a sample of the roots)
        if name == "structure":  # the chains: lists of up to 3000 members, a sample of the roots
            if limit < 64:
                continue
            step = 97
        for twin, raw, host, universe in (
                (lookup.HostLookup(snap), "lookup_page_raw", lookup.host_lookup, st["num_nodes"]),
                (lookup.HostSubjects(snap), "subject_page_raw", lookup.host_subjects, st["num_expandable"])):
            ids = np.arange(0, universe, step, dtype=np.uint32)
            got = pages_of(getattr(twin, raw), ids, limit)
            for r, g in zip(ids, got):
                assert np.array_equal(g, host(snap, int(r), ANY)), (name, raw, int(r))


def test_from_and_bad_ids():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    n = snap.stats()["num_nodes"]
    r = int(lookup.resolve_roots(snap, [("n", "f129", "view")])[0])
    w = lookup.host_subjects(snap, r, ANY)
    hs = lookup.HostSubjects(snap)
    ids = np.array([r, r, r, r, L.NODE_NONE, n, 0xFFFFFFFE], dtype=np.uint32)
    lo = np.array([0, int(w[10]), int(w[-1]) + 1, 0xFFFFFFFF, 0, 0, 0], dtype=np.uint32)
    out, ret, cnt, rem = hs.subject_page_raw(ids, lo, ANY, 20)
    assert list(ret) == [20, 20, 0, 0, 0, lookup.PAGE_INVALID, lookup.PAGE_INVALID]
    assert list(cnt) == [129] * 4 + [0] * 3 and list(rem) == [129, 119, 0, 0, 0, 0, 0]
    assert np.array_equal(out[0, :20], w[:20]) and np.array_equal(out[1, :20], w[10:30])
    same = hs.subject_page_raw(ids[:1], None, ANY, 20)
    assert np.array_equal(same[0][0], out[0]) and same[2][0] == 129
    hl = lookup.HostLookup(snap)
    out, ret, cnt, rem = hl.lookup_page_raw(np.array([n, L.NODE_NONE], dtype=np.uint32), None, ANY, 5)
    assert list(ret) == [lookup.PAGE_INVALID, 0] and not cnt.any() and not rem.any()


def test_tokens():
    assert lookup.parse_page_token("") == 0
    for v in (0, 5, 4294967295):
        assert lookup.parse_page_token(str(v)) == v
    assert lookup.parse_page_token("0000000017") == 17
    for bad in ("x", "-1", "4294967296", " 5", "5 ", "+5", "1e3", "12345678901", "٣", None, 5):
        with pytest.raises(L.KetoError) as e:
            lookup.parse_page_token(bad)
        assert e.value.code == L.EINVAL, bad
    ids = np.array([3, 9, 12], dtype=np.uint32)
    assert lookup.next_page_token(ids, 3, 3) == "" and lookup.next_page_token(ids, 0, 0) == ""
    assert lookup.next_page_token(ids, 2, 5) == "10" and lookup.next_page_token(ids, 3, 4) == "13"


def test_token_round_trips_by_name():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    hs, hl = lookup.HostSubjects(snap), lookup.HostLookup(snap)
    full = lookup.host_list_subjects(snap, "n", "f129", "view")
    assert len(full) == 129
    got, tok, n_pages = [], "", 0
    while True:
        items, tok, total = hs.list_subjects_page("n", "f129", "view", page_size=50, page_token=tok)
        assert total == 129 and len(items) == (50 if tok else 29)
        got += items
        n_pages += 1
        if not tok:
            break
        assert lookup.parse_page_token(tok) > 0
    assert n_pages == 3 and sorted(got, key=lambda s: s.id) == full and len(set(got)) == 129
    objs = lookup.host_list_objects(snap, "n", "view", rt.SubjectID("u65"))
    a, tok, total = hl.list_objects_page("n", "view", rt.SubjectID("u65"), page_size=64)
    b, end, _ = hl.list_objects_page("n", "view", rt.SubjectID("u65"), page_size=64, page_token=tok)
    assert total == 65 and len(a) == 64 and len(b) == 1 and end == "" and sorted(a + b) == objs
    # exactly page_size members: one page, no token
    assert hl.list_objects_page("n", "view", rt.SubjectID("u65"), page_size=65)[1] == ""
    # a token past every id is legal
    assert hs.list_subjects_page("n", "f129", "view", page_token="4294967295") == ([], "", 129)
    # kinds: the chain's subject sets; the batch form is the single form, request by request
    sets = hs.list_subjects_page("n", "c2999", "member", kind=("n", "member"), page_size=10)
    assert sets[2] == 2999 and all(isinstance(s, rt.SubjectSet) for s in sets[0])
    assert hs.list_subjects_page("n", "c2999", "member", kind="ids") == ([rt.SubjectID("uc")], "", 1)
    reqs = [(("n", "f129", "view"), ""), (("n", "f65", "view"), "17"), (("n", "f129", "view"), tok)]
    assert hs.list_subjects_page_batch(reqs, "ids", 50) == [
        hs.list_subjects_page(*r, kind="ids", page_size=50, page_token=t) for r, t in reqs]
    users = [(rt.SubjectID("u65"), ""), (rt.SubjectID("u129"), "40"), (rt.SubjectID("nobody"), "")]
    assert hl.list_objects_page_batch("n", "view", users, 50) == [
        hl.list_objects_page("n", "view", u, 50, t) for u, t in users]


def test_bad_arguments_and_empty_answers():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    hs, hl = lookup.HostSubjects(snap), lookup.HostLookup(snap)
    u = rt.SubjectID("u65")
    for tok in ("x", "-1", "4294967296", " 5"):
        for call in (lambda: hs.list_subjects_page("n", "f65", "view", page_token=tok),
                     lambda: hl.list_objects_page("n", "view", u, page_token=tok)):
            with pytest.raises(L.KetoError) as e:
                call()
            assert e.value.code == L.EINVAL
    for size in (0, 65537, -1):
        for call in (lambda: hs.list_subjects_page("n", "f65", "view", page_size=size),
                     lambda: hl.list_objects_page("n", "view", u, page_size=size),
                     lambda: hs.subject_page_raw([0], None, ANY, size),
                     lambda: hl.lookup_page_raw([0], None, ANY, size)):
            with pytest.raises(L.KetoError) as e:
                call()
            assert e.value.code == L.EINVAL
    assert len(hs.list_subjects_page("n", "f65", "view", page_size=65536)[0]) == 65
    # an unknown namespace, an unused pair, a subject no tuple names, an object no tuple names
    assert hl.list_objects_page("nowhere", "view", u) == ([], "", 0)
    assert hl.list_objects_page("n", "no such relation", u) == ([], "", 0)
    assert hl.list_objects_page("n", "view", rt.SubjectID("nobody")) == ([], "", 0)
    assert hs.list_subjects_page("nowhere", "f65", "view") == ([], "", 0)
    assert hs.list_subjects_page("n", "no such doc", "view") == ([], "", 0)
    assert hs.list_subjects_page("n", "f65", "view", kind=("n", "no such relation")) == ([], "", 0)


def test_wildcard_root_without_a_node():
    _, rows, snap = LC.table(*LC.TABLES[1])
    obj, rel = rows[0][1], rows[0][2]
    assert obj and rel
    with pytest.raises(L.KetoError) as e:  # no namespace is named "": the query has no node of its own
        lookup.HostSubjects(snap).list_subjects_page("", obj, rel)
    assert e.value.code == L.EINVAL
