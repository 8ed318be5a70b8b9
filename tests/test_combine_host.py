"""The CPU twins of the combined listings (lookup.HostLookup / HostSubjects combine_*), checked
against the oracle directly, not against the host lists they are computed from: membership of
every candidate equals Check(.., a) op Check(.., b).  No GPU."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import combine_cases as CC
from tests import lookup_cases as LC
from tests import subjects_cases as SC

ANY, IDS, NONE = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID, L.NODE_NONE
LOGIC = {lookup.OP_AND: lambda x, y: x & y, lookup.OP_ANDNOT: lambda x, y: x & ~y, lookup.OP_OR: lambda x, y: x | y}


def as_mask(ids, size):
    got = np.zeros(size, dtype=bool)
    got[ids] = True
    assert len(ids) == got.sum() and (np.diff(ids.astype(np.int64)) > 0).all()  # ascending, no duplicates
    return got


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_operators_match_the_oracle(case):
    _, _, snap = LC.table(*case)
    check = SC.oracle_matrix(case)  # check[t][r] = Check(r, t)
    n, nx = check.shape
    a, b = CC.pair_sample(n, case[0])
    objects = lambda t: check[t] if t != NONE else np.zeros(nx, dtype=bool)  # per expandable r
    subjects = lambda r: check[:, r] if r < nx else np.zeros(n, dtype=bool)  # per node t; no row: nobody
    hl, hs = lookup.HostLookup(snap), lookup.HostSubjects(snap)
    nonempty = 0
    for op, name in CC.OP_NAMES.items():
        for k, ids in enumerate(hl.combine_ids(a, b, name)):
            want = LOGIC[op](objects(int(a[k])), objects(int(b[k])))
            assert (as_mask(ids, nx) == want).all(), ("lookup", name, int(a[k]), int(b[k]))
            nonempty += bool(len(ids))
        for k, ids in enumerate(hs.combine_ids(a, b, op)):
            want = LOGIC[op](subjects(int(a[k])), subjects(int(b[k])))
            assert (as_mask(ids, n) == want).all(), ("subjects", name, int(a[k]), int(b[k]))
            nonempty += bool(len(ids))
    assert nonempty > len(a)  # the sample is not vacuous


@pytest.mark.parametrize("case", LC.TABLES[:2], ids=lambda c: f"seed{c[0]}")
def test_filters_are_the_any_answer_restricted(case):
    _, _, snap = LC.table(*case)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    a, b = CC.pair_sample(n, case[0])
    pick = np.random.default_rng(case[0]).choice(len(a), 150, replace=False)
    a, b = a[pick], b[pick]
    types = np.array([snap.node_info(t)["type"] for t in range(nx)], dtype=np.uint64)
    classes = np.array([snap.subject_class(t) for t in range(n)], dtype=np.uint64)
    hl, hs = lookup.HostLookup(snap), lookup.HostSubjects(snap)
    for op in CC.OP_IDS:
        every_o, every_s = hl.combine_ids(a, b, op), hs.combine_ids(a, b, op)
        for ty in sorted(set(types.tolist()))[:3]:
            for ids, every in zip(hl.combine_ids(a, b, op, int(ty)), every_o):
                assert np.array_equal(ids, every[types[every] == ty])
        for cls in [IDS] + sorted(set(types.tolist()))[:2]:
            for ids, every in zip(hs.combine_ids(a, b, op, int(cls)), every_s):
                assert np.array_equal(ids, every[classes[every] == cls])
        for nothing in (lookup.TYPE_NONE, lookup.CLASS_UNTYPED_SET):
            assert not any(len(x) for x in hs.combine_ids(a, b, op, nothing))
        assert not any(len(x) for x in hl.combine_ids(a, b, op, lookup.TYPE_NONE))


@pytest.fixture(scope="module")
def snap():
    return Snapshot.from_rows(LC.NS1, SC.structure_rows())


@pytest.mark.parametrize("page_size", [1, 7, 100])
def test_pages_walk_to_the_sorted_full_list(snap, page_size):
    hl, hs = lookup.HostLookup(snap), lookup.HostSubjects(snap)
    ua, ub = rt.SubjectID("u129"), rt.SubjectID("u65")
    da, db = ("n", "f129", "view"), ("n", "f65", "view")
    for op, size in (("or", 194), ("andnot", 129), ("and", 0)):
        full = hl.ListObjectsCombined("n", "view", ua, ub, op)
        assert len(full) == size and full == sorted(full)
        subs = hs.ListSubjectsCombined(da, db, op)
        assert len(subs) == size
        for walk, want in ((lambda tok: hl.list_objects_combined_page("n", "view", ua, ub, op, page_size, tok), full),
                           (lambda tok: hs.list_subjects_combined_page(da, db, op, "ids", page_size, tok),
                            [s.id for s in subs])):
            items, token, pages = [], "", 0
            while True:
                page, token, total = walk(token)
                assert total == size and len(page) <= page_size
                items += [getattr(p, "id", p) for p in page]
                pages += 1
                if token == "":  # the last token
                    break
            assert sorted(items) == want and pages == max(1, -(-size // page_size))


def test_layout_and_degenerate_pairs(snap):
    n = snap.stats()["num_nodes"]
    hl, hs = lookup.HostLookup(snap), lookup.HostSubjects(snap)
    x = CC.LookupSide.node(snap, "u129")
    a, b = np.array([x, x, NONE, n + 5, NONE], dtype=np.uint32), np.array([x, NONE, x, x, NONE], dtype=np.uint32)
    out, begin, count, needed = hl.combine_ids_raw(a, b, "or", ANY, 258)
    assert needed == 387 and list(count) == [129, 129, 129, 0, 0] and begin[3] == lookup.INVALID
    assert list(begin[:3]) == [0, 129, lookup.TRUNCATED]  # every list reserves, written or not
    out, begin, count, needed = hl.combine_ids_raw(a, b, "and", ANY, 0)
    assert needed == 129 and list(count) == [129, 0, 0, 0, 0] and begin[0] == lookup.TRUNCATED
    out, begin, count, needed = hl.combine_ids_raw(a, b, "andnot", ANY, 200)
    assert needed == 129 and list(count) == [0, 129, 0, 0, 0]
    out, returned, count, remaining = hl.combine_page_raw(a, b, lookup.OP_OR, None, ANY, 100)
    assert list(returned) == [100, 100, 100, lookup.PAGE_INVALID, 0] and list(remaining[:3]) == [129] * 3
    with pytest.raises(L.KetoError) as e:
        hl.combine_ids(a, b, "or")  # an id outside the snapshot
    assert e.value.code == L.EINVAL
    r = CC.SubjectsSide.node(snap, "f65")
    assert r < snap.stats()["num_expandable"] <= x  # x: a never-expanded root there
    assert [len(v) for v in hs.combine_ids([r, r, x, r], [x, x, r, NONE], "or")] == [65, 65, 65, 65]
    assert [len(v) for v in hs.combine_ids([r, x], [x, r], "and")] == [0, 0]
    assert [len(v) for v in hs.combine_ids([r, x], [x, r], "andnot")] == [65, 0]
    for h in (hl, hs):
        for op in (3, "xor", "AND"):
            with pytest.raises(L.KetoError) as e:
                h.combine_ids_raw(a[:1], b[:1], op, ANY, 0)
            assert e.value.code == L.EINVAL
        with pytest.raises(L.KetoError):
            h.combine_ids_raw(a, b[:2], "or", ANY, 0)
    assert (lookup.OP_AND, lookup.OP_ANDNOT, lookup.OP_OR) == (0, 1, 2)
    assert [lookup.op_id(s) for s in ("and", "andnot", "or")] == [0, 1, 2]
