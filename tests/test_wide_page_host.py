"""The wide paged and depth calls' surface without a GPU: the library exports them, the keyword
`wide` exists on every call that takes it and is judged before any device is touched, the CPU
twins accept and ignore it, and the list routes of the REST handler mirror take wide=true."""
import ctypes as C
import inspect

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC

SYMBOLS = ["ketogpu_subjects_ids_depth_wide", "ketogpu_lookup_ids_depth_wide", "ketogpu_subjects_page_wide",
           "ketogpu_lookup_page_wide", "ketogpu_wide_clear_tile_ids"]

LOOKUP_METHODS = ["lookup_page_raw", "lookup_depth_raw", "lookup_depth_page_raw", "list_objects_page",
                  "list_objects_page_batch", "list_objects_depth_batch"]
SUBJECT_METHODS = ["subject_page_raw", "subject_depth_raw", "subject_depth_page_raw", "list_subjects_page",
                   "list_subjects_page_batch", "list_subjects_depth_batch"]


def test_the_library_exports_the_wide_page_calls():
    lib = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    abi = L.lib()
    T = abi.ketogpu_wide_clear_tile_ids()
    assert T >= 32 and T % 32 == 0 and T < L.PAGE_LIMIT_MAX  # whole bitmap words; a page can span tiles
    needed = C.c_uint64()
    u32, u64 = np.zeros(4, dtype=np.uint32).ctypes.data, np.zeros(4, dtype=np.uint64).ctypes.data
    for side in ("subjects", "lookup"):  # a null handle is refused, not followed
        page = getattr(abi, f"ketogpu_{side}_page_wide")
        ids = getattr(abi, f"ketogpu_{side}_ids_depth_wide")
        assert page(None, None, None, None, 0, 0, 4, None, None, None, None, None) == L.EINVAL
        assert page(None, u32, None, None, 1, 0, 4, u32, u32, u64, u64, None) == L.EINVAL
        assert ids(None, None, None, 0, 0, None, 0, None, None, None, C.byref(needed)) == L.EINVAL
    assert [n for n, _ in L.WideStats._fields_] == [  # the struct the new calls count in keeps its layout
        "requests", "tier1_requests", "wide_requests", "wide_rounds", "levels", "items", "ids_produced",
        "truncated_lists", "slots", "chunk", "last_call_ms"]


@pytest.mark.parametrize("cls,names", [(lookup.Lookup, LOOKUP_METHODS), (lookup.HostLookup, LOOKUP_METHODS),
                                       (lookup.Subjects, SUBJECT_METHODS), (lookup.HostSubjects, SUBJECT_METHODS)],
                         ids=["Lookup", "HostLookup", "Subjects", "HostSubjects"])
def test_the_keyword_exists_and_defaults_to_false(cls, names):
    for name in names:
        p = inspect.signature(getattr(cls, name)).parameters
        assert "wide" in p and p["wide"].default is False, (cls.__name__, name)
    for name in ("ListObjects", "list_objects_batch", "ListSubjects", "list_subjects_batch"):
        if hasattr(cls, name):  # the full-list calls keep theirs
            assert inspect.signature(getattr(cls, name)).parameters["wide"].default is False


def snapshot():
    return Snapshot.from_rows(LC.NS1, SC.structure_rows())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_wide_does_not_take_with_via(device):
    snap = snapshot()
    # (the keyword is judged first: a device class without a handle never reaches the library)
    sj = object.__new__(lookup.Subjects) if device else lookup.HostSubjects(snap)
    lk = object.__new__(lookup.Lookup) if device else lookup.HostLookup(snap)
    sj.snapshot = lk.snapshot = snap
    user, doc = rt.SubjectID("ux"), ("n", "top", "view")
    for kw in ({}, {"max_depth": 2}):
        with pytest.raises(ValueError):
            sj.list_subjects_page(*doc, wide=True, with_via=True, **kw)
        with pytest.raises(ValueError):
            sj.list_subjects_page_batch([(doc, "")], wide=True, with_via=True, **kw)
        with pytest.raises(ValueError):
            lk.list_objects_page("n", "view", user, wide=True, with_via=True, **kw)
        with pytest.raises(ValueError):
            lk.list_objects_page_batch("n", "view", [(user, "")], wide=True, with_via=True, **kw)
    for kw in ({"max_depth": 1}, {"with_via": True}):  # the full-list calls keep their rule
        with pytest.raises(ValueError):
            sj.list_subjects_batch([doc], wide=True, **kw)
        with pytest.raises(ValueError):
            lk.list_objects_batch("n", "view", [user], wide=True, **kw)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_cpu_twins_answer_the_same_with_and_without_wide():
    snap = snapshot()
    st = snap.stats()
    hs, hl = lookup.HostSubjects(snap), lookup.HostLookup(snap)
    roots = np.array(list(range(0, st["num_expandable"], 7)) + [L.NODE_NONE, st["num_nodes"], st["num_nodes"] - 1],
                     dtype=np.uint32)
    targets = np.array(list(range(0, st["num_nodes"], 7)) + [L.NODE_NONE, st["num_nodes"]], dtype=np.uint32)
    lo_r, lo_t = (roots // 2).astype(np.uint32), (targets // 3).astype(np.uint32)
    for depth in (None, 1, 2, (np.arange(len(roots)) % 4).astype(np.uint32)):
        for f in (lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID):
            assert same(hs.subject_depth_page_raw(roots, depth, lo_r, f, 9),
                        hs.subject_depth_page_raw(roots, depth, lo_r, f, 9, wide=True))
            a, b = hs.subject_depth_raw(roots, depth, f, 50), hs.subject_depth_raw(roots, depth, f, 50, wide=True)
            assert same(a[:4], b[:4]) and a[4] == b[4]
    for depth in (None, 1, 3, (np.arange(len(targets)) % 4).astype(np.uint32)):
        assert same(hl.lookup_depth_page_raw(targets, depth, lo_t, lookup.TYPE_ANY, 9),
                    hl.lookup_depth_page_raw(targets, depth, lo_t, lookup.TYPE_ANY, 9, wide=True))
        a = hl.lookup_depth_raw(targets, depth, lookup.TYPE_ANY, 50)
        b = hl.lookup_depth_raw(targets, depth, lookup.TYPE_ANY, 50, wide=True)
        assert same(a[:4], b[:4]) and a[4] == b[4]
    assert same(hs.subject_page_raw(roots, lo_r, lookup.TYPE_ANY, 5),
                hs.subject_page_raw(roots, lo_r, lookup.TYPE_ANY, 5, wide=True))
    assert same(hl.lookup_page_raw(targets, lo_t, lookup.TYPE_ANY, 5),
                hl.lookup_page_raw(targets, lo_t, lookup.TYPE_ANY, 5, wide=True))
    # a page without a limit is the plain page, whichever way it is asked for
    assert same(hs.subject_page_raw(roots, lo_r, lookup.TYPE_ANY, 5, wide=True),
                hs.subject_depth_page_raw(roots, None, lo_r, lookup.TYPE_ANY, 5, wide=True)[:4])
    docs = [("n", "top", "view"), ("n", "f129", "view"), ("n", "c2999", "member"), ("n", "no such doc", "view")]
    users = [rt.SubjectID("ux"), rt.SubjectID("u129"), rt.SubjectID("uc"), rt.SubjectID("nobody")]
    for kw in ({}, {"max_depth": 2}, {"max_depth": [1, 2, 3, 4]}):
        plain = hs.list_subjects_page_batch([(d, "") for d in docs], "any", 20, **kw)
        assert plain == hs.list_subjects_page_batch([(d, "") for d in docs], "any", 20, wide=True, **kw)
        if not isinstance(kw.get("max_depth"), list):
            assert plain[1] == hs.list_subjects_page(*docs[1], "any", 20, wide=True, **kw)
            assert plain[1] == hs.list_subjects_page(*docs[1], "any", 20, **kw)
        assert len(plain[0]) == (4 if kw else 3)
        plain = hl.list_objects_page_batch("n", "member", [(u, "") for u in users], 20, **kw)
        assert plain == hl.list_objects_page_batch("n", "member", [(u, "") for u in users], 20, wide=True, **kw)
        assert len(plain[0]) == (4 if kw else 3)
    for depth in (1, 2, [1, 2, 3, 4]):
        assert hs.list_subjects_depth_batch(docs, depth, "any") == hs.list_subjects_depth_batch(docs, depth, "any",
                                                                                                 wide=True)
        assert hl.list_objects_depth_batch("n", "member", users, depth) == \
            hl.list_objects_depth_batch("n", "member", users, depth, wide=True)
    lists, complete = hl.list_objects_depth_batch("n", "member", users, 2, wide=True)
    assert lists[0] == ["g0", "g1", "g2"] and complete == [False, True, False, True]


@pytest.fixture(scope="module")
def handler():
    snap = snapshot()
    return Handler(None, expand.Engine(snap), lookup.HostLookup(snap), lookup.HostSubjects(snap))


def test_the_list_routes_take_wide(handler):
    base = "namespace=n&relation=member&subject_id=ux"
    for extra in ("", "&max-depth=1", "&max-depth=2", "&page_size=2", "&page_size=1&page_token=3"):
        plain = handler.get_list_objects(base + extra)
        assert plain[0] == 200 and handler.get_list_objects(base + extra + "&wide=true") == plain
        assert ("complete" in plain[1]) == ("max-depth" in extra)
    base = "namespace=n&object=top&relation=view&kind=any"
    for extra in ("", "&max-depth=1", "&max-depth=2", "&page_size=2"):
        plain = handler.get_list_subjects(base + extra)
        assert plain[0] == 200 and handler.get_list_subjects(base + extra + "&wide=true") == plain
        assert ("complete" in plain[1]) == ("max-depth" in extra)
    assert handler.get_list_subjects(base + "&max-depth=2&wide=true")[1]["complete"] is False


def test_wide_with_via_and_other_values_are_bad_requests(handler):
    objects = "namespace=n&relation=member&subject_id=ux"
    subjects = "namespace=n&object=top&relation=view"
    for get, base in ((handler.get_list_objects, objects), (handler.get_list_subjects, subjects)):
        for extra in ("&via=true&wide=true", "&wide=true&via=true&max-depth=2", "&wide=1", "&wide=false", "&wide=",
                      "&wide=TRUE"):
            code, body = get(base + extra)
            assert code == 400, extra
        assert get(base + "&via=true")[0] == 200  # each alone is served
        assert get(base + "&wide=true")[0] == 200
    none = Handler(None, None)
    assert none.get_list_objects(objects + "&wide=true")[0] == 404
