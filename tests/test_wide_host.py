"""The wide calls' surface without a GPU: the library exports them, the keyword `wide` is judged
before any device is touched, and the CPU twins accept and ignore it."""
import ctypes as C

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC

SYMBOLS = ["ketogpu_subjects_ids_wide", "ketogpu_lookup_ids_wide", "ketogpu_subjects_wide_stats_get",
           "ketogpu_lookup_wide_stats_get"]


def test_the_library_exports_the_wide_calls():
    lib = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert [n for n, _ in L.WideStats._fields_] == [
        "requests", "tier1_requests", "wide_requests", "wide_rounds", "levels", "items", "ids_produced",
        "truncated_lists", "slots", "chunk", "last_call_ms"]
    assert C.sizeof(L.WideStats) == 8 * 8 + 4 + 4 + 8
    st = L.WideStats()  # a null handle is refused, not followed
    assert L.lib().ketogpu_subjects_wide_stats_get(None, C.byref(st)) == L.EINVAL
    assert L.lib().ketogpu_lookup_wide_stats_get(None, C.byref(st)) == L.EINVAL
    needed = C.c_uint64()
    assert L.lib().ketogpu_subjects_ids_wide(None, None, 0, 0, None, 0, None, None, C.byref(needed)) == L.EINVAL
    assert L.lib().ketogpu_lookup_ids_wide(None, None, 0, 0, None, 0, None, None, C.byref(needed)) == L.EINVAL


def snapshot():
    return Snapshot.from_rows(LC.NS1, SC.fwd_split_rows("two", 42, "two_") + SC.fwd_star_rows("f65", 65, "f65_"))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_wide_takes_neither_max_depth_nor_with_via(device):
    snap = snapshot()
    # (the keyword is judged first: a device class without a handle never reaches the library)
    sj = object.__new__(lookup.Subjects) if device else lookup.HostSubjects(snap)
    lk = object.__new__(lookup.Lookup) if device else lookup.HostLookup(snap)
    sj.snapshot = lk.snapshot = snap
    user = rt.SubjectID("two_u0")
    for kw in ({"max_depth": 1}, {"with_via": True}, {"max_depth": 2, "with_via": True}):
        with pytest.raises(ValueError):
            sj.list_subjects_batch([("n", "two", "view")], wide=True, **kw)
        with pytest.raises(ValueError):
            sj.ListSubjects("n", "two", "view", wide=True, **kw)
        with pytest.raises(ValueError):
            lk.list_objects_batch("n", "view", [user], wide=True, **kw)
        with pytest.raises(ValueError):
            lk.ListObjects("n", "view", user, wide=True, **kw)


def test_cpu_twins_accept_and_ignore_wide():
    snap = snapshot()
    st = snap.stats()
    hs, hl = lookup.HostSubjects(snap), lookup.HostLookup(snap)
    roots = np.array(list(range(st["num_expandable"])) + [L.NODE_NONE, st["num_nodes"] - 1], dtype=np.uint32)
    targets = np.array(list(range(st["num_nodes"])) + [L.NODE_NONE], dtype=np.uint32)
    for cls in (lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID):
        want = SC.host_lists(snap, roots[:-2], cls) + [np.zeros(0, dtype=np.uint32)] * 2
        for wide in (False, True):
            got = hs.subject_ids(roots, cls, wide=wide)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            total = sum(len(w) for w in want)
            out, begin, count, needed = hs.subject_ids_raw(roots, cls, total, wide=wide)
            assert needed == total and [int(c) for c in count] == [len(w) for w in want]
    want = [lookup.host_lookup(snap, int(t)) for t in targets[:-1]] + [np.zeros(0, dtype=np.uint32)]
    for wide in (False, True):
        got = hl.lookup_ids(targets, wide=wide)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        out, begin, count, needed = hl.lookup_ids_raw(targets, lookup.TYPE_ANY, 0, wide=wide)
        assert needed == sum(len(w) for w in want)
    docs = [("n", "two", "view"), ("n", "f65", "view"), ("n", "no such doc", "view")]
    for kind in ("ids", "any"):
        plain = hs.list_subjects_batch(docs, kind)
        assert plain == hs.list_subjects_batch(docs, kind, wide=True)
        assert plain == [lookup.host_list_subjects(snap, *d, kind=kind) for d in docs]
        assert hs.ListSubjects(*docs[0], kind=kind, wide=True) == plain[0]
    users = [rt.SubjectID("two_u0"), rt.SubjectID("f65_3"), rt.SubjectID("nobody")]
    plain = hl.list_objects_batch("n", "view", users)
    assert plain == hl.list_objects_batch("n", "view", users, wide=True)
    assert plain == [lookup.host_list_objects(snap, "n", "view", u) for u in users]
    assert hl.ListObjects("n", "view", users[0], wide=True) == plain[0] == ["two"]
    with pytest.raises(L.KetoError) as e:  # an id outside the snapshot, as on the device
        hs.subject_ids([st["num_nodes"]], wide=True)
    assert e.value.code == L.EINVAL
