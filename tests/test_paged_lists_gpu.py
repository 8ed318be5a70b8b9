"""Sorted, paged lists on the device (ketogpu_lookup_page / ketogpu_subjects_page: the ordered
finish of keto_amd/csrc/paged_finish.hpp behind the closures of lookup.hip and subjects.hip).
The yardstick is always the host list (host_lookup / host_subjects, ascending) sliced at
searchsorted(list, from).  Every test runs for both handles unless its name says otherwise."""
import functools
import gc

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check, expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC
from tests import test_subjects_gpu as TS  # WORKLOADS / workload(): the synthetic snapshots, built once

pytestmark = pytest.mark.gpu
ANY, IDS = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


class Side:
    """one of the two handles behind the same calls"""

    def __init__(self, name, handle, page, host, env, universe, c_page):
        self.name, self.handle, self._page, self._host = name, handle, page, host
        self.env, self.universe, self.c_page = env, universe, c_page

    def page(self, h, ids, lo, filt, limit):
        return getattr(h, self._page)(ids, lo, filt, limit)

    def host(self, snap, ids, filt=ANY):
        return [self._host(snap, int(v), filt) for v in ids]

    def __repr__(self):
        return self.name


LK = Side("lookup", lookup.Lookup, "lookup_page_raw", lookup.host_lookup, "KETOGPU_LOOKUP", "num_nodes",
          "ketogpu_lookup_page")
SJ = Side("subjects", lookup.Subjects, "subject_page_raw", lookup.host_subjects, "KETOGPU_SUBJECTS",
          "num_expandable", "ketogpu_subjects_page")
SIDES = [LK, SJ]
# (tiers): the tier fixtures of test_lookup_gpu.py / test_subjects_gpu.py
MODES = [(LK, "default"), (LK, "tier2"), (SJ, "default"), (SJ, "tier2"), (SJ, "tier2-scan")]
mode_ids = lambda m: f"{m[0].name}-{m[1]}"


def set_tier(monkeypatch, side, tier):
    """handles created afterwards: the default tiers, every request through tier 2, or (subjects)
    through tier 2 with every finish by scan"""
    if tier != "default":
        monkeypatch.setenv(side.env + "_TIER", "2")
    if tier == "tier2-scan":
        monkeypatch.setenv(side.env + "_LIST_CAP", "0")


def check_page(side, h, ids, lo, filt, limit, want):
    """one paged call against the host slices"""
    ids = np.asarray(ids, dtype=np.uint32)
    out, ret, cnt, rem = side.page(h, ids, lo, filt, limit)
    assert out.shape == (len(ids), limit)
    for i, w in enumerate(want):
        k = int(np.searchsorted(w, 0 if lo is None else lo[i]))
        exp = w[k:k + limit]
        assert int(cnt[i]) == len(w) and int(rem[i]) == len(w) - k, (i, int(ids[i]), int(cnt[i]), int(rem[i]))
        assert int(ret[i]) == len(exp) == min(limit, len(w) - k), (i, int(ids[i]), int(ret[i]))
        assert np.array_equal(out[i, :len(exp)], exp), (i, int(ids[i]))
    return out, ret, cnt, rem


def walk(side, h, ids, filt, limit, want):
    """pages to the end; -> the number of calls"""
    ids = np.asarray(ids, dtype=np.uint32)
    lo = np.zeros(len(ids), dtype=np.uint32)
    acc = [[] for _ in ids]
    active = np.arange(len(ids))
    calls = 0
    while len(active):
        out, ret, cnt, rem = side.page(h, ids[active], lo[active], filt, limit)
        calls += 1
        for j, i in enumerate(active):
            k = int(ret[j])
            page = out[j, :k]
            assert (np.diff(page.astype(np.int64)) > 0).all(), (int(ids[i]), page)  # strictly ascending
            assert k == min(limit, int(rem[j])) and (k == 0 or page[0] >= lo[i])
            assert int(cnt[j]) == len(want[i])  # constant across pages
            assert int(rem[j]) == len(want[i]) - len(acc[i])  # falls by what was returned
            acc[i].extend(int(v) for v in page)
            if k:
                lo[i] = int(page[-1]) + 1
        active = active[rem > ret]
        assert calls <= 4096
    for i, w in enumerate(want):
        assert np.array_equal(np.array(acc[i], dtype=np.uint32), w), (i, int(ids[i]))
    return calls


# ------------------------------------------------------------------------------- truth tables
@functools.lru_cache(maxsize=None)
def table_lists(side, case):
    _, _, snap = LC.table(*case)
    return side.host(snap, range(snap.stats()[side.universe]))


@pytest.mark.parametrize("mode", MODES, ids=mode_ids)
@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables(case, mode, monkeypatch):
    side, tier = mode
    set_tier(monkeypatch, side, tier)
    _, _, snap = LC.table(*case)
    ids = np.arange(snap.stats()[side.universe], dtype=np.uint32)
    want = table_lists(side, case)
    longest = max(len(w) for w in want)
    assert 7 < longest <= 4096
    with side.handle(snap) as h:
        assert walk(side, h, ids, ANY, 7, want) == -(-longest // 7)  # the longest list's pages
        assert walk(side, h, ids, ANY, 4096, want) == 1
        walk(side, h, ids[:8], ANY, 1, want[:8])
        st = h.stats()
        assert (st["tier2_requests"] == st["requests"]) == (tier != "default")
        assert st["truncated_lists"] == 0


# ---------------------------------------------------------------------------------- from edges
@functools.lru_cache(maxsize=None)
def structure():
    snap = Snapshot.from_rows(LC.NS1, SC.structure_rows())
    return snap


@functools.lru_cache(maxsize=None)
def structure_lists(side):
    snap = structure()
    return side.host(snap, range(snap.stats()["num_nodes"]))


def struct_id(side, lk_user, sj_obj, sj_rel="view"):
    snap = structure()
    if side is LK:
        return int(lookup.resolve_subjects(snap, [rt.SubjectID(lk_user)])[0])
    return int(lookup.resolve_roots(snap, [("n", sj_obj, sj_rel)])[0])


@pytest.mark.parametrize("mode", MODES, ids=mode_ids)
def test_from_edges(mode, monkeypatch):
    side, tier = mode
    set_tier(monkeypatch, side, tier)
    snap = structure()
    n = snap.stats()["num_nodes"]
    chain = struct_id(side, "uc", "c2999", "member")
    w = structure_lists(side)[chain]
    assert len(w) == 3000
    froms = [0]
    for m in (int(w[0]), int(w[len(w) // 2]), int(w[-1])):
        froms += [m, m + 1, max(m - 1, 0)]
    for residue in (31, 0, 1):  # a member at the end, the start and the second bit of a bitmap word
        hit = w[w % 32 == residue]
        if len(hit):
            froms += [int(hit[len(hit) // 2])]
    froms += [n - 1, n, 0xFFFFFFFF]
    with side.handle(snap) as h:
        for f in froms:
            check_page(side, h, [chain], np.array([f], dtype=np.uint32), ANY, 64, [w])
        a = side.page(h, [chain] * 3, None, ANY, 64)
        b = side.page(h, [chain] * 3, np.zeros(3, dtype=np.uint32), ANY, 64)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and int(a[1][0]) == 64
        lo = np.array(froms, dtype=np.uint32)  # one call, a different bound per request
        out, ret, cnt, rem = check_page(side, h, [chain] * len(lo), lo, ANY, 64, [w] * len(lo))
        assert not rem[-2:].any() and not ret[-2:].any() and (cnt == 3000).all()


# ---------------------------------------------------------------------- tier-1 set boundary
@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_set_boundary(side):
    with side.handle(Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])) as h0:
        cap = h0.stats()["set_capacity"]
    assert cap >= 64
    sizes = (cap - 1, cap, cap + 1)
    rows = []
    for k in sizes:
        if side is LK:
            rows += LC.star_rows(f"star{k}", k, f"a{k}_") + LC.split_star_rows(f"split{k}", k, f"b{k}_")
        else:
            rows += SC.fwd_star_rows(f"star{k}", k, f"a{k}_") + SC.fwd_split_rows(f"split{k}", k, f"b{k}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with side.handle(snap) as h:
        for shape in ("star", "split"):
            for k in sizes:
                if side is LK:
                    r = lookup.resolve_subjects(snap, [rt.SubjectID(f"{shape}{k}")])
                else:
                    r = lookup.resolve_roots(snap, [("n", f"{shape}{k}", "view")])
                want = side.host(snap, r)
                assert len(want[0]) == k
                for limit in (1, 64, 65, k, k + 1):
                    before = h.stats()
                    out, ret, cnt, rem = check_page(side, h, r, None, ANY, limit, want)
                    assert int(ret[0]) == min(limit, k)
                    after = h.stats()
                    assert after["tier2_requests"] - before["tier2_requests"] == (1 if k > cap else 0), (shape, k)
                    assert after["tier1_requests"] - before["tier1_requests"] == (0 if k > cap else 1), (shape, k)
                    assert after["ids_produced"] - before["ids_produced"] == min(limit, k)


# ---------------------------------------------------------------- list-finish boundary (subjects)
def test_subjects_list_finish_boundary(monkeypatch):
    k = 130
    monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    monkeypatch.setenv("KETOGPU_SUBJECTS_LIST_CAP", str(k))
    sizes = (k - 1, k, k + 1)
    rows = []
    for m in sizes:
        rows += SC.fwd_star_rows(f"star{m}", m, f"a{m}_") + SC.fwd_split_rows(f"split{m}", m, f"b{m}_")
    snap = Snapshot.from_rows(LC.NS1, rows)
    with lookup.Subjects(snap) as sj:
        assert sj.stats()["list_capacity"] == k
        for rep in range(2):  # the second round finds the bitmaps clean after both finishes
            for shape in ("star", "split"):
                for m in sizes:
                    r = lookup.resolve_roots(snap, [("n", f"{shape}{m}", "view")])
                    want = SJ.host(snap, r)
                    assert len(want[0]) == m
                    before = sj.stats()
                    check_page(SJ, sj, r, None, ANY, 100, want)
                    after = sj.stats()
                    assert after["list_finishes"] - before["list_finishes"] == (1 if m <= k else 0), (shape, m)
                    assert after["scan_finishes"] - before["scan_finishes"] == (0 if m <= k else 1), (shape, m)
        # a paged call and a full call alternate over the same roots: either finish leaves the slots clean
        r = lookup.resolve_roots(snap, [("n", f"{shape}{m}", "view") for shape in ("star", "split") for m in sizes])
        want = SJ.host(snap, r)
        total = sum(len(w) for w in want)
        lo = np.array([int(w[len(w) // 2]) for w in want], dtype=np.uint32)
        for rep in range(2):
            check_page(SJ, sj, r, lo, ANY, 40, want)
            out, begin, count, needed = sj.subject_ids_raw(r, ANY, total)
            assert needed == total
            for b, c, w in zip(begin, count, want):
                assert np.array_equal(np.sort(out[int(b):int(b) + int(c)]), w)
        assert sj.stats()["truncated_lists"] == 0


# ---------------------------------------------------------------------------------- slot reuse
@pytest.mark.parametrize("slots", (1, 2))  # 2: a full round, then a partial one in which slot != request
@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_slot_reuse(side, slots, monkeypatch):
    monkeypatch.setenv(side.env + "_TIER", "2")
    monkeypatch.setenv(side.env + "_SLOTS", str(slots))
    rounds = 3 if slots == 1 else 2  # per call: 3 overflow requests
    snap = structure()
    r = np.array([struct_id(side, "u129", "f129"), struct_id(side, "uc", "c2999", "member"),
                  struct_id(side, "u65", "f65")], dtype=np.uint32)
    filt = ANY if side is LK else IDS
    want = side.host(snap, r, filt)
    assert [len(w) for w in want] == [129, 3000 if side is LK else 1, 65]
    want_any = side.host(snap, r, ANY)
    assert [len(w) for w in want_any] == [129, 3000, 65]
    lo = np.array([int(want_any[0][100]), int(want_any[1][1500]), 0], dtype=np.uint32)
    with side.handle(snap) as h:
        first = check_page(side, h, r, lo, ANY, 100, want_any)
        st = h.stats()
        assert st["tier2_rounds"] == rounds and st["tier2_requests"] == 3 and st["slots"] == slots
        again = check_page(side, h, r, lo, ANY, 100, want_any)  # the slot was left clean
        for x, y, k in zip(first[0], again[0], first[1]):
            assert np.array_equal(x[:int(k)], y[:int(k)])
        assert all(np.array_equal(x, y) for x, y in zip(first[1:], again[1:]))
        check_page(side, h, r, None, filt, 100, want)
        assert h.stats()["tier2_rounds"] == 3 * rounds and h.stats()["uploads"] == 1


# ------------------------------------------------------------------- batch sizes and bad ids
@pytest.mark.parametrize("mode", MODES, ids=mode_ids)
def test_batch_sizes_and_bad_ids(mode, monkeypatch):
    side, tier = mode
    set_tier(monkeypatch, side, tier)
    snap = structure()
    want = structure_lists(side)
    st = snap.stats()
    n, nx = st["num_nodes"], st["num_expandable"]
    with side.handle(snap) as h:
        out, ret, cnt, rem = side.page(h, np.zeros(0, dtype=np.uint32), None, ANY, 8)
        assert out.shape == (0, 8) and len(ret) == len(cnt) == len(rem) == 0
        for m in (1, 63, 64, 65):
            r = np.arange(5, 5 + m, dtype=np.uint32)
            check_page(side, h, r, None, ANY, 16, [want[int(x)] for x in r])
        # a valid id, no node, outside the snapshot (twice), the last node; for subjects also the
        # first never-expanded id and the last expandable one
        r = [7, L.NODE_NONE, n, 9, 0xFFFFFFFE, n - 1] + ([nx, nx - 1] if side is SJ else [])
        r = np.array(r, dtype=np.uint32)
        before = h.stats()
        out, ret, cnt, rem = side.page(h, r, None, ANY, 16)
        bad = ret == lookup.PAGE_INVALID
        assert list(np.nonzero(bad)[0]) == [2, 4]
        assert not cnt[bad].any() and not rem[bad].any()
        assert ret[1] == 0 and cnt[1] == 0 and rem[1] == 0  # NONE: the empty page, not an error
        ok = [k for k in range(len(r)) if k not in (1, 2, 4)]
        check_page(side, h, r[ok], None, ANY, 16, [want[int(x)] for x in r[ok]])
        if side is SJ:
            assert ret[6] == 0 and cnt[6] == 0 and len(want[n - 1]) == 0 and ret[5] == 0  # leaves list nothing
        after = h.stats()
        assert after["requests"] - before["requests"] == len(r) + len(ok)
        listed = (after["tier1_requests"] + after["tier2_requests"]
                  - before["tier1_requests"] - before["tier2_requests"])
        assert listed == 2 * len(ok)  # NONE and the two bad ids belong to neither tier


# ------------------------------------------------------------------------------------- filters
@functools.lru_cache(maxsize=None)
def workload_lists(side, kind, seed, m, filt):
    snap = TS.workload(kind)
    ids = np.random.default_rng(seed).integers(0, snap.stats()[side.universe], m).astype(np.uint32)
    return ids, side.host(snap, ids, filt)


@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_filters(side):
    snap = TS.workload("rbac")
    ty = snap.type_id("groups", "member")
    assert ty not in (lookup.TYPE_NONE, ANY)
    with side.handle(snap) as h:
        for filt in (ANY, IDS, ty, lookup.TYPE_NONE, lookup.CLASS_UNTYPED_SET):
            ids, want = workload_lists(side, "rbac", 11, 300, filt)
            out, ret, cnt, rem = check_page(side, h, ids, None, filt, 100, want)
            if filt in (lookup.TYPE_NONE, lookup.CLASS_UNTYPED_SET):
                assert not ret.any() and not cnt.any() and not rem.any()
            if filt in (ANY, ty) or (filt == IDS and side is SJ):
                assert cnt.any()


# ----------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_argument_errors(side):
    snap = structure()
    with side.handle(snap) as h:
        for limit in (0, 65537):
            with pytest.raises(L.KetoError) as e:
                side.page(h, np.zeros(1, dtype=np.uint32), None, ANY, limit)
            assert e.value.code == L.EINVAL
        ids, ret = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        cnt, rem = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        fn = getattr(L.lib(), side.c_page)
        assert fn(h.h, ids.ctypes.data, None, 1, ANY, 4, None, ret.ctypes.data, cnt.ctypes.data,
                  rem.ctypes.data) == L.EINVAL
        assert fn(h.h, None, None, 0, ANY, 4, None, None, None, None) == L.OK  # n == 0 touches nothing
        assert h.stats()["requests"] == 0


# ------------------------------------------------------------------------ synthetic workloads
@pytest.mark.parametrize("kind", ["rbac", "social"])
@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_synthetic_workloads(side, kind):
    snap = TS.workload(kind)
    ids, want = workload_lists(side, kind, 7, 2000, ANY)
    with side.handle(snap) as h:
        out, ret, cnt, rem = check_page(side, h, ids, None, ANY, 100, want)
        st = h.stats()
        over = sum(len(w) > st["set_capacity"] for w in want)
        assert st["tier2_requests"] == over and 0 < over < len(ids), "the sample uses both tiers"
        more = np.nonzero(rem > ret)[0]
        assert len(more)
        lo = np.array([int(out[i, 99]) + 1 for i in more], dtype=np.uint32)
        check_page(side, h, ids[more], lo, ANY, 100, [want[i] for i in more])


# -------------------------------------------------------------------------------------- writes
@pytest.mark.parametrize("mode", MODES, ids=mode_ids)
def test_writes_are_seen_by_the_next_page(mode, monkeypatch):
    side, tier = mode
    set_tier(monkeypatch, side, tier)
    if side is SJ:
        rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
                LC.sset("doc2", "view", "h", "member"), LC.sid("doc3", "view", "bob")]
        rows += [LC.sid("h", "member", f"m{i}") for i in range(40)]
    else:
        rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"),
                LC.sid("h", "member", "bob"), LC.sid("doc3", "view", "bob")]
        rows += [LC.sset(f"h{i}", "view", "h", "member") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    alice = rt.SubjectID("alice")
    with side.handle(snap) as h:
        if side is SJ:
            twin = lookup.HostSubjects(snap)
            page = lambda x, d, **kw: x.list_subjects_page("n", d, "view", **kw)
            names = lambda x, d: [s.id for s in page(x, d)[0]]
            assert names(h, "doc1") == ["alice"] and len(names(h, "doc2")) == 41 and h.stats()["uploads"] == 1
            assert snap.write([LC.sid("h", "member", "alice")])["applied"]
            got = page(h, "doc2")
            assert got == page(twin, "doc2") and alice in got[0] and got[2] == 42 and h.stats()["uploads"] == 2
            at = got[0].index(alice)  # at its place: also the first item of the page that starts there
            tok = "" if at == 0 else page(h, "doc2", page_size=at)[1]
            assert page(h, "doc2", page_size=3, page_token=tok)[0][0] == alice
            assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (reserved id)
            got = page(h, "doc2")
            assert got == page(twin, "doc2") and rt.SubjectID("carol") in got[0] and got[2] == 43
            assert h.stats()["uploads"] == 3
            assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]  # a deleted row disappears
            assert page(h, "doc1") == ([], "", 0) and page(h, "doc2") == got and h.stats()["uploads"] == 4
        else:
            twin = lookup.HostLookup(snap)
            page = lambda x, s, **kw: x.list_objects_page("n", "view", s, **kw)
            assert page(h, alice) == (["doc1"], "", 1) and h.stats()["uploads"] == 1
            assert snap.write([LC.sid("h", "member", "alice")])["applied"]
            got = page(h, alice)
            assert got == page(twin, alice) and got[2] == 41 and h.stats()["uploads"] == 2
            assert sorted(got[0]) == sorted(["doc1"] + [f"h{i}" for i in range(40)])
            assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (reserved id)
            got = page(h, rt.SubjectID("carol"), page_size=7)
            assert got == page(twin, rt.SubjectID("carol"), page_size=7) and got[2] == 40 and got[1] != ""
            assert h.stats()["uploads"] == 3
            assert snap.write((), [LC.sid("h", "member", "alice")])["applied"]  # a deleted row disappears
            assert page(h, alice) == (["doc1"], "", 1) and h.stats()["uploads"] == 4
        assert page(h, "doc1" if side is SJ else alice) == page(twin, "doc1" if side is SJ else alice)
        assert h.stats()["uploads"] == 4  # no write since: no upload


@pytest.mark.parametrize("side", SIDES, ids=repr)
def test_handle_outlives_its_snapshot(side):
    snap = Snapshot.from_rows(LC.NS1, [LC.sid("d", "view", "u")])
    h = side.handle(snap)
    ids = np.arange(snap.stats()["num_nodes"], dtype=np.uint32)
    assert int(side.page(h, ids, None, ANY, 4)[2].sum()) == 1
    h.snapshot = None
    del snap
    gc.collect()
    with pytest.raises(L.KetoError) as e:  # the rows in HBM are a copy, but the version cannot be read
        side.page(h, ids, None, ANY, 4)
    assert e.value.code == L.EINVAL
    h.close()


# --------------------------------------------------------------------------------------- names
def chain_pages(fn, page_size):
    """fn(page_size=, page_token=) to the end -> the list of (items, token, total)"""
    pages, tok = [], ""
    while True:
        pages.append(fn(page_size=page_size, page_token=tok))
        tok = pages[-1][1]
        if tok == "":
            return pages
        assert len(pages[-1][0]) == page_size and len(pages) < 10000


def test_list_objects_page_by_name():
    snap = TS.workload("rbac")
    users = [rt.SubjectID(f"u{u}") for u in (3, 17, 4242, 19999)] + [rt.SubjectID("nobody")]
    twin = lookup.HostLookup(snap)
    with lookup.Lookup(snap) as lk:
        full = lk.list_objects_batch("docs", "viewer", users)
        assert any(len(f) > 50 for f in full), "some list has more than one page"
        for u, f in zip(users, full):
            pages = chain_pages(lambda **kw: lk.list_objects_page("docs", "viewer", u, **kw), 50)
            assert pages == chain_pages(lambda **kw: twin.list_objects_page("docs", "viewer", u, **kw), 50)
            items = [x for p in pages for x in p[0]]
            assert sorted(items) == f and len(set(items)) == len(items)
            assert all(p[2] == len(f) for p in pages) and pages[-1][1] == ""
        batch = lk.list_objects_page_batch("docs", "viewer", [(u, "") for u in users] + [(users[0], "17")], 50)
        assert batch[:-1] == [lk.list_objects_page("docs", "viewer", u, 50) for u in users]
        assert batch[-1] == lk.list_objects_page("docs", "viewer", users[0], 50, "17")
        reqs = [(u, "") for u in users] + [(users[0], "17")]
        assert batch == twin.list_objects_page_batch("docs", "viewer", reqs, 50)
        assert lk.list_objects_page("docs", "viewer", users[-1]) == ([], "", 0)
        assert lk.list_objects_page("nowhere", "viewer", users[0]) == ([], "", 0)


def test_list_subjects_page_by_name():
    snap = TS.workload("rbac")
    docs = [("docs", f"d{i}", "viewer") for i in (0, 3, 17, 3999)] + [("docs", "no such doc", "viewer"),
                                                                       ("nowhere", "d0", "viewer")]
    twin = lookup.HostSubjects(snap)
    key = lambda s: (0, s.id) if isinstance(s, rt.SubjectID) else (1, s.namespace, s.object, s.relation)
    with lookup.Subjects(snap) as sj:
        for kind in ("ids", "any", ("groups", "member"), ("groups", "no such relation")):
            full = sj.list_subjects_batch(docs, kind)
            for d, f in zip(docs, full):
                pages = chain_pages(lambda **kw: sj.list_subjects_page(*d, kind=kind, **kw), 50)
                assert pages == chain_pages(lambda **kw: twin.list_subjects_page(*d, kind=kind, **kw), 50)
                items = [x for p in pages for x in p[0]]
                assert sorted(items, key=key) == sorted(f, key=key) and len(set(items)) == len(items)
                assert all(p[2] == len(f) for p in pages) and pages[-1][1] == ""
            reqs = [(d, "") for d in docs] + [(docs[0], "17")]
            batch = sj.list_subjects_page_batch(reqs, kind, 50)
            assert batch[:-1] == [sj.list_subjects_page(*d, kind=kind, page_size=50) for d in docs]
            assert batch[-1] == sj.list_subjects_page(*docs[0], kind=kind, page_size=50, page_token="17")
            assert batch == twin.list_subjects_page_batch(reqs, kind, 50)
        assert any(len(f) > 50 for f in sj.list_subjects_batch(docs, "ids")), "some list has more than one page"


def test_handler_routes_over_the_device_handles():
    """the list routes over Lookup / Subjects answer as over the CPU twins, and /check and /expand
    of a Handler built with four arguments answer as with two"""
    snap = structure()
    two = Handler(check.Engine(snap), expand.Engine(snap))
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        four = Handler(two.check, two.expand, lk, sj)
        twin = Handler(None, None, lookup.HostLookup(snap), lookup.HostSubjects(snap))
        for query in ("namespace=n&relation=view&subject_id=u129&page_size=50",
                      "namespace=n&relation=view&subject_id=u129&page_size=50&page_token=4200",
                      "namespace=n&relation=member&subject_id=uc&page_size=1000", "namespace=n&relation=view",
                      "namespace=n&relation=view&subject_id=nobody",
                      "namespace=n&relation=view&subject_id=u65&page_token=x"):
            assert four.get_list_objects(query) == twin.get_list_objects(query), query
        for query in ("namespace=n&object=f129&relation=view&page_size=64",
                      "namespace=n&object=two&relation=view&kind=any",
                      "namespace=n&object=c2999&relation=member&kind=n%23member&page_size=1000&page_token=77",
                      "namespace=n&object=f65&relation=view&page_size=0", "namespace=nowhere&object=f65&relation=view"):
            assert four.get_list_subjects(query) == twin.get_list_subjects(query), query
        assert four.get_list_objects("namespace=n&relation=view&subject_id=u129&page_size=50")[1]["total"] == 129
        for query in ("namespace=n&object=top&relation=view&subject_id=ux",
                      "namespace=n&object=top&relation=view&subject_id=uc",
                      "namespace=nowhere&subject_id=ux", "", "namespace=n&subject_id=ux"):
            assert four.get_check(query) == two.get_check(query), query
        assert four.get_check("namespace=n&object=top&relation=view&subject_id=ux") == (200, {"allowed": True})
        assert four.get_check("namespace=n&object=top&relation=view&subject_id=uc") == (403, {"allowed": False})
        query = "namespace=n&object=top&relation=view&max-depth=3"
        assert four.get_expand(query) == two.get_expand(query) and four.get_expand(query)[0] == 200
