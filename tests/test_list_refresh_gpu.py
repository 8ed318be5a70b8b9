"""The listing handles follow in-place writes by patching rows on the GPU (hip_host.hpp
ListHandle::try_patch, list_patch_kernel; include/ketogpu.h "listing handles and in-place
writes").  Every answer is compared with the host implementation on the written snapshot, and
the refresh statistics say which path served it.  Cases and writes: tests/refresh_cases.py."""
import gc

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check, lookup
from keto_amd import relationtuple as rt
from tests import refresh_cases as RC

pytestmark = pytest.mark.gpu
ANY, IDS = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=["tier1", "tier2"], autouse=True)
def tiers(request, monkeypatch):
    """handles created while active: the default tiers, or every request through tier 2"""
    if request.param == "tier2":
        monkeypatch.setenv("KETOGPU_LOOKUP_TIER", "2")
        monkeypatch.setenv("KETOGPU_SUBJECTS_TIER", "2")
    return request.param


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, k, list(g[:8]), list(w[:8]), len(g), len(w))


def sizes(snap):
    st = snap.stats()
    return st["num_expandable"], st["num_nodes"]


def check_full_lists(snap, lk, sj, what):
    """the full lists of all roots and of all targets under ANY against the host"""
    nx, n = sizes(snap)
    if sj is not None:
        same(sj.subject_ids(np.arange(nx, dtype=np.uint32), ANY), [lookup.host_subjects(snap, r) for r in range(nx)],
             f"{what}: subjects")
    if lk is not None:
        same(lk.lookup_ids(np.arange(n, dtype=np.uint32), ANY), [lookup.host_lookup(snap, t) for t in range(n)],
             f"{what}: lookup")


def same_pages(got, want, what):
    out, ret, cnt, rem = got[:4]
    wout, wret, wcnt, wrem = want[:4]
    assert np.array_equal(ret, wret) and np.array_equal(cnt, wcnt) and np.array_equal(rem, wrem), what
    for i, r in enumerate(ret):
        assert np.array_equal(out[i][:int(r)], wout[i][:int(r)]), (what, i)


def same_via(got, want, starts, what):
    """ids and hop counts equal the host's; every via is the start or a member one hop nearer"""
    (gl, gf), (wl, wf) = got, want
    assert np.array_equal(gf, wf), what
    for (ids, via, hops), (wids, _, whops), start in zip(gl, wl, starts):
        assert np.array_equal(ids, wids) and np.array_equal(hops, whops), what
        level = dict(zip(ids.tolist(), hops.tolist()))
        for v, h in zip(via.tolist(), hops.tolist()):
            assert (h == 1 and v == start) or level[v] == h - 1, what


def check_every_call(snap, lk, sj, roots, second, targets, path_roots, what):
    """the plain, paged, depth (1, 2), via and combined calls of both handles, and the path call,
    against their CPU twins"""
    hs, hl = lookup.HostSubjects(snap), lookup.HostLookup(snap)
    roots, targets = np.asarray(roots, dtype=np.uint32), np.asarray(targets, dtype=np.uint32)
    same(sj.subject_ids(roots, ANY), [lookup.host_subjects(snap, r) for r in roots], f"{what}: subject ids")
    same_pages(sj.subject_page_raw(roots, None, ANY, 50), hs.subject_page_raw(roots, None, ANY, 50), f"{what}: subject page")
    for k in (1, 2):
        got, want = sj.subject_depth(roots, k), hs.subject_depth(roots, k)
        same(got[0], want[0], f"{what}: subject depth {k}")
        assert np.array_equal(got[1], want[1]), f"{what}: subject frontier {k}"
    same_via(sj.subject_via(roots), hs.subject_via(roots), roots.tolist(), f"{what}: subject via")
    b = np.full(len(roots), second, dtype=np.uint32)
    same(sj.combine_ids(roots, b, "and"), hs.combine_ids(roots, b, "and"), f"{what}: subject and")
    same(lk.lookup_ids(targets, ANY), [lookup.host_lookup(snap, t) for t in targets], f"{what}: lookup ids")
    same_pages(lk.lookup_page_raw(targets, None, ANY, 50), hl.lookup_page_raw(targets, None, ANY, 50), f"{what}: lookup page")
    for k in (1, 2):
        got, want = lk.lookup_depth(targets, k), hl.lookup_depth(targets, k)
        same(got[0], want[0], f"{what}: lookup depth {k}")
        assert np.array_equal(got[1], want[1]), f"{what}: lookup frontier {k}"
    same_via(lk.lookup_via(targets), hl.lookup_via(targets), targets.tolist(), f"{what}: lookup via")
    b = np.full(len(targets), targets[0], dtype=np.uint32)
    same(lk.combine_ids(targets, b, "and"), hl.combine_ids(targets, b, "and"), f"{what}: lookup and")
    pr = np.resize(np.asarray(path_roots, dtype=np.uint32), len(targets))
    got, want = lk.path_ids(pr, targets), hl.path_ids(pr, targets)
    for g, w, r, t in zip(got, want, pr, targets):  # a path with the fewest hops, whichever
        assert len(g) == len(w), f"{what}: path"
        assert not len(g) or (g[0] == r and g[-1] == t), f"{what}: path ends"


def test_lock_step_with_the_host():
    base = RC.base_rows()
    snap, writes = RC.snapshot(base), RC.Writes(base)
    applied = 0
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        check_full_lists(snap, lk, sj, "before any write")
        for k in range(RC.Writes.COUNT):
            ins, dele, _ = writes.write(k)
            res = snap.write(ins, dele)
            if not res["applied"]:
                continue
            writes.applied(ins, dele)
            applied += 1
            check_full_lists(snap, lk, sj, f"write {k}")
            if applied % 10 == 0:
                with lookup.Lookup(snap) as lk2, lookup.Subjects(snap) as sj2:
                    check_full_lists(snap, lk2, sj2, f"write {k}, fresh handles")
        assert applied >= 45
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs["full_uploads"] == 1 and rs["patched_refreshes"] == applied, rs
            assert rs["compactions"] == rs["fallbacks_trimmed"] == rs["fallbacks_backlog"] == 0, rs
            assert rs["rows_patched"] > 0 and rs["words_uploaded"] > 0, rs
            assert h.stats()["uploads"] == 1 + applied
        assert lk.refresh_stats()["rows_moved"] == 0


def growth_snapshot():
    """the series' snapshot with more rows, so that the largest write below stays under a quarter
    of a full upload, and a group `grow` of 3 members inside g0"""
    rows = set(RC.base_rows())
    rows |= {RC.user_row(f"g{k % RC.N_GROUPS}", f"x{k}") for k in range(400)}
    rows |= {RC.user_row("grow", f"u{u}") for u in (1, 2, 3)} | {RC.nest_row("g0", "grow")}
    return RC.snapshot(sorted(rows, key=repr))


def growth_writes():
    """(inserts, deletes): the group gains 1, 7, 64 and 130 members (within its room, past it,
    past one wave's 64 entries, past two), loses all of them and gains 70"""
    steps, have, k = [], [], 0
    for n in (1, 7, 64, 130):
        new = [RC.user_row("grow", f"m{k + i}") for i in range(n)]
        k += n
        have += new
        steps.append((new, []))
    steps.append(([], have))
    steps.append(([RC.user_row("grow", f"m{k + i}") for i in range(70)], []))
    return steps


def test_a_row_grows_past_its_room_and_the_wave_step(monkeypatch):
    monkeypatch.setenv("KETOGPU_LIST_BOUND_STEP", "1")  # every new member moves the bound: tier 2's state is dropped
    snap = growth_snapshot()
    node = lambda s: RC.node_of(snap, s)
    grow, g0, g3 = (node(rt.SubjectSet("groups", g, "member")) for g in ("grow", "g0", "g3"))
    docs = [node(rt.SubjectSet("docs", f"d{d}", "viewer")) for d in range(3)]
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        for step, (ins, dele) in enumerate(growth_writes()):
            res = snap.write(ins, dele)
            assert res["applied"], res
            members = [node(rt.SubjectID(r[3])) for r in (ins or dele)[:3]]
            check_every_call(snap, lk, sj, [grow, g0, docs[0]], g3, members + [node(rt.SubjectID("u1")), grow],
                             docs + [g0], f"step {step}")
        rs = sj.refresh_stats()
        assert rs["rows_moved"] > 0 and rs["full_uploads"] == 1 and rs["patched_refreshes"] == 6, rs
        rl = lk.refresh_stats()
        assert rl["rows_moved"] == 0 and rl["full_uploads"] == 1 and rl["patched_refreshes"] == 6, rl
        check_full_lists(snap, lk, sj, "after the growth")


@pytest.mark.parametrize("slack", [0, 20])
def test_an_exhausted_tail_compacts(slack, monkeypatch):
    """grow starts with room for 7.  +1 fits.  +7 makes 11 and asks for 17 words at the tail:
    with no tail that is the compaction; with a tail of 20 the row moves, and the next growth
    (+30: 41 entries, 55 words) finds the tail exhausted and compacts.  One compaction either
    way, and the rows laid out again leave room for the growth that follows."""
    monkeypatch.setenv("KETOGPU_LIST_ARENA_SLACK", str(slack))
    snap = growth_snapshot()
    grow = RC.node_of(snap, rt.SubjectSet("groups", "grow", "member"))
    k = 0
    with lookup.Subjects(snap) as sj:
        for n in (1, 7, 30) if slack else (1, 7, 2):
            assert snap.write([RC.user_row("grow", f"m{k + i}") for i in range(n)], [])["applied"]
            k += n
            check_full_lists(snap, None, sj, f"slack {slack}, +{n}")
        rs = sj.refresh_stats()
        assert rs["compactions"] == 1 and rs["full_uploads"] == 2 and rs["patched_refreshes"] == 2, rs
        assert rs["rows_moved"] == (1 if slack else 0), rs
        assert sj.stats()["uploads"] == 4
        assert len(sj.subject_ids([grow], IDS)[0]) == 3 + k


def test_full_refresh_knob_takes_the_old_path(monkeypatch):
    monkeypatch.setenv("KETOGPU_LIST_REFRESH", "full")
    snap = growth_snapshot()
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        for n, (ins, dele) in enumerate(growth_writes()[:3]):
            assert snap.write(ins, dele)["applied"]
            check_full_lists(snap, lk, sj, f"full refresh, write {n}")
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs["patched_refreshes"] == 0 and rs["full_uploads"] == 1 + 3, rs
            assert rs["rows_patched"] == rs["words_uploaded"] == 0, rs
            assert h.stats()["uploads"] == 4
    # such a handle is no reader of the log: without one, a write leaves it empty
    with snap.patch_reader() as r:
        assert r.position()[1] == r.position()[2]


@pytest.mark.parametrize("step", [1, 32768], ids=["bound-moves", "bound-stays"])
def test_a_new_subject_is_listed_and_the_bound_moves(step, monkeypatch):
    """KETOGPU_LIST_BOUND_STEP=1: the bitmaps span exactly N, so the new subject moves the bound
    and tier 2's state is dropped; the default rounds the span up and keeps it"""
    monkeypatch.setenv("KETOGPU_LIST_BOUND_STEP", str(step))
    snap = RC.snapshot(RC.base_rows())
    g1 = RC.node_of(snap, rt.SubjectSet("groups", "g1", "member"))
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        n0 = sizes(snap)[1]
        before = sj.subject_ids([g1], IDS)[0]
        for h, raw in ((sj, sj.subject_ids_raw), (lk, lk.lookup_ids_raw)):
            assert raw(np.array([n0], dtype=np.uint32), ANY, 16)[1][0] == lookup.INVALID
        res = snap.write([RC.user_row("g1", "somebody new")], [])
        assert res["applied"] and res["new_nodes"] == 1
        new = RC.node_of(snap, rt.SubjectID("somebody new"))
        assert new == n0 and sizes(snap)[1] == n0 + 1
        after = sj.subject_ids([g1], IDS)[0]
        assert np.array_equal(after, np.sort(np.append(before, new)))
        assert new in sj.subject_ids([g1], ANY)[0] and new not in sj.subject_ids([g1], snap.type_id("groups", "member"))[0]
        same(lk.lookup_ids([new], ANY), [lookup.host_lookup(snap, new)], "the new subject's objects")
        assert g1 in lk.lookup_ids([new], ANY)[0]
        for h, raw in ((sj, sj.subject_ids_raw), (lk, lk.lookup_ids_raw)):
            _, begin, count, _ = raw(np.array([new, n0 + 1], dtype=np.uint32), ANY, 64)
            assert begin[0] != lookup.INVALID and begin[1] == lookup.INVALID and count[1] == 0
            assert h.refresh_stats()["patched_refreshes"] == 1 and h.refresh_stats()["full_uploads"] == 1
        check_full_lists(snap, lk, sj, "after a new subject")


def test_an_idle_handle_catches_up_next_to_an_engine():
    base = RC.base_rows()
    snap, writes = RC.snapshot(base), RC.Writes(base, seed=9)
    eng = check.Engine(snap, device=0)
    with lookup.Lookup(snap) as busy_l, lookup.Subjects(snap) as busy_s, lookup.Lookup(snap) as idle_l, \
            lookup.Subjects(snap) as idle_s:
        done = 0
        for k in (0, 1, 2, 3, 4, 5, 7, 8):
            ins, dele, _ = writes.write(k)
            if not snap.write(ins, dele)["applied"]:
                continue
            writes.applied(ins, dele)
            done += 1
            check_full_lists(snap, busy_l, busy_s, f"busy, write {k}")
            if done == 5:
                break
        assert done == 5
        nx, n = sizes(snap)
        same(idle_s.subject_ids(np.arange(nx, dtype=np.uint32)), busy_s.subject_ids(np.arange(nx, dtype=np.uint32)), "idle subjects")
        same(idle_l.lookup_ids(np.arange(n, dtype=np.uint32)), busy_l.lookup_ids(np.arange(n, dtype=np.uint32)), "idle lookup")
        for h in (idle_l, idle_s):
            rs = h.refresh_stats()
            assert rs["patched_refreshes"] == 1 and rs["full_uploads"] == 1 and rs["fallbacks_trimmed"] == 0, rs
            assert h.stats()["uploads"] == 2
        assert busy_s.refresh_stats()["patched_refreshes"] == 5
        # the engine replays the same log and skips the listing handles' entries
        rng = np.random.default_rng(3)
        named = np.array([v for v in range(n) if snap.subject_class(v) != L.TYPE_NONE], dtype=np.uint32)  # no placeholders
        roots, targets = rng.choice(named[named < nx], 600), rng.choice(named, 600)
        reach = [set(lookup.host_lookup(snap, t).tolist()) for t in range(n)]
        want = np.array([int(r) in reach[int(t)] for r, t in zip(roots, targets)])
        assert np.array_equal(np.asarray(eng.check_ids(roots, targets)).astype(bool), want)
    eng.close()


def test_a_handle_created_after_writes_starts_at_the_current_version():
    base = RC.base_rows()
    snap, writes = RC.snapshot(base), RC.Writes(base)
    for k in range(6):
        ins, dele, _ = writes.write(k)
        snap.write(ins, dele)
    assert snap.version() >= 4
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        check_full_lists(snap, lk, sj, "created after writes")
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs["patched_refreshes"] == 0 and rs["full_uploads"] == 1 and rs["rows_patched"] == 0, rs
            assert h.stats()["uploads"] == 1


def test_a_snapshot_that_cannot_be_written_uploads_once():
    snap = RC.snapshot(RC.base_rows(), writable=False)
    assert not snap.write([RC.user_row("g1", "nobody")], [])["applied"]
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj:
        check_full_lists(snap, lk, sj, "not writable")
        check_full_lists(snap, lk, sj, "not writable, again")
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs.pop("full_uploads") == 1
            assert not any(rs.values()), rs
            assert h.stats()["uploads"] == 1


def test_a_handle_freed_after_its_snapshot():
    snap = RC.snapshot(RC.base_rows())
    lk, sj = lookup.Lookup(snap), lookup.Subjects(snap)
    assert snap.write([RC.user_row("g2", "last one")], [])["applied"]
    lk.snapshot = sj.snapshot = None
    del snap
    gc.collect()
    with pytest.raises(L.KetoError):
        sj.subject_ids([0])
    lk.close(), sj.close()  # registered readers of a log that is gone: nothing of it is touched
