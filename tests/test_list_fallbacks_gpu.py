"""The full uploads a listing handle falls back to in the middle of its life
(ListHandle::try_patch, hip_host.hpp): the backlog fallback behind one large write and behind many
small ones on an idle handle, the exhausted tail, the garbage compaction
(KETOGPU_LIST_ARENA_GARBAGE), and all of them in one life.  Every scenario runs every kind of
call (writable_cases.all_calls) before the upload, when tier 2's slots, the wide queue, the expand
mask and the bad-row bitmap exist already, and right behind it, then makes one small write, which
a patch must serve again, and runs them once more.  The thresholds and each scenario's outcome are
proved on the CPU (test_writable_layout_host.py, writable_cases.HandleModel); here the handles'
refresh statistics are compared with that model counter for counter.  Every scenario's snapshot
is a writable_cases.Twin: the calls before the first write, right behind every full upload and
behind the last write are also compared with a read-only snapshot rebuilt from the mirrored rows."""
import contextlib

import pytest

from keto_amd import expand, lookup
from tests import refresh_cases as RC
from tests import test_list_refresh_gpu as RG
from tests import wide_gpu_suite as W
from tests import writable_cases as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    W.need_gpu()


@pytest.fixture(params=["default", "tier2"], autouse=True)
def tiers(request, monkeypatch):
    return WR.set_tiers(monkeypatch, request.param)


@contextlib.contextmanager
def handles(snap):
    with lookup.Lookup(snap) as lk, lookup.Subjects(snap) as sj, expand.DeviceEngine(snap, subjects=sj) as dev:
        yield lk, sj, dev


def every_call(snap, hs, what, users=("u1", "u2", "u3"), t=None):
    lk, sj, dev = hs
    roots, second, targets, path_roots = WR.rc_starts(snap, users)
    WR.all_calls(snap, lk, sj, dev, roots, second, targets, path_roots, what, roots, t)


def patched_again(t, hs, models, what, users, k=0):
    """one small write behind a full upload is served by a patch, and every call is right"""
    lk, sj, _ = hs
    snap = t.rw
    before = [h.refresh_stats() for h in (lk, sj)]
    assert t.write(WR.fb_small_write(k))["applied"]
    every_call(snap, hs, what, users, t)
    for h, b in zip((lk, sj), before):
        rs = h.refresh_stats()
        assert rs["patched_refreshes"] == b["patched_refreshes"] + 1 and rs["full_uploads"] == b["full_uploads"], (what, rs)
    for m, h in zip(models, (sj, lk)):
        assert m.refresh() == "patch"
        m.assert_handle(h, what)


def test_one_large_write(tiers):
    t = WR.Twin(WR.fb_rows(), RC.NAMESPACES)
    snap, users = t.rw, ("w0", "w17", "u1")
    models = WR.HandleModel(snap, "subjects", t.n0), WR.HandleModel(snap, "lookup", t.n0)
    with handles(snap) as hs:
        lk, sj, dev = hs
        every_call(snap, hs, "before", users, t)
        assert sj.wide_stats()["wide_requests"] > 0 and dev.expand_wide_stats()["mask_builds"] == 1
        assert t.write(WR.fb_large_write())["applied"]
        every_call(snap, hs, "behind the large write", users, t)
        RG.check_full_lists(snap, lk, sj, "behind the large write")
        for m, h in zip(models, (sj, lk)):
            assert m.refresh() == "backlog"
            m.assert_handle(h)
            rs = h.refresh_stats()
            assert rs["fallbacks_backlog"] == 1 and rs["full_uploads"] == 2 and rs["patched_refreshes"] == 0, rs
            assert rs["compactions"] == rs["fallbacks_trimmed"] == 0 and h.stats()["uploads"] == 2
        assert dev.expand_wide_stats()["mask_builds"] == 2
        patched_again(t, hs, models, "a small write behind it", users)
    for m in models:
        m.close()


def test_an_idle_handle(tiers):
    t = WR.Twin(WR.fb_rows(), RC.NAMESPACES)
    snap, users = t.rw, ("w0", "w17", "u1")
    host = lambda ids, f: [f(snap, int(x)) for x in ids]
    with handles(snap) as busy, handles(snap) as idle:
        every_call(snap, idle, "idle, before", users, t)  # its tier-2, wide and expand state exists from here on
        every_call(snap, busy, "busy, before", users)
        for k, ins in enumerate(WR.fb_idle_writes()):
            assert t.write(ins)["applied"], k
            g = RC.node_of(snap, lookup.SubjectSet("groups", f"g{k}", "member"))
            gained = [RC.node_of(snap, lookup.SubjectID(r[3])) for r in ins[:3]]
            RG.same(busy[1].subject_ids([g], wide=k % 2 == 1), host([g], lookup.host_subjects), f"busy subjects, write {k}")
            RG.same(busy[0].lookup_ids(gained, wide=k % 2 == 1), host(gained, lookup.host_lookup), f"busy lookup, write {k}")
        every_call(snap, idle, "idle, its first call behind 15 writes", users, t)
        RG.check_full_lists(snap, idle[0], idle[1], "idle, caught up")
        every_call(snap, busy, "busy, behind 15 writes", users, t)
        for h in idle[:2]:
            rs = h.refresh_stats()
            assert rs["fallbacks_backlog"] == 1 and rs["full_uploads"] == 2 and rs["patched_refreshes"] == 0, rs
            assert rs["compactions"] == rs["fallbacks_trimmed"] == 0 and h.stats()["uploads"] == 2
        for h in busy[:2]:
            rs = h.refresh_stats()
            assert rs["patched_refreshes"] == 15 and rs["full_uploads"] == 1, rs
            assert rs["fallbacks_backlog"] == rs["compactions"] == rs["fallbacks_trimmed"] == 0, rs
        assert busy[1].refresh_stats()["rows_moved"] == 15  # every group outgrew its room
        # everybody has caught up: the next write trims the log
        assert t.write(WR.fb_small_write())["applied"]
        with snap.patch_reader() as r:
            pos, begin, end = r.position()
            assert begin > 0 and pos == end
        for hs, what in ((idle, "idle"), (busy, "busy")):
            before = [h.refresh_stats() for h in hs[:2]]
            every_call(snap, hs, f"{what}, a small write behind it", users, t)
            for h, b in zip(hs[:2], before):
                rs = h.refresh_stats()
                assert rs["patched_refreshes"] == b["patched_refreshes"] + 1 and rs["full_uploads"] == b["full_uploads"], rs


@pytest.mark.parametrize("slack", [0, 20])
def test_an_exhausted_tail(slack, tiers, monkeypatch):
    """test_list_refresh_gpu.test_an_exhausted_tail_compacts with every kind of call on both
    handles, and the state of tier 2, the wide tier and the wide expand made beforehand"""
    monkeypatch.setenv("KETOGPU_LIST_ARENA_SLACK", str(slack))
    t = WR.Twin(WR.growth_rows(), RC.NAMESPACES)  # (test_list_refresh_gpu.growth_snapshot's rows)
    snap = t.rw
    models = WR.HandleModel(snap, "subjects", slack=slack), WR.HandleModel(snap, "lookup")
    grow = RC.node_of(snap, lookup.SubjectSet("groups", "grow", "member"))
    k = 0
    with handles(snap) as hs:
        lk, sj, dev = hs
        every_call(snap, hs, "before", t=t)
        want = ["patch", "patch", "compaction"] if slack else ["patch", "compaction", "patch"]
        for n, outcome in zip((1, 7, 30) if slack else (1, 7, 2), want):
            assert t.write([RC.user_row("grow", f"m{k + i}") for i in range(n)], [])["applied"]
            k += n
            every_call(snap, hs, f"slack {slack}, +{n}", t=t)
            RG.same(sj.subject_ids([grow], wide=True), [lookup.host_subjects(snap, grow)], f"slack {slack}, +{n}: grow")
            assert models[0].refresh() == outcome and models[1].refresh() == "patch"
            models[0].assert_handle(sj), models[1].assert_handle(lk)
        rs = sj.refresh_stats()
        assert rs["compactions"] == 1 and rs["full_uploads"] == 2 and rs["patched_refreshes"] == 2, rs
        assert rs["rows_moved"] == (1 if slack else 0) and rs["fallbacks_backlog"] == 0 and sj.stats()["uploads"] == 4
        rl = lk.refresh_stats()
        assert rl["patched_refreshes"] == 3 and rl["full_uploads"] == 1 and rl["rows_moved"] == 0, rl
        assert len(sj.subject_ids([grow], WR.IDS)[0]) == 3 + k
        patched_again(t, hs, models, "a small write behind the compaction", ("u1", "u2", "u3"))
        RG.check_full_lists(snap, lk, sj, "at the end")
    for m in models:
        m.close()


def test_garbage_compacts(tiers, monkeypatch):
    """KETOGPU_LIST_ARENA_GARBAGE=64: the row's second move would leave 70 words of garbage.  One
    compaction; the same growth once more moves the row in the fresh arena without one"""
    monkeypatch.setenv("KETOGPU_LIST_ARENA_GARBAGE", str(WR.GARBAGE_KNOB))
    t = WR.Twin(WR.garbage_rows(), RC.NAMESPACES)
    snap = t.rw
    models = WR.HandleModel(snap, "subjects", garbage=WR.GARBAGE_KNOB), WR.HandleModel(snap, "lookup")
    grow = RC.node_of(snap, lookup.SubjectSet("groups", "grow", "member"))
    want = [("patch", 1, 0), ("compaction", 1, 1), ("patch", 2, 1)]
    with handles(snap) as hs:
        lk, sj, dev = hs
        every_call(snap, hs, "before", t=t)
        for step, (ins, (outcome, moved, compactions)) in enumerate(zip(WR.garbage_writes(), want)):
            assert t.write(ins)["applied"]
            every_call(snap, hs, f"growth {step}", t=t)
            RG.same(sj.subject_ids([grow], wide=True), [lookup.host_subjects(snap, grow)], f"growth {step}: grow")
            assert models[0].refresh() == outcome and models[1].refresh() == "patch"
            models[0].assert_handle(sj), models[1].assert_handle(lk)
            rs = sj.refresh_stats()
            assert rs["rows_moved"] == moved and rs["compactions"] == compactions, (step, rs)
            assert rs["full_uploads"] == 1 + compactions and rs["fallbacks_backlog"] == 0, (step, rs)
            if outcome == "compaction":
                assert dev.expand_wide_stats()["mask_builds"] == 2 + step
                patched_again(t, hs, models, "a small write behind the compaction", ("u1", "u2", "u3"))
        assert lk.refresh_stats()["full_uploads"] == 1 and lk.refresh_stats()["patched_refreshes"] == 4
        assert sj.stats()["uploads"] == lk.stats()["uploads"] == 5
        RG.check_full_lists(snap, lk, sj, "at the end")
    for m in models:
        m.close()


def test_every_outcome_in_one_life(tiers, monkeypatch):
    """RC.Writes' 60 writes and two scripted ones under a tail of 40 words, a garbage bound of 200
    and a bound that moves with every new subject: patches, moved rows, compactions and the full
    uploads behind them in one handle's life"""
    for knob, value in WR.LIFE_KNOBS.items():
        monkeypatch.setenv(knob, value)
    t = WR.Twin(WR.life_rows(), RC.NAMESPACES)
    snap = t.rw
    msj = WR.HandleModel(snap, "subjects", slack=int(WR.LIFE_KNOBS["KETOGPU_LIST_ARENA_SLACK"]),
                         garbage=int(WR.LIFE_KNOBS["KETOGPU_LIST_ARENA_GARBAGE"]))
    mlk = WR.HandleModel(snap, "lookup")
    applied = 0
    with handles(snap) as hs:
        lk, sj, dev = hs
        every_call(snap, hs, "before", t=t)
        for label, ins, dele, refused, writes in WR.life_writes(t.rows):
            res = t.write(ins, dele)
            assert not (refused and res["applied"]), label
            if not res["applied"]:
                continue
            writes.applied(ins, dele)
            applied += 1
            RG.check_full_lists(snap, lk, sj, label)
            outcome = msj.refresh()
            mlk.refresh()
            if applied % 5 == 0 or label.startswith("scripted") or outcome != "patch":
                every_call(snap, hs, label, t=t)
            msj.assert_handle(sj, label), mlk.assert_handle(lk, label)
        assert writes.rows == t.rows
        rs = sj.refresh_stats()
        for k in ("patched_refreshes", "rows_moved", "compactions"):
            assert rs[k] > 0, rs
        assert rs["full_uploads"] - 1 > 0 and rs["full_uploads"] + rs["patched_refreshes"] == 1 + applied, rs
        assert lk.refresh_stats()["patched_refreshes"] == applied and lk.refresh_stats()["full_uploads"] == 1
        for h in (lk, sj):
            assert h.stats()["uploads"] == 1 + snap.version() == 1 + applied
    msj.close(), mlk.close()
