"""Rows of a writable snapshot that grow, move to the arena's tail and shrink, at the sizes where
the kernels take another path: a wide chunk (2048 entries), the run window of the wide expand
(64 x 64), an attention entry at a 64-entry border, a reverse row's free slots, a new subject that
moves the bitmaps' bound.  One graph and one scripted series (tests/writable_cases.py moves_rows,
moves_script; test_writable_layout_host.py proves what each write does on the CPU).  After every
write every kind of call runs on the touched starts and their neighbours (WR.all_calls), against
the host twin on the written snapshot and against a read-only snapshot rebuilt from the mirrored
row table, and the refresh statistics are compared, counter for counter, with the refresh state
machine replayed on the host (WR.HandleModel).

That a run step read the moved row and that fill items were queued from the arena's tail is
asserted from the wide expand's counters under the default tiers only; with tier 2 forced the walk
queues nothing, and that step checks answers alone.  Where a moved row lies is the model's
(`moved_at`), whose counters are the handle's."""
import numpy as np
import pytest

from keto_amd import expand, lookup
from tests import expand_wide_cases as WC
from tests import wide_gpu_suite as W
from tests import writable_cases as WR

pytestmark = pytest.mark.gpu
ANY = WR.ANY
C = WR.CHUNK
# the steps behind which the read-only snapshot is rebuilt from the mirror (a third of a second
# each): a row at the tail, three rows at the tail, shrunk and grown there, the reverse rows, the end
READ_ONLY_AT = (1, 5, 8, 10, 13)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    W.need_gpu()


@pytest.fixture(params=["default", "tier2"])
def tiers(request, monkeypatch):
    return WR.set_tiers(monkeypatch, request.param)


def members_of(snap, rows):
    """the node ids of the subjects these rows name"""
    subs = [lookup.SubjectID(r[3]) if r[3] is not None else lookup.SubjectSet("n", r[5], r[6]) for r in rows]
    return [int(v) for v in lookup.resolve_subjects(snap, subs)]


def root_of(snap, row):
    return int(lookup.resolve_roots(snap, [("n", row[1], row[2])])[0])


def step_starts(t, s, ins, dele):
    """the starts of one step: the row the write touched, its neighbours in the arena and a row
    far from it; the subjects it named and two users nothing touched"""
    rows = list(ins) or list(dele)
    touched = root_of(t.rw, rows[0])
    roots = [touched] + [v for v in (touched - 1, touched + 1) if v not in t.placeholders()] + [s["fill"]]
    named = members_of(t.rw, rows[:2])
    targets = named + [s["a_user"], s["lstars"][0], s["small"]]
    xroots = [touched, s["wl"], s["wl96"], s["wp"], s["wp64"], s["wp_child"], s["wres"]]
    return roots, targets, xroots


def test_rows_grow_move_and_shrink(tiers):
    t = WR.Twin(WR.moves_rows())
    rw = t.rw
    s = WR.moves_starts(t)
    star, wl = s["stars"][0], s["wl"]
    msj, mlk = WR.HandleModel(rw, "subjects", t.n0), WR.HandleModel(rw, "lookup", t.n0)
    tail0 = msj.tail
    with lookup.Lookup(rw) as lk, lookup.Subjects(rw) as sj, expand.DeviceEngine(rw, subjects=sj) as dev:
        assert sj.wide_stats()["chunk"] == C
        ex = expand.Engine(rw)
        WR.all_calls(rw, lk, sj, dev, [star, s["stars"][1], s["fill"]], s["stars"][2],
                     [s["a_user"], s["lstars"][0], s["small"]], [star], "before any write",
                     [star, wl, s["wp"], s["wres"]], t)
        builds = dev.expand_wide_stats()["mask_builds"]
        assert builds == 1
        applied = 0
        for k, (label, ins, dele, expect) in enumerate(WR.moves_script()):
            before = {"sj": sj.refresh_stats(), "uploads": (sj.stats()["uploads"], lk.stats()["uploads"]),
                      "xw": dev.expand_wide_stats(), "wide": sj.wide_stats()}
            res = t.write(ins, dele)
            assert res["reason"] == expect, (label, res)
            roots, targets, xroots = step_starts(t, s, ins, dele)
            WR.all_calls(rw, lk, sj, dev, roots, s["stars"][2], targets, roots, label, xroots, t if k in READ_ONLY_AT else None)
            if not res["applied"]:  # refused: nothing of the handles moves
                assert (sj.stats()["uploads"], lk.stats()["uploads"]) == before["uploads"], label
                assert dev.expand_wide_stats()["mask_builds"] == builds, label
                continue
            applied += 1
            assert msj.refresh() == "patch" and mlk.refresh() == "patch", label
            msj.assert_handle(sj, label), mlk.assert_handle(lk, label)
            builds += 1  # the rows' epoch moved: the first wide expand call behind the write builds the mask again
            xw = dev.expand_wide_stats()
            assert xw["mask_builds"] == builds, label
            if tiers == "default":
                assert xw["items_queued"] > before["xw"]["items_queued"], label
            moved = sj.refresh_stats()["rows_moved"] - before["sj"]["rows_moved"]
            if k == 0:
                assert moved == 0
            if k == 1:  # the star of C + 601 now lies at the tail, off a 64-word boundary: two wide chunks read it
                assert moved == 1 and msj.moved_at[star] == tail0 and tail0 % 64
                w0 = sj.wide_stats()
                out, begin, count, needed = sj.subject_ids_raw([star], ANY, C + 601, wide=True)
                assert needed == C + 601 and begin[0] == 0 and np.array_equal(np.sort(out), lookup.host_subjects(rw, star))
                w1 = sj.wide_stats()
                assert w1["wide_requests"] - w0["wide_requests"] == 1 and w1["items"] - w0["items"] == 2
            if k in (2, 3):
                assert moved == 0
            if k == 4:  # 5197 entries at the tail: a run past the window, its fill items' sources in the tail
                assert moved == 1 and msj.moved_at[wl] >= tail0 + C + 601
                x0 = dev.expand_wide_stats()
                assert (WC.assert_device_wide(dev, ex, [wl], WC.ALL) == 0).all()
                x1 = dev.expand_wide_stats()
                if tiers == "default":
                    assert x1["run_steps"] > x0["run_steps"] and x1["items_queued"] - x0["items_queued"] >= 2
                    assert x1["skipped_entries"] - x0["skipped_entries"] >= 5197
            if k == 5:
                assert moved == 1 and msj.moved_at[s["wp"]] > msj.moved_at[wl]
                _, kids, _ = ex.expand_ids(s["wp"], WC.ALL)
                assert kids[0] == 380 and kids[1 + 63 + 80] == 1  # the opening child, 80 entries later
            if k == 6:
                _, kids, _ = ex.expand_ids(s["wp"], WC.ALL)
                assert moved == 0 and kids[1 + 63 + 80] == 2
            if k in (7, 8):  # shrunk inside its room at the tail, then grown by one: no second move
                assert moved == 0 and msj.moved_at[star] == tail0
            if k == 13:  # patched where it lies: the opening child 79 entries later, in another 64-entry window
                _, kids, _ = ex.expand_ids(s["wp64"], WC.ALL)
                assert moved == 0 and kids[0] == 379 and kids[1 + 64 + 79] == 1 and kids[1 + 64] == 0
        assert applied == 13
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs["full_uploads"] == 1 and rs["patched_refreshes"] == applied, rs
            assert rs["compactions"] == rs["fallbacks_backlog"] == rs["fallbacks_trimmed"] == 0, rs
            assert h.stats()["uploads"] == 1 + applied
        assert sj.refresh_stats()["rows_moved"] == 3 and lk.refresh_stats()["rows_moved"] == 0
        assert sj.wide_stats()["wide_requests"] > 0 and lk.wide_stats()["wide_requests"] > 0
    msj.close(), mlk.close()


@pytest.mark.parametrize("step", [1, 32768], ids=["bound-moves", "bound-stays"])
def test_a_new_subject_joins_the_largest_star(step, tiers, monkeypatch):
    """KETOGPU_LIST_BOUND_STEP=1: the new subject moves the bound, and tier 2's slots, the wide
    queue and the expand state are dropped; the default step keeps them.  The next wide, wide-page
    and wide-expand calls are right either way"""
    monkeypatch.setenv("KETOGPU_LIST_BOUND_STEP", str(step))
    t = WR.Twin(WR.moves_rows())
    rw = t.rw
    s = WR.moves_starts(t)
    big = s["stars"][3]
    label, ins, dele, _ = WR.moves_script()[12]
    with lookup.Lookup(rw) as lk, lookup.Subjects(rw) as sj, expand.DeviceEngine(rw, subjects=sj) as dev:
        roots, xroots = [big, s["stars"][2], s["fill"]], [big, s["wl"], s["wp"]]
        WR.all_calls(rw, lk, sj, dev, roots, s["stars"][0], [s["a_user"], s["lstars"][3], s["small"]], [big],
                     "before the write", xroots, t)
        assert sj.wide_stats()["wide_requests"] > 0 and dev.expand_wide_stats()["mask_builds"] == 1
        n0 = rw.stats()["num_nodes"]
        assert sj.subject_ids_raw(np.array([n0], dtype=np.uint32), ANY, 16, wide=True)[1][0] == lookup.INVALID
        res = t.write(ins, dele)
        assert res["applied"] and res["new_nodes"] == 1
        new = members_of(rw, ins)[0]
        assert new == n0
        WR.all_calls(rw, lk, sj, dev, roots, s["stars"][0], [new, s["a_user"], s["lstars"][3]], [big], label, xroots, t)
        got = sj.subject_ids([big], ANY, wide=True)[0]
        assert len(got) == 2 * C + 2 and got[-1] == new
        page = sj.subject_page_raw([big], np.array([new], dtype=np.uint32), ANY, 50, wide=True)
        assert page[1][0] == 1 and page[0][0, 0] == new and page[3][0] == 1
        for h in (lk, sj):
            rs = h.refresh_stats()
            assert rs["patched_refreshes"] == 1 and rs["full_uploads"] == 1 and h.stats()["uploads"] == 2, rs
        assert dev.expand_wide_stats()["mask_builds"] == 2
        for h, raw in ((sj, sj.subject_ids_raw), (lk, lk.lookup_ids_raw)):
            _, begin, count, _ = raw(np.array([new, n0 + 1], dtype=np.uint32), ANY, 64, wide=True)
            assert begin[0] != lookup.INVALID and begin[1] == lookup.INVALID and count[1] == 0
