"""The fixtures of the writable-snapshot GPU tests (tests/writable_cases.py), proved on the CPU:
every fixture's host lists and trees on the writable snapshot equal the read-only snapshot's
through the id map; every scripted write applies (or is refused as the script says) and the row
table's mirror agrees with the snapshot after the last one; and the sizes each GPU scenario relies
on hold, recomputed from the snapshot by the formulas of ListHandle::try_patch and the two
upload() functions (writable_cases.HandleModel), with a factor 2 to spare at every backlog
threshold.  A fixture that drifts fails here, not silently on the GPU."""
import numpy as np
import pytest

from keto_amd import expand, lookup
from tests import expand_wide_cases as WC
from tests import refresh_cases as RC
from tests import test_list_refresh_gpu as RG
from tests import writable_cases as WR

SIDES = ("subjects", "lookup")


def every_start(t, starts):
    """the named starts, the placeholders, and ids next to them"""
    return np.array(sorted(set(int(s) for s in starts) | set(t.placeholders())), dtype=np.uint32)


# ---------------------------------------------------------------------- the layout, no writes
def test_three_placeholders_shift_every_id_and_the_map_keeps_the_order():
    for t in [WR.boundary_twin(s, w)[0] for s in SIDES for w in ("chunk", "set")] + \
            [WR.depth_twin(s)[0] for s in SIDES] + [WR.wide_expand_twin()]:
        rw, ro = t.rw.stats(), t.ro.stats()
        assert rw["num_nodes"] == ro["num_nodes"] + 3 and rw["num_expandable"] == ro["num_expandable"] + 3
        assert len(t.placeholders()) == 3
        m = t.to_ro
        real = m[m != WR.INVALID]
        assert len(real) == ro["num_nodes"] and (np.diff(real.astype(np.int64)) > 0).all()
        assert t.n_cap - rw["num_nodes"] >= 1024
        assert (t.map(WR.non_nodes(t)) == WR.INVALID).all()


@pytest.mark.parametrize("which", ["chunk", "set"])
@pytest.mark.parametrize("side", SIDES)
def test_boundary_graphs_equal_the_read_only_ones(side, which):
    t, starts = WR.boundary_twin(side, which)
    ids = every_start(t, starts.values())
    n = WR.host_equal(t, ids if side == "subjects" else [], ids if side == "lookup" else [], depths=(1, WR.ALL))
    assert n == len(starts)
    S = WR.W.SIDES[side]
    for name, v in starts.items():  # the sizes the GPU cases are named for
        assert len(S.host(t.rw, [v])[0]) == int(name.lstrip("starsplit")), name


@pytest.mark.parametrize("side", SIDES)
def test_depth_graphs_equal_the_read_only_ones(side):
    t, starts = WR.depth_twin(side)
    ids = every_start(t, starts)
    assert WR.host_equal(t, ids if side == "subjects" else [], ids if side == "lookup" else []) == len(starts)
    S = WR.W.SIDES[side]
    deep = lookup.host_subjects_via if side == "subjects" else lookup.host_lookup_via
    assert max(max(deep(t.rw, int(x))[2]) for x in starts[:3]) == 5  # the joined chains: members 5 hops away
    assert len(S.host(t.rw, [starts[3]])[0]) == WR.CHUNK + 1


def test_wide_expand_graph_equals_the_read_only_one():
    t = WR.wide_expand_twin()
    roots = WC.roots(t.rw)
    assert len(roots) == len(WC.root_names()) == 148 and np.array_equal(t.map(roots), WC.roots(t.ro))
    WR.trees_equal(t, roots)
    assert t.rw.stats()["num_wildcard_nodes"] == 1 and t.rw.stats()["num_bad_rows"] == 1
    assert t.write([WR.LC.sid("wfan_a_g", "member", "one more")])["reason"] == "wildcard"  # static: no write applies


# ---------------------------------------------------------------------- rows that move
def test_the_moves_script_applies_and_moves_what_it_says():
    t = WR.Twin(WR.moves_rows())
    s = WR.moves_starts(t)
    C = WR.CHUNK
    ex = expand.Engine(t.rw)
    sj, lk = WR.HandleModel(t.rw, "subjects", t.n0), WR.HandleModel(t.rw, "lookup", t.n0)
    tail0 = sj.tail
    assert tail0 % 64 != 0  # the first row that moves begins off a 64-word boundary
    assert [WR.row_len(ex, v) for v in (s["stars"][0], s["wl"], s["wp"], s["wp_child"])] == [C - 1, 4095, 300, 1]
    assert WR.rev_row_words(t.rw, s["small"]) == 3 and WR.rev_row_words(t.rw, s["lstars"][0]) == C - 1 + 2 + (C - 1) // 8
    want_len = {0: (s["stars"][0], C + 1), 1: (s["stars"][0], C + 601), 2: (s["wl"], 4096), 3: (s["wl"], 4097),
                4: (s["wl"], 5197), 5: (s["wp"], 380), 6: (s["wp_child"], 2), 7: (s["stars"][0], C - 1),
                8: (s["stars"][0], C), 13: (s["wp64"], 379)}
    moved = {1: s["stars"][0], 4: s["wl"], 5: s["wp"]}
    applied = 0
    for k, (label, ins, dele, expect) in enumerate(WR.moves_script()):
        res = t.write(ins, dele)
        assert res["reason"] == expect, (label, res)
        if not res["applied"]:
            assert sj.refresh() is None and lk.refresh() is None
            continue
        applied += 1
        before = sj.stats["rows_moved"]
        assert sj.refresh() == "patch" and lk.refresh() == "patch", label
        assert sj.stats["rows_moved"] - before == (1 if k in moved else 0), label
        if k in want_len:
            v, n = want_len[k]
            assert WR.row_len(expand.Engine(t.rw), v) == n, label
    assert applied == 13 and sj.margin >= 2 and lk.margin >= 2, (sj.margin, lk.margin)
    assert sj.moved_at[s["stars"][0]] == tail0  # m_begin of the first moved row: the arena's tail before it
    assert sj.moved_at[s["wl"]] == tail0 + (C + 601) + (C + 601) // 4 + 4
    assert sj.cap[s["wp64"]] == 379  # the last write fills WP64's room to the word
    assert 5197 > WC.WINDOW + 1024  # at the tail: one run past the window, with fill items of 1024 behind it
    for m in (sj, lk):
        assert m.stats == dict(full_uploads=1, patched_refreshes=13, rows_moved=3 if m is sj else 0, compactions=0,
                               fallbacks_backlog=0, fallbacks_trimmed=0)
        m.close()
    # the mirror and the snapshot agree
    assert t.rw.stats()["num_rows"] == t.ro.stats()["num_rows"] == len(t.rows)
    roots = s["stars"] + [s["wl"], s["wl96"], s["wp"], s["wp64"], s["wp_child"], s["fill"], s["wres"]]
    targets = s["lstars"] + [s["small"], s["a_user"], s["fill_user"]]
    WR.host_equal(t, roots, targets, depths=(1, WR.ALL))
    WR.trees_equal(t, roots)


# ---------------------------------------------------------------------- placeholders as expand roots
def test_a_placeholder_expands_to_the_nil_tree():
    """the host twin's answer on its own: a placeholder stands for no subject, at any depth; a
    reserved id is no node"""
    rw, ro, to_ro = WR.twin(WR.depth_rows("subjects"))
    ex = expand.Engine(rw)
    holes = [v for v in range(rw.stats()["num_expandable"]) if WR.is_placeholder(rw, v)]
    assert len(holes) == 3 and (to_ro[holes] == WR.INVALID).all()
    for v in holes:
        for d in (1, 2, 3, WR.EC.ALL):
            nodes, kids, flags = ex.expand_ids(v, d)
            assert len(nodes) == 0 and len(kids) == 0 and flags == 0, (v, d)
            assert WR.EC.twin(ex, v, d)[0] == WR.L.EXPAND_NIL
    with pytest.raises(WR.L.KetoError):
        ex.expand_ids(rw.stats()["num_nodes"], 2)
    assert len(to_ro) == rw.stats()["num_nodes"] == ro.stats()["num_nodes"] + 3


# ---------------------------------------------------------------------- fallbacks
def rc_twin(rows):
    return WR.Twin(rows, RC.NAMESPACES)


def models(snap, **kw):
    return WR.HandleModel(snap, "subjects", **kw), WR.HandleModel(snap, "lookup", **kw)


def spare(*ms):
    """every backlog threshold these models met was missed or passed by a factor 2 at least"""
    for m in ms:
        assert m.margin is not None and m.margin >= 2, (m.kind, m.margin)


FB_USERS = ("w0", "w17", "u1")


def test_one_large_write_passes_both_backlog_thresholds():
    t = rc_twin(WR.fb_rows())
    WR.rc_equal(t, FB_USERS)
    sj, lk = models(t.rw)
    assert t.write(WR.fb_large_write())["applied"]
    assert sj.refresh() == "backlog" and lk.refresh() == "backlog"
    spare(sj, lk)
    assert t.write(WR.fb_small_write())["applied"]
    assert sj.refresh() == "patch" and lk.refresh() == "patch"
    spare(sj, lk)
    for m in (sj, lk):
        assert m.stats["full_uploads"] == 2 and m.stats["fallbacks_backlog"] == 1 and m.stats["patched_refreshes"] == 1
    WR.rc_equal(t, FB_USERS)


def test_small_writes_pass_the_thresholds_only_together():
    t = rc_twin(WR.fb_rows())
    busy, idle = models(t.rw), models(t.rw)
    for k, ins in enumerate(WR.fb_idle_writes()):
        assert t.write(ins)["applied"], k
        assert [m.refresh() for m in busy] == ["patch", "patch"], k
    assert [m.refresh() for m in idle] == ["backlog", "backlog"]
    spare(*busy, *idle)
    for m in busy + idle:
        assert m.stats["compactions"] == 0
    assert busy[0].stats["patched_refreshes"] == 15 and busy[0].stats["rows_moved"] == 15
    assert t.write(WR.fb_small_write())["applied"]
    assert [m.refresh() for m in busy + idle] == ["patch"] * 4
    WR.rc_equal(t, FB_USERS)


def test_the_growth_rows_are_the_growth_snapshot():
    a, b = WR.Twin(WR.growth_rows(), RC.NAMESPACES).rw, RG.growth_snapshot()
    sa, sb = a.stats(), b.stats()
    sa.pop("build_seconds"), sb.pop("build_seconds")
    assert sa == sb
    ga, gb = a.graph(), b.graph()
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)


@pytest.mark.parametrize("slack", [0, 20])
def test_the_growth_snapshot_exhausts_its_tail(slack):
    t = rc_twin(WR.growth_rows())
    grow = RC.node_of(t.rw, lookup.SubjectSet("groups", "grow", "member"))
    WR.rc_equal(t, more_roots=[grow])
    sj, lk = WR.HandleModel(t.rw, "subjects", slack=slack), WR.HandleModel(t.rw, "lookup")
    k, got = 0, []
    for n in (1, 7, 30) if slack else (1, 7, 2):
        assert t.write([RC.user_row("grow", f"m{k + i}") for i in range(n)], [])["applied"]
        k += n
        got.append(sj.refresh())
        assert lk.refresh() == "patch"
    assert got == (["patch", "patch", "compaction"] if slack else ["patch", "compaction", "patch"])
    assert sj.stats["compactions"] == 1 and sj.stats["rows_moved"] == (1 if slack else 0)
    assert t.write(WR.fb_small_write())["applied"]
    assert sj.refresh() == "patch" and lk.refresh() == "patch"
    spare(sj, lk)
    WR.rc_equal(t, more_roots=[grow])


def test_garbage_passes_the_knob_at_the_second_move():
    t = rc_twin(WR.garbage_rows())
    grow = RC.node_of(t.rw, lookup.SubjectSet("groups", "grow", "member"))
    WR.rc_equal(t, more_roots=[grow])
    sj, lk = models(t.rw, garbage=WR.GARBAGE_KNOB)
    got = []
    for ins in WR.garbage_writes():
        assert t.write(ins)["applied"]
        got.append((sj.refresh(), lk.refresh()))
    assert got == [("patch", "patch"), ("compaction", "patch"), ("patch", "patch")]
    assert sj.stats["rows_moved"] == 2 and sj.stats["compactions"] == 1 and sj.stats["full_uploads"] == 2
    spare(sj, lk)
    WR.rc_equal(t, more_roots=[grow])
    # without the knob the default bound, 2^20 words at this size, is out of reach
    plain = WR.HandleModel(RC.snapshot(WR.garbage_rows()), "subjects")
    assert max(plain.snap.stats()["num_edges"] // 4, 1 << 20) > 100 * plain.tail


def test_one_life_has_every_outcome():
    t = rc_twin(WR.life_rows())
    WR.rc_equal(t)
    sj = WR.HandleModel(t.rw, "subjects", slack=int(WR.LIFE_KNOBS["KETOGPU_LIST_ARENA_SLACK"]),
                        garbage=int(WR.LIFE_KNOBS["KETOGPU_LIST_ARENA_GARBAGE"]))
    lk = WR.HandleModel(t.rw, "lookup")
    seen, applied = [], 0
    for label, ins, dele, refused, writes in WR.life_writes(t.rows):
        res = t.write(ins, dele)
        assert not (refused and res["applied"]), label
        if not res["applied"]:
            continue
        writes.applied(ins, dele)
        applied += 1
        seen.append(sj.refresh())
        assert lk.refresh() == "patch"
    assert writes.rows == t.rows  # the series' own mirror and the twin's
    assert seen[-2:] in (["patch", "compaction"], ["compaction", "patch"])
    for k in ("patched_refreshes", "rows_moved", "compactions"):
        assert sj.stats[k] > 0, sj.stats
    assert sj.stats["full_uploads"] - 1 > 0 and sj.uploads == lk.uploads == 1 + applied
    assert sj.stats["fallbacks_backlog"] == 0 and lk.stats["full_uploads"] == 1
    spare(sj, lk)
    d12 = [RC.node_of(t.rw, lookup.SubjectSet("docs", d, "viewer")) for d in ("d1", "d2")]
    WR.rc_equal(t, more_roots=d12)
