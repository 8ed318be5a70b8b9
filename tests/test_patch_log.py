"""The patch log of a writable snapshot as the listing handles read it (include/ketogpu.h
"listing handles and in-place writes"): every committed write names the reverse rows
(KETOGPU_PATCH_REVERSE) and the full forward rows (KETOGPU_PATCH_FORWARD_FULL) it rewrote, a
refused write names nothing, the log is kept for its slowest reader, and the derived type and
class indexes, which now survive a write instead of being rebuilt, still answer like a snapshot
rebuilt from the final rows.  No GPU."""
import pytest

from keto_amd import _lib as L
from keto_amd import lookup as LK
from tests import refresh_cases as RC


def _one_hop(snap, n_nodes):
    """the depth-1 answers of both host listings for every node id below n_nodes"""
    subj = [tuple(LK.host_subjects_depth(snap, v, 1)[0]) for v in range(n_nodes)]
    look = [tuple(LK.host_lookup_depth(snap, v, 1)[0]) for v in range(n_nodes)]
    return subj, look


def _run(snap, writes, on_write):
    """the series against `snap`: on_write(k, result, refused) after every write"""
    for k in range(RC.Writes.COUNT):
        ins, dele, refused = writes.write(k)
        res = snap.write(ins, dele)
        if res["applied"]:
            writes.applied(ins, dele)
        on_write(k, res, refused)


def test_log_covers_every_row_whose_answer_changed():
    snap = RC.snapshot(RC.base_rows())
    writes = RC.Writes(RC.base_rows())
    reader = snap.patch_reader()
    state = {"before": _one_hop(snap, snap.stats()["num_nodes"]), "applied": 0, "refused": 0, "new": 0, "kinds": set()}

    def check(k, res, refused):
        entries = reader.read()
        if not res["applied"]:
            assert entries == [], f"write {k} was refused ({res['reason']}) and logged {entries}"
            state["refused"] += 1
            assert not (k in (10, 12))  # the scripted writes are representable
            return
        assert not refused, f"write {k} should have been refused"
        state["applied"] += 1
        state["new"] += res["new_nodes"]
        state["kinds"] |= {kind for kind, _ in entries}
        n = snap.stats()["num_nodes"]
        subj0, look0 = state["before"]
        subj1, look1 = _one_hop(snap, n)
        pad = lambda a: a + [()] * (n - len(a))  # a new node answered nothing before
        full = {v for kind, v in entries if kind == L.PATCH_FORWARD_FULL}
        rev = {v for kind, v in entries if kind == L.PATCH_REVERSE}
        assert {v for v in range(n) if pad(subj0)[v] != subj1[v]} <= full, f"write {k}"
        assert {v for v in range(n) if pad(look0)[v] != look1[v]} <= rev, f"write {k}"
        # the engine's count of device rows does not see the new kind
        assert res["device_rows"] == sum(kind != L.PATCH_FORWARD_FULL for kind, _ in entries)
        assert len(full) == res["groups_touched"]
        state["before"] = (subj1, look1)

    _run(snap, writes, check)
    assert state["applied"] >= 45 and state["refused"] >= 3 and state["new"] >= 5
    assert state["kinds"] == {L.PATCH_FORWARD_INTERIOR, L.PATCH_REVERSE, L.PATCH_FORWARD_FULL}
    emptied = RC.node_of(snap, RC.rt.SubjectSet("groups", RC.EMPTIED, "member"))
    assert len(LK.host_subjects_depth(snap, emptied, 1)[0]) == 4  # deleted to empty, filled again


def test_refused_write_logs_nothing():
    snap = RC.snapshot(RC.base_rows())
    reader = snap.patch_reader()
    start = reader.position()
    res = snap.write([RC.user_row("no_such_group", "u1")], [])
    assert not res["applied"] and res["reason"] == "class"
    res = snap.write([(1, "g3", "member", None, 2, "d4", "viewer")], [])
    assert not res["applied"]
    assert reader.read() == [] and reader.position() == start
    # a reader of a snapshot that cannot be written never sees an entry
    fixed = RC.snapshot(RC.base_rows(), writable=False)
    r2 = fixed.patch_reader()
    assert not fixed.write([RC.user_row("g1", "zed")], [])["applied"]
    assert r2.read() == []


def test_slow_reader_keeps_the_log_and_free_releases_it():
    snap = RC.snapshot(RC.base_rows())
    slow, fast = snap.patch_reader(), snap.patch_reader()
    seen = []
    for k in range(5):
        assert snap.write([RC.user_row(f"g{k}", f"late{k}")], [])["applied"]
        seen += fast.read()
        pos, lo, hi = slow.position()
        assert lo == pos and hi == fast.position()[0]  # kept from the slow reader on, and no further back
    assert len(seen) >= 10
    assert slow.read(chunk=3) == seen  # every entry, in write order, across several calls
    slow.close()
    assert snap.write([RC.user_row("g9", "late9")], [])["applied"]
    pos, lo, hi = fast.position()
    assert lo == pos < hi  # trimmed up to the reader that is left
    fast.read()
    fast.close()
    assert snap.write([RC.user_row("g10", "late10")], [])["applied"]
    late = snap.patch_reader()
    pos, lo, hi = late.position()
    assert pos == lo == hi  # without readers the log is trimmed whole at the end of a write
    assert late.read() == []


def test_reader_outlives_its_snapshot():
    snap = RC.snapshot(RC.base_rows())
    reader = snap.patch_reader()
    reader.snapshot = None
    del snap
    with pytest.raises(L.KetoError):
        reader.read()
    reader.close()  # touches nothing of the freed snapshot


def _class_name(snap, cls, types):
    if cls in (L.CLASS_SUBJECT_ID, L.CLASS_UNTYPED_SET, L.TYPE_NONE):
        return cls
    return types[cls]


def test_types_and_classes_after_writes_equal_a_rebuild():
    base = RC.base_rows()
    snap = RC.snapshot(base)
    writes = RC.Writes(base)
    pairs = [(ns, rel) for ns, rel in (("groups", "member"), ("docs", "viewer"), ("docs", "owner"), ("docs", "member"))]
    first = {p: snap.type_id(*p) for p in pairs}
    classes_seen = []
    # (asking between the writes makes the indexes live through them: each answer comes from
    # the index built before the first write, extended by the nodes the writes added)
    _run(snap, writes, lambda k, res, refused: classes_seen.append(snap.subject_class(0)))
    final = sorted(writes.rows, key=repr)
    rebuilt = RC.snapshot(base, writable=False).apply(
        [r for r in final if r not in set(base)], [r for r in base if r not in writes.rows])
    assert {p: snap.type_id(*p) for p in pairs} == first  # type ids are stable for a snapshot's life
    names = {}
    for s in (snap, rebuilt):
        names[s] = {s.type_id(*p): p for p in pairs if s.type_id(*p) != L.TYPE_NONE}
    assert set(names[snap].values()) == set(names[rebuilt].values())
    compared = 0
    for label, subject in RC.node_names():
        a, b = RC.node_of(snap, subject), RC.node_of(rebuilt, subject)
        if b == L.NODE_NONE:
            continue  # (a writable snapshot keeps the node of a subject whose last row went)
        assert a != L.NODE_NONE, label
        ca = _class_name(snap, snap.subject_class(a), names[snap])
        cb = _class_name(rebuilt, rebuilt.subject_class(b), names[rebuilt])
        assert ca == cb, label
        compared += 1
    assert compared >= RC.N_GROUPS + 2 * RC.N_DOCS + RC.N_USERS // 2  # every set, and most of the users
    n = snap.stats()["num_nodes"]
    with pytest.raises(L.KetoError):
        snap.subject_class(n)
    assert snap.subject_class(n - 1) == L.CLASS_SUBJECT_ID  # the last node a write added
