"""The wide tier on the subjects handle (ketogpu_subjects_ids_wide): wide_gpu_suite.py's checks
over the forward rows, and what only this handle has: a forward row that holds a subject twice,
and in-place writes into the arena."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC
from tests import wide_gpu_suite as W

pytestmark = pytest.mark.gpu
S = W.SUBJECTS
ANY, IDS = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    W.need_gpu()


@pytest.fixture(params=[False, True], ids=["default", "forced"])
def forced(request):
    return request.param


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables(case, forced, monkeypatch):
    W.check_truth_table(S, case, forced, monkeypatch)


def test_structure_cases(monkeypatch):
    W.check_structure(S, monkeypatch)


def test_chunk_boundaries(monkeypatch):
    W.check_chunk_boundaries(S, monkeypatch)


def test_a_subject_twice_in_one_row(monkeypatch):
    S.force(monkeypatch)
    rows = SC.fwd_star_rows("d", 70, "u") + [LC.sid("d", "view", "u3"), LC.sid("d", "view", "u69"),
                                             LC.sset("d", "view", "g", "member"), LC.sid("g", "member", "u3")]
    snap = Snapshot.from_rows(LC.NS1, rows)
    assert snap.stats()["num_edges"] == len(rows)  # the forward rows keep both copies
    r = lookup.resolve_roots(snap, [("n", "d", "view")])
    with lookup.Subjects(snap) as sj:
        want = W.assert_call_matches(S, sj, r, ANY, S.host(snap, r))
        assert len(want[0]) == 71  # 70 users and the group: every id once
        out, begin, count, needed = sj.subject_ids_raw(r, IDS, 0, wide=True)  # count only: exact
        assert needed == 70 and count[0] == 70


def test_set_boundary():
    W.check_set_boundary(S)


@pytest.mark.parametrize("kind", list(W.WORKLOADS))
def test_synthetic_workloads(kind):
    W.check_workload(S, kind)


@pytest.mark.parametrize("slots", [1, 2])
def test_rounds_and_repeated_calls(slots, monkeypatch):
    W.check_rounds(S, slots, monkeypatch)


def test_plain_and_wide_calls_share_the_bitmaps(monkeypatch):
    W.check_plain_wide_plain(S, monkeypatch)


def test_truncation_protocol(forced, monkeypatch):
    W.check_truncation(S, forced, monkeypatch)


def test_none_leaf_and_invalid_roots(forced, monkeypatch):
    W.check_starts(S, forced, monkeypatch)


def test_writes_are_seen_by_the_next_wide_call(monkeypatch):
    """test_subjects_gpu.py's scenario through wide=True, and a row that outgrows its arena slot"""
    S.force(monkeypatch)
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
            LC.sset("doc2", "view", "h", "member"), LC.sid("doc3", "view", "bob")]
    rows += [LC.sid("h", "member", f"m{i}") for i in range(40)]
    rows += SC.fwd_star_rows("big", 3000, "f_")  # bulk: a patched row stays small against a full upload
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    members = sorted(["bob"] + [f"m{i}" for i in range(40)])
    users = lambda sj, d: [s.id for s in sj.ListSubjects("n", d, "view", wide=True)]
    with lookup.Subjects(snap) as sj:
        assert users(sj, "doc1") == ["alice"] and users(sj, "doc2") == members
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert users(sj, "doc2") == sorted(members + ["alice"])
        assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (the bound may move)
        assert users(sj, "doc2") == sorted(members + ["alice", "carol"])
        assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]  # a deleted row disappears
        assert users(sj, "doc1") == [] and users(sj, "doc2") == sorted(members + ["alice", "carol"])
        assert sj.stats()["uploads"] == 4
        before = sj.refresh_stats()
        more = [f"f_{i}" for i in range(30)]  # 43 entries had room for 55: the row moves to the arena's tail
        assert snap.write([LC.sid("h", "member", u) for u in more])["applied"]
        assert users(sj, "doc2") == sorted(members + ["alice", "carol"] + more)
        after = sj.refresh_stats()
        assert after["rows_moved"] == before["rows_moved"] + 1 and after["full_uploads"] == before["full_uploads"]
        real = []
        for v in range(snap.stats()["num_nodes"]):  # every node but the placeholders, as the host lists them
            try:
                snap.describe(v)
                real.append(v)
            except L.KetoError:
                pass
        real = np.array(real, dtype=np.uint32)
        W.assert_call_matches(S, sj, real, ANY, S.host(snap, real))
        st = sj.wide_stats()
        assert st["wide_requests"] > 0 and st["tier1_requests"] + st["wide_requests"] <= st["requests"]
