"""The wide tier on the lookup handle (ketogpu_lookup_ids_wide): wide_gpu_suite.py's checks over
the reverse rows, and in-place writes, which this handle patches where the rows lie."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import lookup
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import wide_gpu_suite as W

pytestmark = pytest.mark.gpu
S = W.LOOKUP
ANY = lookup.TYPE_ANY


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


def test_none_and_invalid_targets(forced, monkeypatch):
    W.check_starts(S, forced, monkeypatch)


def test_writes_are_seen_by_the_next_wide_call(monkeypatch):
    """test_lookup_gpu.py's scenario through wide=True"""
    S.force(monkeypatch)
    rows = [LC.sid("g", "member", "alice"), LC.sset("doc1", "view", "g", "member"), LC.sid("h", "member", "bob"),
            LC.sid("doc3", "view", "bob")]
    rows += [LC.sset(f"h{i}", "view", "h", "member") for i in range(40)]
    snap = Snapshot.from_rows(LC.NS1, rows, writable=True)
    alice = rt.SubjectID("alice")
    objects = lambda lk, s: lk.ListObjects("n", "view", s, wide=True)
    with lookup.Lookup(snap) as lk:
        assert objects(lk, alice) == ["doc1"]
        assert snap.write([LC.sid("h", "member", "alice")])["applied"]
        assert objects(lk, alice) == sorted(["doc1"] + [f"h{i}" for i in range(40)])
        assert snap.write([LC.sid("h", "member", "carol")])["applied"]  # a new subject (reserved id)
        assert len(objects(lk, rt.SubjectID("carol"))) == 40
        assert snap.write((), [LC.sid("g", "member", "alice")])["applied"]  # a deleted row disappears
        assert objects(lk, alice) == sorted(f"h{i}" for i in range(40))
        assert lk.stats()["uploads"] == 4
        real = []
        for v in range(snap.stats()["num_nodes"]):  # every node but the placeholders, as the host lists them
            try:
                snap.describe(v)
                real.append(v)
            except L.KetoError:
                pass
        real = np.array(real, dtype=np.uint32)
        W.assert_call_matches(S, lk, real, ANY, S.host(snap, real))
        assert lk.wide_stats()["wide_requests"] > 0 and lk.stats()["uploads"] == 4
