"""The first stages that only KETOGPU_UNITS reaches: b16 (unit_kernel<16> -> <4> -> <1>) and
w4 / w8 / w16 (wave_unit_kernel, then unit_kernel<1>), forward-only with 4-byte column
entries.  The random tables of test_gpu_parity.py (wildcards, poisoned pages, ambiguous
keys: these kernels raise R4 flags themselves) and the mixed-width fan batch whose units
spill through every pass to the global path.  An unknown plan name is refused."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import fan_graph, randgraph

pytestmark = pytest.mark.gpu

PLANS = {"b16": 4, "w4": 3, "w8": 3, "w16": 3}  # -> the plan number the engine reports


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(params=list(PLANS))
def legacy_plan(request, monkeypatch):
    monkeypatch.setenv("KETOGPU_UNITS", request.param)
    return request.param


@pytest.mark.parametrize("seed,page_size,poison,collide,empty_ns,words", [
    (31, 100, False, False, False, 0), (32, 3, True, False, True, 0), (33, 2, True, True, False, 0),
    (34, 1, False, True, True, 0), (35, 100, False, False, False, 1), (36, 5, True, True, True, 2)])
def test_random_tables_match_oracle(seed, page_size, poison, collide, empty_ns, words, legacy_plan):
    namespaces, rows = randgraph.make_graph(seed, n_rows=600, n_obj=30, n_users=40, poison=poison, collide=collide,
                                            empty_ns=empty_ns)
    snap = Snapshot.from_rows(namespaces, rows, page_size=page_size, sort=True)
    eng = check.Engine(snap, max_words_per_round=words)
    orc = randgraph.oracle_store(namespaces, rows, page_size)
    reqs = randgraph.make_requests(seed, namespaces, rows, n=1000)
    got = eng.check_many([rt.InternalRelationTuple(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    want = orc.check_batch(reqs)
    bad = [(reqs[i], got[i], bool(want[i])) for i in range(len(reqs)) if got[i] != bool(want[i])]
    assert not bad, bad[:5]
    assert any(want) and not all(want)
    assert eng.last_stats()["plan"] == PLANS[legacy_plan]


WIDTHS = fan_graph.WIDTHS


@pytest.fixture(scope="module")
def mixed():
    snap = Snapshot.from_rows([("n", 1)], fan_graph.fan_rows(WIDTHS), sort=True)
    reqs, want = fan_graph.mixed_batch(WIDTHS)
    return (snap,) + snap.resolve_many(reqs) + (want,)


def test_mixed_units(mixed, legacy_plan):
    """units that hold small and huge requests: resident three times, then a pinned host batch"""
    snap, r, t, want = mixed
    eng = check.Engine(snap)
    q = eng.upload(r, t)
    for _ in range(3):
        q.run()
        ab, fb = q.download_words()
        np.testing.assert_array_equal(check.unpack_bits(ab, len(r)), want)
        assert int(ab[-1]) >> (len(r) % 64) == 0 and not fb.any()
    st = eng.last_stats()
    assert st["plan"] == PLANS[legacy_plan] and st["spilled_units"] > 0
    pr, pt = check.pinned(r), check.pinned(t)
    out = check.PinnedBuffer((len(r) + 63) // 64, np.uint64)
    eng.check_ids_raw(pr.array.ctypes.data, pt.array.ctypes.data, len(r), out.array.ctypes.data)
    np.testing.assert_array_equal(check.unpack_bits(out.array.copy(), len(r)), want)


@pytest.mark.parametrize("name", ["b32", "bidi2", "LITE", "w2", "lite,core"])
def test_unknown_plan_is_refused(name, monkeypatch):
    monkeypatch.setenv("KETOGPU_UNITS", name)
    snap = Snapshot.from_rows([("n", 1)], [(1, "o", "r", "u", None, None, None)])
    with pytest.raises(L.KetoError) as e:
        check.Engine(snap)
    assert e.value.code == L.EINVAL and "KETOGPU_UNITS" in str(e.value)
    monkeypatch.delenv("KETOGPU_UNITS")
    assert check.Engine(snap).check_many([rt.InternalRelationTuple("n", "o", "r", rt.SubjectID("u"))]) == [True]
