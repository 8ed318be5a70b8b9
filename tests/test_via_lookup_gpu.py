"""Object lists that say why, on the device (ketogpu_lookup_ids_via / _page_via,
keto_amd/csrc/via.hpp): the tests of via_gpu_suite.py over the lookup handle, the synthetic
workloads of test_lookup_gpu.py at k = 1, 2, 3 and mixed, and the named calls."""
import pytest

from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import depth_cases as DC
from tests import test_lookup_gpu as TL
from tests import via_cases as VC
from tests.via_gpu_suite import *  # noqa: F401,F403  (the shared tests and their fixtures)
from tests.via_gpu_suite import check_workload

pytestmark = pytest.mark.gpu


@pytest.fixture
def side():
    return VC.LookupSide


@pytest.mark.parametrize("kind", list(TL.WORKLOADS))
def test_synthetic_workloads_match_the_host_twins(kind, side, tiers):
    snap = TL.workload(kind)
    ty = snap.type_id(*TL.WORKLOADS[kind][1][0])
    assert ty not in (lookup.TYPE_NONE, lookup.TYPE_ANY)
    st = check_workload(side, tiers, snap, ty)
    assert st["list_finishes"] == st["scan_finishes"] == 0  # the lookup handle has no seen list
    if tiers == "default":
        assert st["tier1_requests"] > 0


def test_named_calls():
    snap, truth, v = DC.levels("lookup")
    uk, nobody = rt.SubjectID("uk"), rt.SubjectID("nobody")
    host = lookup.HostLookup(snap)
    group = lambda i: rt.SubjectSet("n", f"k{i}", "member")
    with lookup.Lookup(snap) as lk:
        want = [(f"k{i}", uk if i == 0 else group(i - 1), i + 1) for i in range(6)]
        assert lk.ListObjects("n", "member", uk, with_via=True) == want
        assert lk.ListObjects("n", "member", uk, max_depth=2, with_via=True) == want[:2]
        assert lk.ListObjects("n", "member", uk) == [f"k{i}" for i in range(6)]  # False: today's path
        assert lk.list_objects_batch("n", "member", [uk, nobody], with_via=True) == [want, []]
        assert lk.list_objects_batch("n", "member", [uk, nobody], with_via=True) == \
            host.list_objects_via_batch("n", "member", [uk, nobody])
        assert lk.list_objects_page("n", "member", uk, 4, "", with_via=True) == \
            host.list_objects_page("n", "member", uk, 4, "", with_via=True)
        items, tok, total = lk.list_objects_page("n", "member", uk, 4, "", with_via=True)
        assert items == want[:4] and total == 6
        items, tok, total, complete = lk.list_objects_page("n", "member", uk, 4, tok, max_depth=5, with_via=True)
        assert items == want[4:5] and tok == "" and total == 5 and complete is False
        assert lk.list_objects_batch("nowhere", "member", [uk], with_via=True) == [[]]
        st = lk.via_stats()
        assert st["requests"] == 1 + 1 + 2 + 2 + 1 + 1 + 1 and lk.stats()["requests"] == 1
        assert lk.depth_stats()["requests"] == 0
