"""Subject lists that say why, on the device (ketogpu_subjects_ids_via / _page_via,
keto_amd/csrc/via.hpp): the tests of via_gpu_suite.py over the subjects handle, both tier-2
finishes (the seen list and the scan), the synthetic workloads of test_subjects_gpu.py at
k = 1, 2, 3 and mixed, and the named calls."""
import pytest

from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import depth_cases as DC
from tests import test_subjects_gpu as TS
from tests import via_cases as VC
from tests.via_gpu_suite import *  # noqa: F401,F403  (the shared tests and their fixtures)
from tests.via_gpu_suite import check_chain, check_workload, u32

pytestmark = pytest.mark.gpu


@pytest.fixture
def side():
    return VC.SubjectsSide


def test_the_chain_through_the_scan_finish(side, monkeypatch):
    """the other tier-2 finish: a seen list of 100 entries does not hold the chain"""
    monkeypatch.setenv(side.list_cap_env, "100")
    snap, _, truth, v = DC.structure(side.name)
    chk = VC.Checker(side, snap, truth)
    with side.Handle(snap) as h:
        check_chain(side, h, chk, v)
        st = h.via_stats()
        assert st["scan_finishes"] == 4 and st["list_finishes"] == 0 and st["tier2_requests"] == 4


def test_seen_list_boundary(side, monkeypatch):
    """a seen list of 64 entries: M_k of 65 finishes by scan, of 64 and fewer by list"""
    monkeypatch.setenv(side.tier_env, "2")
    monkeypatch.setenv(side.list_cap_env, "64")
    snap, truth, v = DC.levels(side.name)
    chk = VC.Checker(side, snap, truth)
    ids = u32([v["w65"], v["chain"], v["w129"], v["w65"]])
    depth = u32([1, 4, 2, 2])
    with side.Handle(snap) as h:
        lists = VC.assert_via(side, h, chk, ids, depth)
        assert [len(m[0]) for m in lists] == [65, 4, 258, 130]
        st = h.via_stats()
        assert (st["list_finishes"], st["scan_finishes"]) == (1, 3)
        out, via, hops, returned, count, remaining, fr = side.page(h, ids, depth, None, VC.ANY, 7)
        for k, (m, mv, mh) in enumerate(lists):
            r = int(returned[k])
            assert r == min(7, len(m)) and (out[k, :r] == m[:7]).all() and (hops[k, :r] == mh[:7]).all()
            assert all(chk.edge(via[k, j], out[k, j]) for j in range(r))
        st = h.via_stats()
        assert (st["list_finishes"], st["scan_finishes"]) == (2, 6)


@pytest.mark.parametrize("kind", list(TS.WORKLOADS))
def test_synthetic_workloads_match_the_host_twins(kind, side, tiers):
    snap = TS.workload(kind)
    st = check_workload(side, tiers, snap, lookup.CLASS_SUBJECT_ID)
    assert st["list_finishes"] + st["scan_finishes"] == st["tier2_requests"]
    if tiers == "default":
        assert st["tier1_requests"] > 0


def test_named_calls():
    snap, truth, v = DC.levels("subjects")
    host = lookup.HostSubjects(snap)
    group = lambda i: rt.SubjectSet("n", f"k{i}", "member")
    root = ("n", "k5", "member")
    with lookup.Subjects(snap) as sj:
        assert sj.ListSubjects(*root, with_via=True) == [(rt.SubjectID("uk"), group(0), 6)]
        assert sj.ListSubjects(*root) == [rt.SubjectID("uk")]  # False: today's path
        want = [(group(i), group(i + 1), 5 - i) for i in range(5)]
        assert sj.ListSubjects(*root, kind="any", max_depth=5, with_via=True) == want
        assert sj.list_subjects_batch([root], "any", 2, with_via=True) == [want[3:]] == \
            host.list_subjects_via_batch([root], "any", 2)
        assert sj.list_subjects_page(*root, "any", 4, "", with_via=True) == \
            host.list_subjects_page(*root, "any", 4, "", with_via=True)
        items, tok, total, complete = sj.list_subjects_page(*root, "any", 4, "", max_depth=3, with_via=True)
        assert sorted(h for _, _, h in items) == [1, 2, 3] and total == 3 and tok == "" and complete is False
        st = sj.via_stats()
        assert st["requests"] == 5 and sj.stats()["requests"] == 1 and sj.depth_stats()["requests"] == 0
