"""Depth-limited subject lists on the device (ketogpu_subjects_ids_depth / _page_depth,
keto_amd/csrc/depth.hpp): the tests of depth_gpu_suite.py over the subjects handle, both tier-2
finishes (the seen list and the scan), the synthetic workloads of test_subjects_gpu.py at
k = 1, 2 and 3, and the named calls."""
import pytest

from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import depth_cases as DC
from tests import test_subjects_gpu as TS
from tests.depth_gpu_suite import *  # noqa: F401,F403  (the shared tests and their fixtures)
from tests.depth_gpu_suite import check_chain, check_workload, u32

pytestmark = pytest.mark.gpu


@pytest.fixture
def side():
    return DC.SubjectsSide


def test_tier2_chain_finishes_by_scan_without_a_seen_list(side, tiers, monkeypatch):
    """KETOGPU_SUBJECTS_LIST_CAP=0: every tier-2 request finishes by the scan of the bitmap"""
    monkeypatch.setenv(side.list_cap_env, "0")
    snap = DC.structure(side.name)[0]
    with side.Handle(snap) as h:
        assert h.stats()["list_capacity"] == 0
        check_chain(side, h, "scan_finishes")


def test_seen_list_boundary(side, monkeypatch):
    """a seen list of 64 entries: M_k of 65 finishes by scan, of 64 and fewer by list"""
    monkeypatch.setenv(side.tier_env, "2")
    monkeypatch.setenv(side.list_cap_env, "64")
    snap, truth, v = DC.levels(side.name)
    ids = u32([v["w65"], v["chain"], v["w129"], v["w65"]])
    depth = u32([1, 4, 2, 2])
    want, wfr = truth.want(ids, depth)
    assert [len(w) for w in want] == [65, 4, 258, 130]
    with side.Handle(snap) as h:
        DC.assert_depth(side, h, ids, depth, DC.ANY, want, wfr)
        st = h.depth_stats()
        assert (st["list_finishes"], st["scan_finishes"]) == (1, 3)
        DC.assert_pages(side, h, ids, depth, None, DC.ANY, 7, want, wfr)
        st = h.depth_stats()
        assert (st["list_finishes"], st["scan_finishes"]) == (2, 6)
        DC.assert_depth(side, h, ids, depth, DC.ANY, want, wfr)  # both finishes left the slots clean


@pytest.mark.parametrize("kind", list(TS.WORKLOADS))
def test_synthetic_workloads_match_the_host_twins(kind, side, tiers):
    snap = TS.workload(kind)
    st = check_workload(side, tiers, snap, lookup.CLASS_SUBJECT_ID)
    assert st["list_finishes"] + st["scan_finishes"] == st["tier2_requests"]


def test_named_calls():
    snap, truth, v = DC.levels("subjects")
    host = lookup.HostSubjects(snap)
    root, nothing = ("n", "k5", "member"), ("n", "nothing", "member")
    with lookup.Subjects(snap) as sj:
        roots, depths = [root, root, root, nothing], [5, 6, lookup.DEPTH_ALL, 2]
        lists, complete = sj.list_subjects_depth_batch(roots, depths)
        assert (lists, complete) == host.list_subjects_depth_batch(roots, depths)
        assert lists == [[], [rt.SubjectID("uk")], [rt.SubjectID("uk")], []] and complete == [False, True, True, True]
        assert [s.object for s in sj.ListSubjects(*root, "any", max_depth=2)] == ["k3", "k4"]
        assert sj.ListSubjects(*root) == [rt.SubjectID("uk")]  # None: today's path
        assert sj.list_subjects_batch([root], "any", max_depth=1) == [[rt.SubjectSet("n", "k4", "member")]]
        assert sj.list_subjects_page(*root, "any", 2, "", max_depth=3) == \
            host.list_subjects_page(*root, "any", 2, "", max_depth=3)
        items, tok, total, complete = sj.list_subjects_page(*root, "any", 2, "", max_depth=3)
        assert len(items) == 2 and total == 3 and complete is False
        items, tok, total, complete = sj.list_subjects_page(*root, "any", 2, tok, max_depth=3)
        assert len(items) == 1 and tok == "" and complete is False
        assert len(sj.list_subjects_page(*root, "any", 2, "")) == 3
        st = sj.depth_stats()
        assert st["requests"] == 4 + 1 + 1 + 3 and sj.stats()["requests"] == 2
