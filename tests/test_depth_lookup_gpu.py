"""Depth-limited object lists on the device (ketogpu_lookup_ids_depth / _page_depth,
keto_amd/csrc/depth.hpp): the tests of depth_gpu_suite.py over the lookup handle, the synthetic
workloads of test_lookup_gpu.py at k = 1, 2 and 3, the named calls, and tools/depth_probe.py at
a small scale."""
import json
import os
import subprocess
import sys

import pytest

from keto_amd import lookup
from keto_amd import relationtuple as rt
from tests import depth_cases as DC
from tests import test_lookup_gpu as TL
from tests.depth_gpu_suite import *  # noqa: F401,F403  (the shared tests and their fixtures)
from tests.depth_gpu_suite import check_workload

pytestmark = pytest.mark.gpu


@pytest.fixture
def side():
    return DC.LookupSide


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
    with lookup.Lookup(snap) as lk:
        subjects, depths = [uk, uk, uk, nobody], [1, 6, lookup.DEPTH_ALL, 2]
        lists, complete = lk.list_objects_depth_batch("n", "member", subjects, depths)
        assert (lists, complete) == host.list_objects_depth_batch("n", "member", subjects, depths)
        assert lists == [["k0"], [f"k{i}" for i in range(6)], [f"k{i}" for i in range(6)], []]
        assert complete == [False, True, True, True]
        assert lk.ListObjects("n", "member", uk, max_depth=2) == ["k0", "k1"]
        assert lk.ListObjects("n", "member", uk) == [f"k{i}" for i in range(6)]  # None: today's path
        assert lk.list_objects_batch("n", "member", [uk], max_depth=3) == [["k0", "k1", "k2"]]
        assert lk.list_objects_page("n", "member", uk, 2, "", max_depth=3) == \
            host.list_objects_page("n", "member", uk, 2, "", max_depth=3)
        items, tok, total, complete = lk.list_objects_page("n", "member", uk, 2, "", max_depth=3)
        assert items == ["k0", "k1"] and total == 3 and complete is False
        items, tok, total, complete = lk.list_objects_page("n", "member", uk, 2, tok, max_depth=3)
        assert items == ["k2"] and tok == "" and complete is False
        assert len(lk.list_objects_page("n", "member", uk, 2, "")) == 3
        assert lk.list_objects_depth_batch("nowhere", "member", [uk], 2) == ([[]], [True])
        st = lk.depth_stats()
        assert st["requests"] == 4 + 1 + 1 + 3 and lk.stats()["requests"] == 2


def test_probe_at_a_small_scale(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "probe.json"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "depth_probe.py"), "--scale", "500", "--requests",
                        "96", "--reps", "2", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(out.read_text())
    for handle in ("subjects", "lookup"):
        res = doc[handle]
        assert res["answers_equal_host_twins"] == {"first_round": True, "last_round": True, "sample_per_k": 64}
        assert set(res["depth"]) == {"1", "2", "3", "all"}
        assert res["depth"]["all"]["cut_requests"] == 0
        assert res["depth"]["all"]["ids_produced"] == res["ids_per_plain_call"]
        for k in ("1", "2", "3", "all"):
            d = res["depth"][k]
            assert d["tier1_requests"] + d["tier2_requests"] <= res["requests"] and d["list"]["reps"] == 2
