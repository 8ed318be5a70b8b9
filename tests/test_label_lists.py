"""Plan label on the GPU over lists past its heads, its stages and its prefetch: the comb
graph (randgraph.make_comb_graph; tests/test_label_census.py asserts on the CPU which
branches it reaches at each head pair) through label_kernel, label_host_kernel,
label_full_kernel and the device head build, against the CPU oracle bit for bit, and the
first stage's routing (last_stats()["full_requests"]) against its restatement
(tests/test_core_index.py first_stage)."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from tests import label_census as C
from tests.test_core_index import NONE_, first_stage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def routing(heads):
    """the host index for `heads` and, per request, whether the restated first stage leaves
    it open (None: the dense pass) -> (li, open flags); computed once per head pair"""
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    opened = np.array([r != NONE_ and t != NONE_ and first_stage(li, int(r), int(t), c["ni"]) is None
                       for r, t in zip(c["roots"], c["targets"])])
    opened.setflags(write=False)
    return li, opened


def label_env(monkeypatch, heads, **more):
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", f"{heads[0]},{heads[1]}")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize("heads", C.HEAD_PAIRS)
def test_comb_matches_oracle_and_routing(heads, monkeypatch):
    """every way into plan label (ketogpu_check, host ids, an HBM-resident batch, pinned
    host requests read in place, pipelined calls) equals the oracle on the comb graph, and
    every synchronized call sends exactly the requests to the dense pass that the restated
    first stage leaves open (the first call and the calls with events collect statistics, the
    lean resident calls in between have the dense pass write its list total itself)"""
    label_env(monkeypatch, heads)
    c = C.comb_case()
    li, opened = routing(heads)
    n_open = int(opened.sum())
    assert n_open > 0
    want, roots, targets = c["want"], c["roots"], c["targets"]
    eng = check.Engine(c["snap"])

    def stats_ok():
        st = eng.last_stats()
        assert st["plan"] == 7 and st["label_on"] == 1
        assert (st["label_s_head"], st["label_p_head"]) == (li["s_head_words"], li["p_head_words"])
        assert (st["full_requests"], st["rest_requests"]) == (n_open, 0)

    tuples = [rt.InternalRelationTuple(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in c["reqs"]]
    assert eng.check_many(tuples) == want.tolist()
    stats_ok()
    if heads != (0, 0):
        assert (li["s_head_words"], li["p_head_words"]) == heads
    np.testing.assert_array_equal(eng.check_ids(roots, targets), want)
    stats_ok()
    q = eng.upload(roots, targets)  # HBM-resident: the first call, then lean ones
    for _ in range(3):
        q.run()
        np.testing.assert_array_equal(q.download(), want)
        stats_ok()
    pr, pt = check.pinned(roots), check.pinned(targets)  # pinned host requests read in place
    out = check.PinnedBuffer((len(roots) + 63) // 64, np.uint64)
    eng.check_ids_raw(pr.array.ctypes.data, pt.array.ctypes.data, len(roots), out.array.ctypes.data)
    np.testing.assert_array_equal(check.unpack_bits(out.array.copy(), len(roots)), want)
    stats_ok()
    q2 = eng.upload(roots[::-1].copy(), targets[::-1].copy())
    q2.run()
    assert [q.run(pipelined=True), q2.run(pipelined=True), q.run(pipelined=True)] == [True] * 3
    eng.wait()
    np.testing.assert_array_equal(q.download(), want)
    np.testing.assert_array_equal(q2.download(), want[::-1])
    assert eng.last_stats()["plan"] == 7
    eng.set_events(True)  # an event between the kernels: statistics in every call
    q.run()
    np.testing.assert_array_equal(q.download(), want)
    stats_ok()


@pytest.mark.parametrize("heads", [(8, 8), (64, 64)])
def test_comb_routing_with_unlabelled_heads(heads, monkeypatch):
    """a quarter of the S heads marked unlabelled (KETOGPU_LABEL_REST_PERMILLE): their
    requests go to the second stage and the answers still equal the oracle; the dense pass
    gets the restatement's open requests among the labelled ones only.  The host index hook
    builds without the knob, so the marked heads are read from the engine's own S heads (the
    count word alone); without the knob the equality is test_comb_matches_oracle_and_routing's"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_REST_PERMILLE=250)
    c = C.comb_case()
    li, opened = routing(heads)
    want, roots, targets = c["want"], c["roots"], c["targets"]
    eng = check.Engine(c["snap"])
    S, hs = eng.label_heads(0)
    assert hs == heads[0]
    some = (roots != NONE_) & (targets != NONE_)
    marked = np.zeros(len(roots), dtype=bool)
    marked[some] = S[targets[some].astype(np.int64) * hs] == NONE_
    assert 0 < marked.sum() < some.sum()
    n_open = int((opened & ~marked).sum())
    assert 0 < n_open < opened.sum()
    np.testing.assert_array_equal(eng.check_ids(roots, targets), want)
    st = eng.last_stats()
    assert st["plan"] == 7
    assert (st["full_requests"], st["rest_requests"]) == (n_open, int(marked.sum()))
    q = eng.upload(roots, targets)
    for _ in range(2):
        q.run()
        np.testing.assert_array_equal(q.download(), want)
        st = eng.last_stats()
        assert (st["full_requests"], st["rest_requests"]) == (n_open, int(marked.sum()))


@pytest.mark.parametrize("big_cap", [None, 1])
@pytest.mark.parametrize("heads", [(0, 0), (8, 8), (64, 64)])
def test_comb_device_build_equals_host(heads, big_cap, monkeypatch):
    """the head arrays built on the device equal the host build word for word where both
    sides have lists of more than 64 entries: those are the host's nodes of the device build
    (label_big_io_kernel, label_patch_kernel); big_cap 1: room for one such node at first, so
    the count pass runs again"""
    label_env(monkeypatch, heads)
    if big_cap:
        monkeypatch.setenv("KETOGPU_TEST_LABEL_BIG_CAP", str(big_cap))
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    for A, h, n in ((li["S"], li["s_head_words"], li["s_nodes"]), (li["P"], li["p_head_words"], li["p_nodes"])):
        assert (A[: n * h].reshape(-1, h)[:, 0] > 64).sum() >= 2  # (no head is marked: counts only)
    eng = check.Engine(c["snap"])
    S, hs_dev = eng.label_heads(0)
    P, hp_dev = eng.label_heads(1)
    assert (hs_dev, hp_dev) == (li["s_head_words"], li["p_head_words"])
    np.testing.assert_array_equal(S, li["S"])
    np.testing.assert_array_equal(P, li["P"])


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 48, 49, 63, 64, 65, 1025])
def test_comb_request_count_edges(n, fuse, monkeypatch):
    """HBM-resident calls back to back over n requests around the unit (16), the result
    word (64) and past 1024, alternating with the whole batch on the same engine: every
    call's answers equal the oracle, no bit past n is set, the flag words are zero and the
    dense pass gets exactly the slice's open requests (lean calls skip the clear,
    KETOGPU_LABEL_FUSE=0 clears and collects statistics in every call)"""
    label_env(monkeypatch, (0, 0), KETOGPU_LABEL_FUSE=fuse)
    c = C.comb_case()
    _, opened = routing((0, 0))
    pick = np.random.default_rng(11).permutation(len(c["roots"]))[:n]  # (a mix of every class)
    want, roots, targets = c["want"][pick], c["roots"][pick], c["targets"][pick]
    eng = check.Engine(c["snap"])

    def run_ok(q, w, n_open):
        q.run()
        ab, fb = q.download_words()
        np.testing.assert_array_equal(check.unpack_bits(ab, q.n), w)
        if q.n % 64:
            assert int(ab[-1]) >> (q.n % 64) == 0  # no bit past n
        assert not fb.any()
        st = eng.last_stats()
        assert (st["plan"], st["full_requests"], st["rest_requests"]) == (7, n_open, 0)

    short, long_ = eng.upload(roots, targets), eng.upload(c["roots"], c["targets"])
    for _ in range(4):
        run_ok(short, want, int(opened[pick].sum()))
    for _ in range(2):  # a long batch and a short one in turn
        run_ok(long_, c["want"], int(opened.sum()))
        run_ok(short, want, int(opened[pick].sum()))
    rev = eng.upload(roots[::-1].copy(), targets[::-1].copy())
    for _ in range(4):
        run_ok(rev, want[::-1], int(opened[pick].sum()))
