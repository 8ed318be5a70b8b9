"""Plan label's tail phase on the device (label_carry_kernel<.., true>, KETOGPU_LABEL_TAIL):
queued calls answer short P overflows inside their first stage.  On the tail graph
(tests/label_tail.py: every head pair reaches every case of the phase and its neighbours, as
tests/test_label_tail_census.py asserts on the CPU) every observable result equals the CPU
oracle word for word and equals KETOGPU_LABEL_TAIL=0's; the dense pass of a queued call finds
exactly the restatement's still-dense requests listed (Engine.piped_full_requests), while
synchronized calls keep reporting the whole open count; units of only, of one and of no tail
request; a write that shortens a tail on a writable snapshot."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import label_tail as T
from tests import randgraph

pytestmark = pytest.mark.gpu

HEADS = T.HEAD_PAIRS


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def label_env(monkeypatch, heads, **more):
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", f"{heads[0]},{heads[1]}")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def engine(c):
    """an engine whose first (synchronized) call is behind it: pipelined calls are queued"""
    eng = check.Engine(c["snap"])
    warm = eng.upload(c["roots"][:64], c["targets"][:64])
    warm.run()
    assert eng.last_stats()["plan"] == 7
    assert eng.piped_full_requests() == 0  # (no queued call's pass yet)
    return eng


def queue(*qs):
    for q in qs:
        assert q.run(pipelined=True) is True  # enqueued: no host wait


def words_ok(q, want):
    """the batch's raw words: the oracle's bits, none set past n, no flag"""
    ab, fb = q.download_words()
    np.testing.assert_array_equal(check.unpack_bits(ab, q.n), want)
    if q.n % 64:
        assert int(ab[-1]) >> (q.n % 64) == 0
    assert not fb.any()
    return ab


def is_tail(heads):
    k = T.kinds(heads)
    return (k == "tail-true") | (k == "tail-false")


@pytest.mark.parametrize("heads", HEADS)
def test_answers_and_the_path_taken(heads, monkeypatch):
    """a batch queued alone, two batches alternating A, B, A, B, A and one batch back to
    back: the oracle's words, with and without the phase; after a batch queued alone the
    flushed pass found the still-dense requests (all open ones without the phase); every
    synchronized way in reports the old open count"""
    c = T.tail_case()
    want, roots, targets = c["want"], c["roots"], c["targets"]
    n_open, n_dense = T.open_count(heads)
    assert n_dense < n_open
    got = []
    for tail in ("1", "0"):
        label_env(monkeypatch, heads, KETOGPU_LABEL_TAIL=tail)
        eng = engine(c)
        a, b = eng.upload(roots, targets), eng.upload(roots[::-1].copy(), targets[::-1].copy())
        queue(a)
        eng.wait()
        assert eng.piped_full_requests() == (n_dense if tail == "1" else n_open)
        alone = words_ok(a, want)
        queue(a, b, a, b, a)
        eng.wait()
        got.append((alone, words_ok(a, want), words_ok(b, want[::-1])))
        queue(a, a, a, a, a)
        np.testing.assert_array_equal(words_ok(a, want), alone)
        # synchronized calls: the first stage as it was, the tail class listed with the rest
        a.run()
        assert eng.last_stats()["full_requests"] == n_open
        np.testing.assert_array_equal(words_ok(a, want), alone)
        np.testing.assert_array_equal(eng.check_ids(roots, targets), want)
        assert eng.last_stats()["full_requests"] == n_open
        pr, pt = check.pinned(roots), check.pinned(targets)
        out = check.PinnedBuffer((len(roots) + 63) // 64, np.uint64)
        eng.check_ids_raw(pr.array.ctypes.data, pt.array.ctypes.data, len(roots), out.array.ctypes.data)
        np.testing.assert_array_equal(out.array, alone)
        assert eng.last_stats()["full_requests"] == n_open
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("heads", HEADS)
def test_request_counts(heads, monkeypatch):
    """n requests around the unit (16) and the result word (64), every other one of the tail
    class: queued twice (both streams) and read with the pass pending"""
    label_env(monkeypatch, heads)
    c = T.tail_case()
    want, roots, targets = c["want"], c["roots"], c["targets"]
    tl = is_tail(heads)
    ti, oi = np.flatnonzero(tl), np.flatnonzero(~tl)
    eng = engine(c)
    for n in (1, 15, 16, 17, 64):
        idx = np.empty(n, dtype=np.int64)
        idx[0::2] = ti[: (n + 1) // 2]
        idx[1::2] = oi[n: n + n // 2]
        q = eng.upload(roots[idx], targets[idx])
        queue(q, q)
        words_ok(q, want[idx])
        queue(q)
        eng.wait()
        assert eng.piped_full_requests() == T.open_count(heads, idx)[1]
        words_ok(q, want[idx])


@pytest.mark.parametrize("heads", HEADS)
def test_units_of_only_one_and_no_tail_request(heads, monkeypatch):
    """a unit of 16 tail requests, units with exactly one (at quad 0, at quad 15) among
    requests of every other kind, and a unit without one (its wave skips the phase)"""
    label_env(monkeypatch, heads)
    c = T.tail_case()
    want, roots, targets = c["want"], c["roots"], c["targets"]
    tl = is_tail(heads)
    ti, oi = np.flatnonzero(tl), np.random.default_rng(5).permutation(np.flatnonzero(~tl))
    true_i = np.flatnonzero(T.kinds(heads) == "tail-true")
    idx = np.concatenate([ti[:16], true_i[:1], oi[:15], oi[15:30], true_i[1:2], oi[30:46]])
    assert tl[idx].tolist() == [True] * 17 + [False] * 30 + [True] + [False] * 16 and want[idx[16]] and want[idx[47]]
    eng = engine(c)
    q = eng.upload(roots[idx], targets[idx])
    queue(q)
    eng.wait()
    assert eng.piped_full_requests() == T.open_count(heads, idx)[1]
    words_ok(q, want[idx])
    queue(q, q, q)
    words_ok(q, want[idx])


@pytest.mark.parametrize("heads", HEADS)
def test_tail_only_batches_beside_batches_without(heads, monkeypatch):
    """a batch of tail requests only (its pass finds nothing listed) followed by batches with
    none — decided by the heads, or 2,000 dense requests: the carried grid, sized from the
    empty pass, is too small and the persistent loop covers the list — and the reverse order
    (the grid too large)"""
    label_env(monkeypatch, heads)
    c = T.tail_case()
    want, roots, targets = c["want"], c["roots"], c["targets"]
    k = T.kinds(heads)
    ti = np.flatnonzero(is_tail(heads))
    hi = np.flatnonzero(k == "heads")
    di = np.resize(np.flatnonzero(k == "dense"), 2000)
    eng = engine(c)
    qt, qh, qd = (eng.upload(roots[i], targets[i]) for i in (ti, hi, di))
    queue(qt)
    eng.wait()
    assert eng.piped_full_requests() == 0
    of = {qt: ti, qh: hi, qd: di}
    for order in ((qt, qh), (qt, qd), (qd, qt), (qh, qt)):
        queue(*order, *order)
        eng.wait()
        for q in order:
            words_ok(q, want[of[q]])
        queue(*order)
        words_ok(order[1], want[of[order[1]]])
        words_ok(order[0], want[of[order[0]]])
    queue(qd)
    eng.wait()
    assert eng.piped_full_requests() == 2000


@pytest.mark.parametrize("heads", HEADS)
def test_a_write_shortens_a_tail(heads, monkeypatch):
    """a writable snapshot (VersionedEngine): a write removes the membership that gives a P
    list its last tail entry, the only landmark some user shares with the document.  The
    list is rewritten in place, one entry shorter: a call queued before the write answers
    true, one queued after it false — the words behind a list's end are never taken for
    entries."""
    from keto_amd.freshness import VersionedEngine
    from tests.test_writes import _tuple
    label_env(monkeypatch, heads)
    cp = heads[1] - 4
    namespaces, rows, reqs, docs, pairs = T.make_tail_graph()
    id2name = {i: nm for nm, i in namespaces}
    doc, (a, n) = next((d, v) for d, v in sorted(docs.items()) if v[1] == cp + 3)
    at = next(i for i, (d, _, role) in enumerate(pairs) if d == doc and role == "last")
    dele = [(1, doc, "view", None, 1, f"g{a + 2 * (n - 1):03d}", "member")]
    assert dele[0] in rows
    after = [r for r in rows if r != dele[0]]
    want0 = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    want1 = np.asarray(randgraph.oracle_store(namespaces, after).check_batch(reqs), dtype=bool)
    assert want0[at] and not want1[at]
    ve = VersionedEngine(Snapshot.from_rows(namespaces, rows, sort=True, writable=True))
    snap, eng = ve._state[0], ve._state[1]
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    li, ni = snap.label_index(*heads), int(snap.stats()["num_interior"])
    assert T.tail_stage(li, int(roots[at]), int(targets[at]), ni)["kind"] == "tail-true"
    q0, q1 = eng.upload(roots, targets), eng.upload(roots, targets)
    q0.run()
    np.testing.assert_array_equal(q0.download(), want0)
    assert q0.run(pipelined=True) is True
    ve.transact(delete=[_tuple(r, id2name) for r in dele])
    assert ve.last_write["path"] == "in_place" and ve._state[1] is eng
    assert q1.run(pipelined=True) is True  # (a document's row: no root is marked, the call is queued)
    np.testing.assert_array_equal(q0.download(), want0)
    np.testing.assert_array_equal(q1.download(), want1)
    queue(q0, q1)
    eng.wait()
    np.testing.assert_array_equal(q0.download(), want1)
    np.testing.assert_array_equal(q1.download(), want1)
