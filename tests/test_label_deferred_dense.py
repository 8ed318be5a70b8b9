"""Plan label's deferred dense passes: a pipelined call's dense pass stays pending on its
stream and rides in the next pipelined call's launch (label_carry_kernel), or is launched on
its own at a flush point (device_engine.hip: PendingDense).  On the comb graph
(randgraph.make_comb_graph: every head pair sends more than half of the 2,616 requests to
the dense pass) every result that can be observed equals the CPU oracle bit for bit: batches
alternating on the two streams, one batch queued back to back (its two result arrays),
downloads with the pass still pending, every flush point, request counts around the unit and
the word with batches of no and of only dense requests (chosen with tests/label_census.py),
writes between queued calls on a writable snapshot, and KETOGPU_LABEL_DEFER=0 (two launches
per call) word for word."""
import functools
from collections import Counter

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import label_census as C
from tests import randgraph

pytestmark = pytest.mark.gpu

HEADS = [(8, 8), (32, 32), (64, 64), (8, 64)]
COUNTS = [1, 15, 16, 17, 64, 1024, 2616]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def classes(heads):
    """label_census's class of every comb request at `heads` (computed once per head pair)"""
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    return tuple(C.classify(li, int(r), int(t), c["ni"]) for r, t in zip(c["roots"], c["targets"]))


def opened(heads):
    """the requests the dense pass answers"""
    return np.array([isinstance(k, tuple) for k in classes(heads)])


def label_env(monkeypatch, heads, **more):
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", f"{heads[0]},{heads[1]}")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def comb(heads):
    c = C.comb_case()
    n_open = int(opened(heads).sum())
    assert 1361 <= n_open <= 2200  # more than half of every batch goes through the dense pass
    return c, c["want"], c["roots"], c["targets"]


def engine(c):
    """an engine whose first (synchronized) call is behind it: pipelined calls are queued"""
    eng = check.Engine(c["snap"])
    warm = eng.upload(c["roots"][:64], c["targets"][:64])
    warm.run()
    assert eng.last_stats()["plan"] == 7
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


@pytest.mark.parametrize("heads", HEADS)
def test_two_batches_alternating(heads, monkeypatch):
    """A, B, A, B, A queued on one engine, then wait: both downloads equal the oracle, and
    equal KETOGPU_LABEL_DEFER=0's words (two launches per call; with the completion event
    recorded after every call: the calls as they were before deferral)"""
    got = []
    for defer, event in (("1", "demand"), ("0", "demand"), ("0", "record")):
        label_env(monkeypatch, heads, KETOGPU_LABEL_DEFER=defer, KETOGPU_LABEL_DONE_EVENT=event)
        c, want, roots, targets = comb(heads)
        eng = engine(c)
        a, b = eng.upload(roots, targets), eng.upload(roots[::-1].copy(), targets[::-1].copy())
        queue(a, b, a, b, a)
        eng.wait()
        got.append((words_ok(a, want), words_ok(b, want[::-1])))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("heads", HEADS)
def test_one_batch_back_to_back_and_three_batches(heads, monkeypatch):
    """one batch queued five times back to back (its calls alternate between its two result
    arrays and between the streams), then three batches over the two streams, twice around"""
    label_env(monkeypatch, heads)
    c, want, roots, targets = comb(heads)
    eng = engine(c)
    a = eng.upload(roots, targets)
    queue(a, a, a, a, a)
    words_ok(a, want)
    half = len(roots) // 2
    b = eng.upload(roots[::-1].copy(), targets[::-1].copy())
    d = eng.upload(roots[:half], targets[:half])
    queue(a, b, d, a, b, d)
    eng.wait()
    words_ok(a, want)
    words_ok(b, want[::-1])
    words_ok(d, want[:half])
    queue(a, b, d, a, b, d)  # and read with no wait, the last batch first
    words_ok(d, want[:half])
    words_ok(b, want[::-1])
    words_ok(a, want)


@pytest.mark.parametrize("event", ["demand", "record", "nofence"])
@pytest.mark.parametrize("heads", HEADS)
def test_download_with_the_pass_pending(heads, event, monkeypatch):
    """a download with no wait before it launches the batch's pending pass; a batch whose
    pass later launches carried is read after them.  The copy that follows the completion
    event sees every result word however the event is recorded (KETOGPU_LABEL_DONE_EVENT:
    when something waits for it, after every call, after every call without the system fence)"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_DONE_EVENT=event)
    c, want, roots, targets = comb(heads)
    eng = engine(c)
    a = eng.upload(roots, targets)
    queue(a)
    words_ok(a, want)  # pending on its stream
    b = eng.upload(roots[::-1].copy(), targets[::-1].copy())
    d = eng.upload(roots[::2].copy(), targets[::2].copy())
    queue(a, b, d)  # d's launch carries a's pass (same stream), b's and d's stay pending
    words_ok(a, want)
    words_ok(b, want[::-1])
    words_ok(d, want[::2])
    queue(a, b, d, a)
    words_ok(b, want[::-1])
    words_ok(a, want)
    words_ok(d, want[::2])


@pytest.mark.parametrize("point", ["check_ids", "run", "upload", "regrow", "close", "engine"])
@pytest.mark.parametrize("heads", HEADS)
def test_flush_points(heads, point, monkeypatch):
    """work that is not a pipelined call, issued right after a queued call: the pending pass
    is launched first and the earlier batch's download equals the oracle"""
    label_env(monkeypatch, heads)
    c, want, roots, targets = comb(heads)
    eng = engine(c)
    a = eng.upload(roots, targets)
    b = eng.upload(roots[::-1].copy(), targets[::-1].copy())
    big = eng.upload(np.tile(roots, 3), np.tile(targets, 3)) if point == "regrow" else None
    queue(a, b)
    if point == "check_ids":
        np.testing.assert_array_equal(eng.check_ids(roots[:500], targets[:500]), want[:500])
    elif point == "run":
        b.run()
        words_ok(b, want[::-1])
    elif point == "upload":
        big = eng.upload(np.tile(roots, 3), np.tile(targets, 3))
    elif point == "regrow":  # the spill lists and the dense pass's records are reallocated for this call
        big.run(pipelined=True)
        words_ok(big, np.tile(want, 3))
    elif point == "close":  # a batch freed with its pass pending, then calls on another
        b.close()
        queue(a, a)
    elif point == "engine":  # the engine freed with passes pending: the process goes on
        eng.close()
        return
    words_ok(a, want)
    if point not in ("close", "run"):
        words_ok(b, want[::-1])
    queue(a, a)
    eng.wait()
    words_ok(a, want)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("heads", HEADS)
def test_request_counts(heads, n, monkeypatch):
    """n requests around the unit (16) and the result word (64): the first pipelined call of
    a fresh engine (nothing to carry), then a batch without dense requests followed by one
    of dense requests only (the carrying grid, sized from the last synchronized call, is too
    small: the persistent loop covers the list) and the reverse order"""
    label_env(monkeypatch, heads)
    c, want, roots, targets = comb(heads)
    cl, op = classes(heads), opened(heads)

    def pick(idx):
        idx = np.resize(idx, n)
        return idx, Counter(cl[i] for i in idx)

    mixed = np.random.default_rng(7).permutation(len(roots))[:n]
    none, census = pick(np.flatnonzero(~op))
    assert C.dense_count(census) == 0
    dense, census = pick(np.flatnonzero(op))
    assert C.dense_count(census) == n
    eng = check.Engine(c["snap"])
    first = eng.upload(roots[mixed], targets[mixed])
    first.run(pipelined=True)  # (the engine's first call: it may synchronize)
    words_ok(first, want[mixed])
    q0, q1 = eng.upload(roots[none], targets[none]), eng.upload(roots[dense], targets[dense])
    q0.run()  # full_requests of the last synchronized call: 0
    assert eng.last_stats()["full_requests"] == 0
    for order in ((q0, q1), (q1, q0)):
        for _ in range(2):  # (twice: each on both streams' turn)
            queue(*order, *order)
            eng.wait()
            words_ok(q0, want[none])
            words_ok(q1, want[dense])
        queue(*order)
        words_ok(order[0], want[none] if order[0] is q0 else want[dense])
        words_ok(order[1], want[none] if order[1] is q0 else want[dense])


@pytest.mark.parametrize("heads", HEADS)
def test_writes_between_queued_calls(heads, monkeypatch):
    """a writable snapshot (VersionedEngine): a call queued before a write answers from the
    rows before it — its pending pass is launched before label_update rewrites the heads and
    overflow lists — and a call queued after it from the rows after it.  The write adds a
    group to a document whose P list overflows its head and a nesting edge between two
    components"""
    from keto_amd.freshness import VersionedEngine
    from tests.test_writes import _tuple
    label_env(monkeypatch, heads)
    namespaces, rows, reqs = randgraph.make_comb_graph(95)
    id2name = {i: nm for nm, i in namespaces}
    held = Counter(r[1] for r in rows if r[1].startswith("D") and r[5] and r[5].startswith("g"))
    doc, count = held.most_common(1)[0]
    assert count > 60  # past every head's inline entries
    mine = {r[5] for r in rows if r[1] == doc and r[5] and r[5].startswith("g")}
    free = sorted(g for g in {r[1] for r in rows if r[1].startswith("g")} if g not in mine)
    inside = sorted(mine)[0]
    ins = [(1, doc, "view", None, 1, free[0], "member"),                   # P(doc) grows
           (1, inside, "member", None, 1, "h" + free[-1][1:], "member")]  # a nesting edge g -> h elsewhere
    after = rows + ins
    want0 = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    want1 = np.asarray(randgraph.oracle_store(namespaces, after).check_batch(reqs), dtype=bool)
    assert (want0 != want1).any()
    ve = VersionedEngine(Snapshot.from_rows(namespaces, rows, sort=True, writable=True))
    snap, eng = ve._state[0], ve._state[1]
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    q0, q1 = eng.upload(roots, targets), eng.upload(roots, targets)
    q0.run()
    np.testing.assert_array_equal(q0.download(), want0)
    assert q0.run(pipelined=True) is True
    ve.transact(insert=[_tuple(r, id2name) for r in ins])
    assert ve.last_write["path"] == "in_place" and ve._state[1] is eng
    q1.run(pipelined=True)  # (marked roots may send it through the second stage: synchronized then)
    np.testing.assert_array_equal(q0.download(), want0)
    np.testing.assert_array_equal(q1.download(), want1)
    q0.run(pipelined=True)
    q1.run(pipelined=True)
    eng.wait()
    np.testing.assert_array_equal(q0.download(), want1)
    np.testing.assert_array_equal(q1.download(), want1)


@pytest.mark.parametrize("heads", [(8, 8), (64, 64)])
def test_second_stage_calls_stay_synchronous(heads, monkeypatch):
    """a quarter of the S heads unlabelled (KETOGPU_LABEL_REST_PERMILLE=250): requests may
    need the second stage, so run(pipelined=True) does not queue and is correct as before"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_REST_PERMILLE=250)
    c, want, roots, targets = comb(heads)
    eng = check.Engine(c["snap"])
    a, b = eng.upload(roots, targets), eng.upload(roots[::-1].copy(), targets[::-1].copy())
    for q, w in ((a, want), (b, want[::-1]), (a, want)):
        assert q.run(pipelined=True) is False
        np.testing.assert_array_equal(q.download(), w)
    eng.wait()
    np.testing.assert_array_equal(b.download(), want[::-1])
