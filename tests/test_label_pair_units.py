"""Plan label's first stage with two units per wave (device_engine.hip label_pair,
KETOGPU_LABEL_PAIR): a wave reads 32 requests as two whole lines and settles units 2p and
2p + 1 one after the other.  On the comb graph (tests/label_census.py) every observable
result equals the CPU oracle bit for bit at request counts around the pair (32) and the
result word (64), the raw words are the same with the switch at 2 (every launch paired), 1
(the default: queued calls at 32-word heads) and 0 and with the tail phase on and off, the
engine's count of paired launches says that the launches meant were paired, NONE requests in both halves of a pair leave their neighbours alone, the
synchronized call's statistics do not depend on the switch, and the random-line probe runs on
one and on two streams."""
import ctypes as ct

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from tests import label_census as C

pytestmark = pytest.mark.gpu

HEADS = [(8, 8), (32, 32), (64, 64), (8, 64), (64, 8)]
COUNTS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 2616]
NONE_ = np.uint32(L.NODE_NONE)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def label_env(monkeypatch, heads, **more):
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", f"{heads[0]},{heads[1]}")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


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


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("heads", HEADS)
def test_counts_around_the_pair_and_the_word(heads, n, monkeypatch):
    """one synchronized call (label_kernel), then the batch queued twice with a download
    between (label_carry_kernel, the second call carrying the first's dense pass), every
    launch with two units per wave (KETOGPU_LABEL_PAIR=2)"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_PAIR=2)
    c = C.comb_case()
    idx = np.random.default_rng(11).permutation(len(c["roots"]))[:n]
    roots, targets, want = c["roots"][idx].copy(), c["targets"][idx].copy(), c["want"][idx].copy()
    eng = check.Engine(c["snap"])
    q = eng.upload(roots, targets)
    q.run()
    assert eng.last_stats()["plan"] == 7
    words_ok(q, want)
    assert eng.label_pair_launches() == 1
    queue(q)
    words_ok(q, want)
    queue(q)
    words_ok(q, want)
    assert eng.label_pair_launches() == 3


@pytest.mark.parametrize("heads", HEADS)
def test_switch_and_tail_word_for_word(heads, monkeypatch):
    """A, B, A, B, A queued on one engine with KETOGPU_LABEL_PAIR at 2, 1 and 0 and
    KETOGPU_LABEL_TAIL on and off: the raw result words of all runs are identical and equal
    the oracle.  Paired launches: at 2 the warm-up call and the five queued ones, at 1 the
    queued ones at 32-word heads only, at 0 none"""
    got = []
    for pair, tail in ((2, 1), (1, 1), (0, 1), (2, 0), (1, 0), (0, 0)):
        label_env(monkeypatch, heads, KETOGPU_LABEL_PAIR=pair, KETOGPU_LABEL_TAIL=tail)
        c = C.comb_case()
        roots, targets, want = c["roots"], c["targets"], c["want"]
        eng = check.Engine(c["snap"])
        warm = eng.upload(roots[:64], targets[:64])
        warm.run()
        a, b = eng.upload(roots, targets), eng.upload(roots[::-1].copy(), targets[::-1].copy())
        queue(a, b, a, b, a)
        eng.wait()
        assert eng.label_pair_launches() == {2: 6, 1: 5 if heads == (32, 32) else 0, 0: 0}[pair]
        got.append((words_ok(a, want), words_ok(b, want[::-1])))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("n", [35, 40, 2616])
@pytest.mark.parametrize("heads", [(8, 8), (32, 32), (64, 64)])
def test_none_requests_in_both_halves(heads, n, monkeypatch):
    """requests 14-18 and 30-34 carry NONE (as root, as target, or both): they answer false
    and every other request answers as the oracle, synchronized and queued.  At n = 35 and 40
    the second pair's second unit lies wholly past n.  An id outside the snapshot is refused
    at upload with the first such request's index, as before"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_PAIR=2)
    c = C.comb_case()
    roots, targets, want = c["roots"][:n].copy(), c["targets"][:n].copy(), c["want"][:n].copy()
    assert want[:48].any()
    holes = [k for k in list(range(14, 19)) + list(range(30, 35)) if k < n]
    for k in holes:
        if k % 3 != 1:
            roots[k] = NONE_
        if k % 3 != 0:
            targets[k] = NONE_
    want[holes] = False
    eng = check.Engine(c["snap"])
    q = eng.upload(roots, targets)
    q.run()
    words_ok(q, want)
    q.run(pipelined=True)
    words_ok(q, want)
    q.run(pipelined=True)
    q.run(pipelined=True)
    words_ok(q, want)
    bad_r, bad_t = c["roots"][:n].copy(), c["targets"][:n].copy()
    for k in holes:
        (bad_r if k % 2 else bad_t)[k] = np.uint32(0x7FFFFFF0)
    with pytest.raises(L.KetoError) as err:
        eng.upload(bad_r, bad_t)
    assert err.value.code == L.EINVAL and "request 14 " in str(err.value)
    q.run(pipelined=True)  # the engine goes on
    words_ok(q, want)


def test_statistics_do_not_depend_on_the_switch(monkeypatch):
    """a synchronized call with events: rows, entries, full_requests and rest_requests over
    the 2,616 comb requests at 32,32 are the same with two units per wave (KETOGPU_LABEL_PAIR=2:
    label_kernel paired) and with one"""
    seen = []
    for pair in (2, 0):
        label_env(monkeypatch, (32, 32), KETOGPU_LABEL_PAIR=pair)
        c = C.comb_case()
        eng = check.Engine(c["snap"])
        q = eng.upload(c["roots"], c["targets"])
        q.run()
        eng.set_events(True)
        q.run()
        np.testing.assert_array_equal(q.download(), c["want"])
        st = eng.last_stats()
        assert eng.label_pair_launches() == pair
        seen.append({k: st[k] for k in ("unit_rows", "unit_rev", "label_entries", "full_requests", "rest_requests")})
    assert seen[0]["unit_rows"] > 0 and seen[0]["full_requests"] > 0
    assert seen[0] == seen[1]


def test_probe_on_streams():
    """ketogpu_probe_random_lines_streams: a positive time per launch on one and on two
    streams (64 MiB table, 4,096 requests); no stream is an invalid argument"""
    lib = L.lib()
    for streams in (1, 2):
        ms = ct.c_double(0)
        assert lib.ketogpu_probe_random_lines_streams(0, 64 << 20, 4096, 4, streams, ct.byref(ms)) == L.OK
        assert ms.value > 0
    ms = ct.c_double(0)
    assert lib.ketogpu_probe_random_lines_streams(0, 64 << 20, 4096, 4, 0, ct.byref(ms)) == L.EINVAL
