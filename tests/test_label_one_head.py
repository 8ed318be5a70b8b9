"""Plan label's queued first stage reading S first and P only where S leaves the answer
open (device_engine.hip label_head_s / label_s_decides, KETOGPU_LABEL_SFIRST).  Two classes
of requests are decided by the S head alone: a one-edge hit (the root among S(t)'s inline raw
entries) and settled-false (S's mask zero, no inline landmark, the one-edge test settled).

On the CPU: for every request of the class, the first-stage replay (first_stage) decides the
same with P(r) replaced by an empty head, that decision is the oracle's answer, and a
lane-by-lane restatement of the kernel's register computation calls exactly the class decided.
On the GPU (KETOGPU_LABEL_SFIRST=2): every observable result equals the oracle bit for bit at
request counts around the pair and the word, the raw words do not depend on the switches,
the count of skipped P reads equals the count computed from the index, units built by index
(all skipped, none, a pair of both) with NONE neighbours, writes on a writable snapshot, and
the synchronized call's statistics are untouched."""
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
from tests.test_core_index import NONE_, first_stage

HEADS = [(8, 8), (32, 32), (64, 64), (8, 64), (64, 8)]
COUNTS = [1, 15, 16, 17, 31, 32, 33, 52, 53, 63, 64, 65, 2616]
# the comb graph's classes per S head (one-edge hits, settled false by S).  At 8-word S
# heads the settled-false requests are lists of 9 and 11 raw entries and no landmark that
# overflow the head: es == 0 and r <= the last inline entry (or r interior) settle them too
COMB_CLASSES = {8: (12, 38), 32: (45, 88), 64: (65, 88)}


def flagged(heads, pair):
    """a queued launch reads S first at KETOGPU_LABEL_SFIRST=2: all but 8/64 heads paired, the
    one instantiation the flag takes past 64 VGPRs (launched as it was)"""
    return not (pair and heads == (8, 64))


def s_class(li, r, t, ni):
    """'edge' / 'false' when S(t)'s head alone decides request (r, t), else None: the rule,
    over the whole head"""
    hs, S = li["s_head_words"], li["S"]
    if r == NONE_ or t == NONE_:
        return None
    ns = int(S[t * hs])
    assert ns != NONE_ and int(li["P"][r * li["p_head_words"]]) != NONE_  # (a queued engine: every head labelled)
    se = S[t * hs + 4: t * hs + hs].astype(np.int64)
    if r >= ni and (se == r).any():
        return "edge"
    mask_zero = int(S[t * hs + 2]) == 0 and int(S[t * hs + 3]) == 0
    raw_done = r < ni or ns <= hs - 4 or r <= se[-1]
    if mask_zero and not (se < ni).any() and raw_done:
        return "false"
    return None


def s_decides_lanes(li, r, t, ni):
    """the kernel's computation, lane by lane (label_s_landmarks, label_s_edge,
    label_s_decides): lane `sub` of the request's four holds words [W sub, W sub + W) of the
    head; header words (0-3) are no entries"""
    hs, S = li["s_head_words"], li["S"]
    if r == NONE_ or t == NONE_:
        return False
    w = hs // 4
    head = [int(x) for x in S[t * hs: t * hs + hs]]
    es, any_edge = 0, False
    for sub in range(4):
        words = head[w * sub: w * sub + w]
        s_body = sub * w >= 4
        es += sum(1 for k, x in enumerate(words) if (k >= 4 or s_body) and x < ni)
        in_head = any(x == r for x in words[:4])
        in_body = any(x == r for x in words[4:])
        any_edge |= r >= ni and (in_body or (in_head and s_body))
    ns, sm, s_end = head[0], head[2] | head[3], head[hs - 1]
    raw_done = r < ni or ns <= hs - 4 or r <= s_end
    return any_edge or (sm == 0 and es == 0 and raw_done)


def with_empty_p(li, r):
    """the index with P(r) an empty head: count, overflow start and mask zero, pads"""
    hp = li["p_head_words"]
    P = li["P"].copy()
    P[r * hp: r * hp + 4] = 0
    P[r * hp + 4: r * hp + hp] = NONE_
    return dict(li, P=P)


@functools.lru_cache(maxsize=None)
def comb_classes(heads):
    """s_class of every comb request at `heads`"""
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    return tuple(s_class(li, int(r), int(t), c["ni"]) for r, t in zip(c["roots"], c["targets"]))


def check_class(snap, roots, targets, want, heads):
    li = snap.label_index(*heads)
    assert (li["s_head_words"], li["p_head_words"]) == heads
    ni = int(snap.stats()["num_interior"])
    seen = Counter()
    for i in range(len(roots)):
        r, t = int(roots[i]), int(targets[i])
        if r == NONE_ or t == NONE_:
            assert not s_decides_lanes(li, r, t, ni)
            continue
        k = s_class(li, r, t, ni)
        assert s_decides_lanes(li, r, t, ni) == (k is not None), (i, k)  # no request outside the class is closed
        if k is None:
            continue
        seen[k] += 1
        d = first_stage(with_empty_p(li, r), r, t, ni)
        assert d is not None and d == first_stage(li, r, t, ni), (i, k)
        assert d == (k == "edge") and d == bool(want[i]), (i, k)
    return seen


@pytest.mark.parametrize("heads", HEADS)
def test_the_class_settles_without_p_comb(heads):
    c = C.comb_case()
    seen = check_class(c["snap"], c["roots"], c["targets"], c["want"], heads)
    assert (seen["edge"], seen["false"]) == COMB_CLASSES[heads[0]]
    k = comb_classes(heads)
    assert k.index("edge") == 52
    if heads[0] >= 32:
        assert k.index("false") == 0


@pytest.mark.parametrize("seed", [81, 83])
@pytest.mark.parametrize("heads", HEADS)
def test_the_class_settles_without_p_random(heads, seed):
    namespaces, rows = randgraph.make_graph(seed, n_rows=900, n_obj=40, n_users=50)
    snap = Snapshot.from_rows(namespaces, rows, page_size=4, sort=True)
    reqs = randgraph.make_requests(seed, namespaces, rows, n=600, wildcard=False)
    want = randgraph.oracle_store(namespaces, rows, 4).check_batch(reqs)
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    seen = check_class(snap, roots, targets, want, heads)
    assert seen["edge"] + seen["false"] > 0


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@pytest.fixture
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


def warm_engine(c):
    """an engine whose first (synchronized) call is behind it: pipelined calls are queued"""
    eng = check.Engine(c["snap"])
    warm = eng.upload(c["roots"][:64], c["targets"][:64])
    warm.run()
    assert eng.last_stats()["plan"] == 7
    return eng


@gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("heads", HEADS)
def test_counts_around_the_pair_and_the_word(heads, n, monkeypatch, need_gpu):
    """one synchronized call, then the first n comb requests (request 52 is the first
    one-edge hit) queued twice with a download between; only the queued launches read S
    first"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_SFIRST=2)
    c = C.comb_case()
    roots, targets, want = c["roots"][:n].copy(), c["targets"][:n].copy(), c["want"][:n].copy()
    eng = check.Engine(c["snap"])
    q = eng.upload(roots, targets)
    q.run()
    assert eng.last_stats()["plan"] == 7
    words_ok(q, want)
    assert eng.label_sfirst_launches() == 0
    queue(q)
    words_ok(q, want)
    queue(q)
    words_ok(q, want)
    assert eng.label_sfirst_launches() == 2


@gpu
@pytest.mark.parametrize("heads", HEADS)
def test_switches_word_for_word(heads, monkeypatch, need_gpu):
    """A, B, A, B, A queued with KETOGPU_LABEL_SFIRST in {2, 0}, KETOGPU_LABEL_TAIL in {1, 0}
    and KETOGPU_LABEL_PAIR in {2, 0}: the raw words of all runs are identical and equal the
    oracle.  S first is built with the tail phase only: without it no launch has the flag"""
    got = []
    for sf in (2, 0):
        for tail in (1, 0):
            for pair in (2, 0):
                label_env(monkeypatch, heads, KETOGPU_LABEL_SFIRST=sf, KETOGPU_LABEL_TAIL=tail, KETOGPU_LABEL_PAIR=pair)
                c = C.comb_case()
                roots, targets, want = c["roots"], c["targets"], c["want"]
                eng = warm_engine(c)
                a, b = eng.upload(roots, targets), eng.upload(roots[::-1].copy(), targets[::-1].copy())
                queue(a, b, a, b, a)
                eng.wait()
                assert eng.label_sfirst_launches() == (5 if sf == 2 and tail and flagged(heads, pair) else 0)
                got.append((words_ok(a, want), words_ok(b, want[::-1])))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            np.testing.assert_array_equal(x, y)


@gpu
@pytest.mark.parametrize("pair", [2, 0])
@pytest.mark.parametrize("heads", HEADS)
def test_skipped_request_count(heads, pair, monkeypatch, need_gpu):
    """KETOGPU_LABEL_SFIRST_COUNT=1: after one queued call over the whole comb batch the
    engine's count of skipped P reads is the size of the class computed from the index; zero
    with the switch at 0"""
    k = comb_classes(heads)
    expect = sum(x is not None for x in k)
    assert expect == sum(COMB_CLASSES[heads[0]])
    for sf in (2, 0):
        label_env(monkeypatch, heads, KETOGPU_LABEL_SFIRST=sf, KETOGPU_LABEL_SFIRST_COUNT=1, KETOGPU_LABEL_PAIR=pair)
        c = C.comb_case()
        eng = warm_engine(c)
        q = eng.upload(c["roots"], c["targets"])
        queue(q)
        assert eng.label_one_head_requests() == (expect if sf and flagged(heads, pair) else 0)
        words_ok(q, c["want"])


@gpu
@pytest.mark.parametrize("pair", [2, 0])
@pytest.mark.parametrize("heads", HEADS)
def test_units_built_by_index(heads, pair, monkeypatch, need_gpu):
    """a unit whose 16 requests all skip P, one where none does, a pair whose first unit skips
    everything and whose second nothing, and the reverse; then the same pairs with NONE roots
    or targets next to skipped requests; with two units per wave (label_pair) and with one
    (label_unit: the only S-first kernel at 8/64 heads).  The words equal the oracle and the
    skipped count is the number of class requests left in the batch"""
    label_env(monkeypatch, heads, KETOGPU_LABEL_SFIRST=2, KETOGPU_LABEL_SFIRST_COUNT=1, KETOGPU_LABEL_PAIR=pair)
    c = C.comb_case()
    k = comb_classes(heads)
    valid = (c["roots"] != NONE_) & (c["targets"] != NONE_)
    dec = np.resize(np.flatnonzero([x is not None for x in k]), 16)
    opn = np.resize(np.flatnonzero([x is None and v for x, v in zip(k, valid)]), 16)
    assert {k[i] for i in dec} >= {"edge"} and c["want"][opn].any()
    eng = warm_engine(c)
    total = 0
    for idx in (dec, opn, np.concatenate([dec, opn]), np.concatenate([opn, dec])):
        for holes in (False, True):
            roots, targets, want = c["roots"][idx].copy(), c["targets"][idx].copy(), c["want"][idx].copy()
            closed = np.array([k[i] is not None for i in idx])
            if holes:
                for j in range(1, len(idx), 5):
                    if j % 3 != 1:
                        roots[j] = NONE_
                    if j % 3 != 0:
                        targets[j] = NONE_
                    want[j] = closed[j] = False
            q = eng.upload(roots, targets)
            queue(q)
            words_ok(q, want)
            queue(q)
            words_ok(q, want)
            total += 2 * int(closed.sum()) if flagged(heads, pair) else 0
            assert eng.label_one_head_requests() == total


def _writable(monkeypatch, heads, **more):
    from keto_amd.freshness import VersionedEngine
    label_env(monkeypatch, heads, KETOGPU_LABEL_SFIRST=2, **more)
    namespaces, rows, reqs = randgraph.make_comb_graph(95)
    ve = VersionedEngine(Snapshot.from_rows(namespaces, rows, sort=True, writable=True))
    snap, eng = ve._state[0], ve._state[1]
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    return ve, eng, namespaces, rows, reqs, roots, targets


@gpu
@pytest.mark.parametrize("heads", [(32, 32), (64, 64)])
def test_direct_grant_written_in_place(heads, monkeypatch, need_gpu):
    """a direct grant D <- U written in place lands among S(U)'s raw entries: the next queued
    call allows it by the S head alone, and after its deletion denies it"""
    from tests.test_writes import _tuple
    ve, eng, namespaces, rows, reqs, roots, targets = _writable(monkeypatch, heads)
    id2name = {i: nm for nm, i in namespaces}
    want0 = np.asarray(C.comb_case()["want"])
    held = Counter(r[3] for r in rows if r[3])  # rows per user: a short S(U) keeps the grant inline
    i = next(j for j, (ns, o, r, s) in enumerate(reqs) if not want0[j] and o.startswith("D") and
             s["subject_id"].startswith("U") and held[s["subject_id"]] <= 3)
    grant = (1, reqs[i][1], "view", reqs[i][3]["subject_id"], None, None, None)
    want1 = np.asarray(randgraph.oracle_store(namespaces, rows + [grant]).check_batch(reqs), dtype=bool)
    assert want1[i] and not want0[i]
    q = eng.upload(roots, targets)
    q.run()
    words_ok(q, want0)
    queue(q)
    ve.transact(insert=[_tuple(grant, id2name)])
    assert ve.last_write["path"] == "in_place" and ve._state[1] is eng
    words_ok(q, want0)  # (queued before the write)
    queue(q)
    words_ok(q, want1)
    ve.transact(delete=[_tuple(grant, id2name)])
    assert ve.last_write["path"] == "in_place" and ve._state[1] is eng
    queue(q)
    words_ok(q, want0)
    assert eng.label_sfirst_launches() == 3


@gpu
@pytest.mark.parametrize("heads", [(8, 8), (32, 32)])
def test_nesting_write_leaves_the_queued_path(heads, monkeypatch, need_gpu):
    """a nesting edge between two components marks the roots above it (never relabelled
    here): requests may need the second stage, so run(pipelined=True) is not queued, no
    launch reads S first, and the answers equal the oracle"""
    from tests.test_writes import _tuple
    ve, eng, namespaces, rows, reqs, roots, targets = _writable(monkeypatch, heads, KETOGPU_LABEL_RELABEL_PERMILLE=1000)
    id2name = {i: nm for nm, i in namespaces}
    edge = (1, "g000", "member", None, 1, "h200", "member")
    assert edge not in rows
    want1 = np.asarray(randgraph.oracle_store(namespaces, rows + [edge]).check_batch(reqs), dtype=bool)
    q = eng.upload(roots, targets)
    q.run()
    queue(q)
    before = eng.label_sfirst_launches()
    assert before == 1
    ve.transact(insert=[_tuple(edge, id2name)])
    assert ve.last_write["path"] == "in_place" and ve._state[1] is eng
    assert q.run(pipelined=True) is False
    assert eng.last_stats()["label_marked"] > 0
    words_ok(q, want1)
    assert eng.label_sfirst_launches() == before


@gpu
def test_synchronized_statistics_do_not_depend_on_the_switch(monkeypatch, need_gpu):
    """a synchronized call with events over the 2,616 comb requests at 32,32: rows, entries,
    full_requests and rest_requests are equal with the switch at 0 and at 2, and no
    synchronized launch reads S first"""
    seen = []
    for sf in (0, 2):
        label_env(monkeypatch, (32, 32), KETOGPU_LABEL_SFIRST=sf)
        c = C.comb_case()
        eng = check.Engine(c["snap"])
        q = eng.upload(c["roots"], c["targets"])
        q.run()
        eng.set_events(True)
        q.run()
        np.testing.assert_array_equal(q.download(), c["want"])
        st = eng.last_stats()
        assert eng.label_sfirst_launches() == 0
        seen.append({k: st[k] for k in ("unit_rows", "unit_rev", "label_entries", "full_requests", "rest_requests")})
    assert seen[0]["unit_rows"] > 0 and seen[0]["full_requests"] > 0
    assert seen[0] == seen[1]
