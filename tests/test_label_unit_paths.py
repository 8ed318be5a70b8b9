"""Plan label's first stage (device_engine.hip label_unit) on the paths it takes from a
request's two heads in registers: the header words kept out of the one-edge test, the inline
landmark count, units whose 16 requests take different paths at once, and the statistics of
calls with events.  Every input is chosen and asserted on the CPU (tests/label_census.py,
tests/test_core_index.py first_stage) before any device call; every case then runs as an
HBM-resident batch (first and lean calls), pipelined, as host ids and as pinned host
requests read in place (label_host_kernel)."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import label_census as C
from tests import randgraph
from tests.test_core_index import NONE_, first_stage, label_answer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def label_env(monkeypatch, heads):
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", f"{heads[0]},{heads[1]}")


def restate(li, roots, targets, ni):
    """-> (requests the restated first stage leaves open, requests without label) of a batch"""
    hs, hp = li["s_head_words"], li["p_head_words"]
    n_open = n_rest = 0
    for r, t in zip(roots.tolist(), targets.tolist()):
        if r == NONE_ or t == NONE_:
            continue
        if int(li["S"][t * hs]) == NONE_ or int(li["P"][r * hp]) == NONE_:
            n_rest += 1
        else:
            n_open += first_stage(li, r, t, ni) is None
    return n_open, n_rest


def four_ways(eng, li, roots, targets, want, ni):
    """the batch through every way into label_unit: answers equal `want`, no bit is set past
    n, and every synchronized call lists exactly the restatement's requests"""
    n = len(roots)
    routed = restate(li, roots, targets, ni)

    def stats_ok():
        st = eng.last_stats()
        assert st["plan"] == 7 and st["label_on"] == 1
        assert (st["label_s_head"], st["label_p_head"]) == (li["s_head_words"], li["p_head_words"])
        assert (st["full_requests"], st["rest_requests"]) == routed

    q = eng.upload(roots, targets)
    for _ in range(3):  # the first call, then lean ones
        q.run()
        ab, fb = q.download_words()
        np.testing.assert_array_equal(check.unpack_bits(ab, n), want)
        if n % 64:
            assert int(ab[-1]) >> (n % 64) == 0  # no bit past n
        assert not fb.any()
        stats_ok()
    assert q.run(pipelined=True) and q.run(pipelined=True)
    eng.wait()
    np.testing.assert_array_equal(q.download(), want)
    np.testing.assert_array_equal(eng.check_ids(roots, targets), want)
    stats_ok()
    pr, pt = check.pinned(roots), check.pinned(targets)
    out = check.PinnedBuffer((n + 63) // 64, np.uint64)
    eng.check_ids_raw(pr.array.ctypes.data, pt.array.ctypes.data, n, out.array.ctypes.data)
    words = out.array.copy()
    np.testing.assert_array_equal(check.unpack_bits(words, n), want)
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0
    stats_ok()


# ------------------------------------------------------------------ 1. header-word collisions
COLLISION_SEED = 2


@functools.lru_cache(maxsize=None)
def collision_graph():
    """a random table (randgraph.make_graph, 300 rows) thinned to the subject sets of two
    objects: a handful of interior nodes, so that list lengths, mask words and overflow
    starts fall among the ids of the non-interior roots.  -> snapshot, the candidate requests
    (every root with rows x every subject) with ids and oracle answers"""
    namespaces, rows = randgraph.make_graph(COLLISION_SEED, n_rows=300, n_obj=14, n_rel=3, n_users=8, n_ns=1,
                                            wildcard=False)
    rows = [x for x in rows if x[3] is not None or x[5] in ("o0", "o1")]
    snap = Snapshot.from_rows(namespaces, rows, sort=True)
    name = {i: n for n, i in namespaces}
    heads_ = sorted({(name[x[0]], x[1], x[2]) for x in rows})
    subjects = [{"subject_id": u} for u in sorted({x[3] for x in rows if x[3] is not None})]
    subjects += [{"subject_set": {"namespace": name[a], "object": b, "relation": c}}
                 for a, b, c in sorted({(x[4], x[5], x[6]) for x in rows if x[3] is None})]
    reqs = [(ns, o, r, s) for ns, o, r in heads_ for s in subjects]
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    want = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    for a in (roots, targets, want):
        a.setflags(write=False)
    return {"snap": snap, "reqs": reqs, "roots": roots, "targets": targets, "want": want,
            "ni": int(snap.stats()["num_interior"])}


def collision_batch(heads):
    """the candidate requests whose non-interior root's id equals a header word of the
    target's S head and that the oracle denies, then as many other candidates
    -> (li, roots, targets, want, collisions per header word)"""
    g = collision_graph()
    li = g["snap"].label_index(*heads)
    hs, ni = li["s_head_words"], g["ni"]
    roots, targets, want = g["roots"], g["targets"], g["want"]
    some = (roots != NONE_) & (targets != NONE_)
    hit = np.zeros((4, len(roots)), dtype=bool)
    t64 = np.where(some, targets, 0).astype(np.int64)
    for j in range(4):
        hit[j] = some & (roots >= ni) & (li["S"][t64 * hs + j] == roots) & (li["S"][t64 * hs] != NONE_) & ~want
    pick = np.flatnonzero(hit.any(axis=0))
    others = np.setdiff1d(np.arange(len(roots)), pick)
    others = others[np.random.default_rng(5).permutation(len(others))[: max(len(pick), 64)]]
    order = np.random.default_rng(6).permutation(np.concatenate([pick, others]))
    return li, roots[order].copy(), targets[order].copy(), want[order].copy(), hit[:, pick].sum(axis=1)


@pytest.mark.parametrize("heads", [(8, 8), (32, 32), (64, 64)])
def test_header_words_are_no_entries(heads, monkeypatch):
    """a non-interior root whose id equals the count word, the overflow start or a mask word of
    the target's S head is not "among S's inline raw entries": the one-edge test compares the
    entry words only (with 8-word heads the header is the first two lanes' words, else the
    first lane's first four).  The batch holds oracle-denied collisions with the count word
    and with a mask word at every head pair, and with the overflow-start word at 8-word heads;
    at 32 and 64 words no list of this graph overflows (the word is 0, never a non-interior
    root), so no seed gives one there."""
    label_env(monkeypatch, heads)
    g = collision_graph()
    li, roots, targets, want, per_word = collision_batch(heads)
    assert (li["s_head_words"], li["p_head_words"]) == heads
    assert per_word[0] >= 1 and per_word[2] + per_word[3] >= 1, per_word
    assert (per_word[1] >= 1) == (heads == (8, 8)), per_word
    assert want.any() and not want.all()
    for i in range(len(roots)):
        assert label_answer(li, int(roots[i]), int(targets[i]), g["ni"]) == bool(want[i])
    four_ways(check.Engine(g["snap"]), li, roots, targets, want, g["ni"])


# ------------------------------------------------------------------ 2. the landmark count
def s_shapes(li, t, ni):
    """which of the four S-head shapes of the landmark count node t's head has"""
    hs = li["s_head_words"]
    cs = hs - 4
    ns = int(li["S"][t * hs])
    if ns == NONE_:
        return set()
    se = li["S"][t * hs + 4: t * hs + hs]
    es = int((se < ni).sum())
    out = set()
    if es == 0 and 0 < ns < ni:
        out.add("raw-only")  # (a count below ni right before the entries: no entry)
    if es == cs and ns == cs:
        out.add("exactly-cs-landmarks")
    if ns > cs and se[cs - 1] >= ni:
        out.add("overflow-last-raw")
    if ns > cs and se[cs - 1] < ni:
        out.add("overflow-last-landmark")
    return out


SHAPES = {"raw-only", "exactly-cs-landmarks", "overflow-last-raw", "overflow-last-landmark"}


@pytest.mark.parametrize("heads", [(8, 8), (32, 32), (64, 64)])
def test_landmark_count_shapes(heads, monkeypatch):
    """the inline landmark count (the entry words below ni, counted in registers and summed
    over the request's four lanes) on S heads with raw entries only, with exactly head - 4
    landmarks, and overflowing with the last inline entry raw / a landmark: the comb graph's
    requests on such targets, answers and both lists' totals against the restatement"""
    label_env(monkeypatch, heads)
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    assert (li["s_head_words"], li["p_head_words"]) == heads
    by_target = {int(t): s_shapes(li, int(t), c["ni"]) for t in set(c["targets"].tolist()) if t != NONE_}
    found = set().union(*by_target.values())
    assert found == SHAPES, found
    pick = np.array([t != NONE_ and bool(by_target[int(t)]) for t in c["targets"]])
    for shape in SHAPES:  # each shape among the chosen requests, labelled on both sides
        assert any(shape in by_target[int(t)] and r != NONE_ for r, t in zip(c["roots"][pick], c["targets"][pick]))
    four_ways(check.Engine(c["snap"]), li, c["roots"][pick].copy(), c["targets"][pick].copy(), c["want"][pick].copy(),
              c["ni"])


# ------------------------------------------------------------------ 3. mixed units
MIXED = ("landmark-walk-S", "landmark-walk-P", "settled-false", "dense", "none")


def last_walked_off_lane0(li, r, t, ni):
    """a landmark-walk hit whose only matching entry is the last walked one, on a lane other
    than the request's first (entry k is walked by lane k % 4)"""
    hs, hp = li["s_head_words"], li["p_head_words"]
    se = li["S"][t * hs + 4: t * hs + hs]
    es, ep = int((se < ni).sum()), min(int(li["P"][r * hp]), hp - 4)
    pe = li["P"][r * hp + 4: r * hp + 4 + ep]
    walked, other = (se[:es], pe) if es <= ep else (pe, se[:es])
    m = np.isin(walked, other)
    return bool(m[-1]) and m.sum() == 1 and (len(walked) - 1) % 4 != 0


@functools.lru_cache(maxsize=None)
def mixed_batch(heads):
    """the comb graph's requests permuted so that the first units of 16 each hold a hit of
    either walk, a settled denial, a dense request and a request with a NONE id (a kind the
    comb set has fewer of than units, such as the last, is repeated)
    -> (li, order into the comb requests, mixed units at the front)"""
    c = C.comb_case()
    li = c["snap"].label_index(*heads)
    ni = c["ni"]
    kinds = [C.classify(li, int(r), int(t), ni) for r, t in zip(c["roots"], c["targets"])]
    kinds = ["dense" if isinstance(k, tuple) else k for k in kinds]
    # "none" is also a head without label: here only a missing id (no head is marked)
    by = {k: [i for i, x in enumerate(kinds) if x == k] for k in MIXED}
    assert all((c["roots"][i] == NONE_) | (c["targets"][i] == NONE_) for i in by["none"])
    last = [i for k in MIXED[:2] for i in by[k]
            if last_walked_off_lane0(li, int(c["roots"][i]), int(c["targets"][i]), ni)]
    assert last, "no hit on the last walked entry off lane 0"
    for k in MIXED[:2]:  # such hits first
        by[k].sort(key=lambda i: i not in last)
    units = 12
    assert all(by[k] for k in MIXED)
    rng = np.random.default_rng(17)
    front = [[by[k][u % len(by[k])] for k in MIXED] for u in range(units)]  # (a scarce kind: repeated)
    used = {i for f in front for i in f}
    rest = [i for i in rng.permutation(len(kinds)).tolist() if i not in used]
    order = []
    for f in front:
        unit = f + [rest.pop() for _ in range(11)]
        order += [unit[i] for i in rng.permutation(16).tolist()]
    order = np.array(order + rest)
    mixed = 0
    for u in range(len(order) // 16):  # asserted per unit of the batch as it is sent
        mixed += set(MIXED) <= {kinds[i] for i in order[16 * u: 16 * u + 16]}
    assert mixed >= 8 and any(i in last for i in order[: 16 * units])
    order.setflags(write=False)
    return li, order, mixed


@pytest.mark.parametrize("heads", C.HEAD_PAIRS)
def test_mixed_units(heads, monkeypatch):
    """units whose 16 requests take every path of the first stage at once (hits of the walk
    over S and over P, among them one on the last walked entry off the request's first lane,
    settled denials, dense requests, missing ids), whole and cut at 1, 15, 16 and 17
    requests, with equal heads (one walk loop) and with 8/64 and 64/8 (two)"""
    label_env(monkeypatch, heads)
    c = C.comb_case()
    li, order, _ = mixed_batch(heads)
    eng = check.Engine(c["snap"])
    for n in (1, 15, 16, 17, len(order)):
        o = order[:n]
        four_ways(eng, li, c["roots"][o].copy(), c["targets"][o].copy(), c["want"][o].copy(), c["ni"])


# ------------------------------------------------------------------ 4. statistics with events
def test_statistics_with_events(monkeypatch):
    """a resident call with events reports 2 rows opened per labelled request and, from the
    first stage, ns + np + 4 entries read per labelled request (both lists and the header),
    computed from the head arrays; the entries counter also holds what the dense pass adds
    for the requests the first stage leaves open (their longer list once more), restated
    here too so that the total is asserted exactly.  A lean call in between (no statistics,
    no reduction in the kernel) leaves the next call's numbers unchanged"""
    heads = (32, 32)
    label_env(monkeypatch, heads)
    c = C.comb_case()
    li, order, _ = mixed_batch(heads)
    roots, targets, want = c["roots"][order].copy(), c["targets"][order].copy(), c["want"][order].copy()
    some = (roots != NONE_) & (targets != NONE_)
    ns = li["S"][targets[some].astype(np.int64) * heads[0]].astype(np.int64)
    np_ = li["P"][roots[some].astype(np.int64) * heads[1]].astype(np.int64)
    labelled = (ns != NONE_) & (np_ != NONE_)
    rows, entries = 2 * int(labelled.sum()), int((ns + np_ + 4)[labelled].sum())
    assert labelled.sum() > 1000
    # the same counter also takes the dense pass's reads (label_full_kernel: the longer list
    # of every request the first stage leaves open, once more)
    opened = np.array([first_stage(li, int(r), int(t), c["ni"]) is None for r, t in zip(roots[some], targets[some])])
    assert (opened <= labelled).all() and opened.any()
    entries += int(np.maximum(ns, np_)[opened].sum())
    eng = check.Engine(c["snap"])
    q = eng.upload(roots, targets)
    q.run()  # (the first call)

    def with_events():
        eng.set_events(True)
        q.run()
        np.testing.assert_array_equal(q.download(), want)
        st = eng.last_stats()
        assert (st["unit_rows"], st["unit_rev"]) == (rows, entries)

    with_events()
    eng.set_events(False)
    q.run()  # lean
    np.testing.assert_array_equal(q.download(), want)
    with_events()
