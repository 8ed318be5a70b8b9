"""The global multi-word path (seed / expand / gather / pull kernels, Engine::round,
run_global) at its own edges: frontier-list overflow, the dense reset, the halving of the
round width and the passes over a single word's requests (split_word).

The lists are kept at their 65536-entry floor (state_budget_bytes = 1 MiB) and the graph is
a chain g0 -> g1 -> ... -> gL, gL holding one subject id: requests of one word rooted along
the chain append a node once per level in which another request's bit reaches it, so a
word's list use is known in closed form (tests/global_path_model.py, pinned to the engine's
own counters by the first test here).  Truth on the chain is analytic: g_a reaches every
subject id under gL, reaches the subject set g_b#m iff b > a, and reaches no unknown user.
"""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import global_path_model as M
from tests import randgraph

pytestmark = pytest.mark.gpu

CHAIN = 1500
BUDGET = 1 << 20
NONE = M.NODE_NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(autouse=True)
def global_path(monkeypatch):
    monkeypatch.setenv("KETOGPU_PATH", "global")


def chain_rows(ns=1, n=CHAIN):
    rows = [(ns, f"g{i:04d}", "m", None, ns, f"g{i + 1:04d}", "m") for i in range(n)]
    rows.append((ns, f"g{n:04d}", "m", "alice", None, None, None))
    return rows


class Chain:
    """a snapshot holding the chain (namespace `ns`), its node ids and request builders"""

    def __init__(self, snap, ns):
        self.snap, self.ns = snap, ns
        self.graph = snap.graph()
        self.alice = snap.resolve(ns, "g0000", "m", rt.SubjectID("alice"))[1]
        self.g = [snap.resolve(ns, f"g{i:04d}", "m", rt.SubjectID("alice"))[0] for i in range(CHAIN + 1)]
        assert self.alice != NONE and NONE not in self.g
        self.ni = snap.stats()["num_interior"]
        assert self.ni == self.graph["Ni"]
        self.cap = M.list_capacity(BUDGET)

    def width(self, max_words=0):
        return M.round_width(self.ni, self.cap, BUDGET, max_words)

    def request(self, a, kind):
        """a request rooted at g_a -> (root, target, truth).  kind 0: alice; 1: the subject
        set g_b#m a little further down (true); 2: g_b#m at or above the root (false); 3: an
        unknown user (target NODE_NONE: false, no search)"""
        if kind == 0:
            return self.g[a], self.alice, True
        if kind == 1:
            return self.g[a], self.g[min(a + 1 + a % 7, CHAIN)], a < CHAIN
        if kind == 2:
            return self.g[a], self.g[a - a % 5], False
        return self.g[a], NONE, False

    def word(self, starts, shift=0):
        """a word of 64 requests: chain roots g_a for a in `starts` on every (64 /
        len(starts))-th bit (targets of kinds 0..2), the other bits cheap requests without a
        search (the chain's end as root, unknown users, an unknown object)"""
        step = 64 // len(starts)
        r, t, w = [], [], []
        for b in range(64):
            if b % step == 0 and b // step < len(starts):
                x = self.request(starts[b // step], (b // step + shift) % 3)
            elif b % 3 == 0:
                x = self.g[CHAIN], self.alice, True  # no interior row: answered by the pull
            elif b % 3 == 1:
                x = self.request((7 * b + shift) % CHAIN, 3)
            else:
                x = NONE, self.alice, False
            r.append(x[0]), t.append(x[1]), w.append(x[2])
        return r, t, w

    def batch(self, words):
        r, t, w = [], [], []
        for x in words:
            r += x[0]
            t += x[1]
            w += x[2]
        return np.array(r, np.uint32), np.array(t, np.uint32), np.array(w, bool)


@pytest.fixture(scope="module")
def chain():
    c = Chain(Snapshot.from_rows([("n", 1)], chain_rows(), sort=True), "n")
    assert c.ni == CHAIN
    return c


def test_model_is_the_engine(chain):
    """a batch the model says fits: the engine's entries and levels are the model's"""
    r, t, want = chain.batch([chain.word([96 * k + 5 for k in range(16)])])
    cost = M.round_cost(chain.graph, r, t)
    assert cost["slots"] == sum(CHAIN - (96 * k + 5) for k in range(16)) <= chain.cap
    eng = check.Engine(chain.snap, state_budget_bytes=BUDGET)
    got, flags = eng.check_ids(r, t, with_flags=True)
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all() and not flags.any()
    st = eng.last_stats()
    print("model", cost["slots"], cost["levels"], "engine", st["frontier_entries"], st["levels"])
    assert st["hubs"] == 0 and st["plan"] == 0
    assert (st["frontier_entries"], st["levels"]) == (cost["slots"], cost["levels"])
    assert st["overflow_retries"] == 0 and st["rounds"] == 1


def retry_batch(chain, max_words):
    if max_words == 0:
        # 32 words of 16 chain roots 96 apart: 12000 to 12500 slots per word
        words = [chain.word([96 * k + w for k in range(16)], w) for w in range(32)]
    else:
        # 9 words of 16 chain roots 10 apart: 22000 to 23000 slots per word, so that three
        # words do not fit either and the width goes 7 -> 3 -> 1 over an odd word count
        words = [chain.word([10 * k + 3 * w for k in range(16)], w) for w in range(9)]
    return chain.batch(words)


@pytest.mark.parametrize("max_words", [0, 7])
def test_retry_that_succeeds(chain, max_words):
    r, t, want = retry_batch(chain, max_words)
    width = chain.width(max_words)
    plan = M.plan_rounds(chain.graph, r, t, width, chain.cap)
    first = M.round_cost(chain.graph, r[:64 * width], t[:64 * width])["slots"]
    print("width", width, "first round slots", first, "plan", plan)
    assert first > chain.cap and plan["retries"] > 0 and plan["split_words"] == 0
    if max_words == 7:
        assert width == 7 and plan["widths"][:3] == [7, 3, 1] and plan["retries"] == 2
    eng = check.Engine(chain.snap, max_words_per_round=max_words, state_budget_bytes=BUDGET)
    for _ in range(2):  # the second run finds the state the first one's dense resets left
        got, flags = eng.check_ids(r, t, with_flags=True)
        st = eng.last_stats()
        print({k: st[k] for k in ("overflow_retries", "rounds", "levels", "frontier_entries", "push_launches")})
        np.testing.assert_array_equal(got, want)
        assert not flags.any()
        assert st["overflow_retries"] == plan["retries"] and st["rounds"] == plan["rounds"]
        assert st["hubs"] == 0
    # an unrelated small batch afterwards
    r2, t2, w2 = chain.batch([chain.word([700, 1400], 1)])
    np.testing.assert_array_equal(eng.check_ids(r2[:50], t2[:50]), w2[:50])
    assert eng.last_stats()["overflow_retries"] == 0


def test_retry_with_flags():
    """the same shape on a snapshot with ambiguous Subject.String() keys: the flag words of
    a retried round are zeroed and raised again by the narrower rounds, bit for bit as an
    engine whose lists never overflow raises them"""
    seed = 33
    namespaces, rows = randgraph.make_graph(seed, n_rows=600, n_obj=30, n_users=40, collide=True, wildcard=False)
    ns_id = namespaces[-1][1]
    ns = namespaces[-1][0]
    rows = rows + chain_rows(ns_id)
    snap = Snapshot.from_rows(namespaces, rows, sort=True)
    assert snap.stats()["num_ambiguous_nodes"] > 0
    c = Chain(snap, ns)
    rnd = randgraph.make_requests(seed, namespaces, rows[:600], n=32 * 48, wildcard=False)
    rr, tt = snap.resolve_many([(a, o, r, rt.subject_from_dict(s)) for a, o, r, s in rnd])
    reqs, roots, targets = [], [], []
    k = 0
    for w in range(32):  # 16 chain roots per word, the other 48 requests random ones
        for b in range(64):
            if b % 4 == 0:
                a = 96 * (b // 4) + w
                roots.append(c.g[a])
                targets.append(c.alice)
                reqs.append((ns, f"g{a:04d}", "m", {"subject_id": "alice"}))
            else:
                roots.append(rr[k])
                targets.append(tt[k])
                reqs.append(rnd[k])
                k += 1
    roots, targets = np.array(roots, np.uint32), np.array(targets, np.uint32)
    width = c.width()
    plan = M.plan_rounds(c.graph, roots, targets, width, c.cap)
    print("Ni", c.ni, "width", width, "plan", plan)
    assert plan["retries"] > 0 and plan["split_words"] == 0
    small = check.Engine(snap, state_budget_bytes=BUDGET)
    big = check.Engine(snap)
    a1, f1 = small.check_ids(roots, targets, with_flags=True)
    st = small.last_stats()
    a2, f2 = big.check_ids(roots, targets, with_flags=True)
    assert st["overflow_retries"] == plan["retries"] and big.last_stats()["overflow_retries"] == 0
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(f1, f2)
    # every word of the first (failed) round was retried: a flag bit among them
    retried = 64 * plan["widths"][0]
    print("flag bits", int(f1.sum()), "in retried words", int(f1[:retried].sum()))
    assert f1[:retried].any()
    want = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    np.testing.assert_array_equal(a1, want)
    # (a flagged request's bit is final only after its sequential re-evaluation,
    # include/ketogpu.h ketogpu_check_ids: that path too)
    redo = np.flatnonzero(f1)
    again = small.check_many([rt.InternalRelationTuple(a, o, r, rt.subject_from_dict(s))
                              for a, o, r, s in (reqs[i] for i in redo)])
    assert again == [bool(x) for x in want[redo]]


def spread_word(c):
    """64 requests of one word rooted at g_0, g_8, ..., g_504"""
    r, t, w = [], [], []
    for k in range(64):
        x = c.request(8 * k, k % 3)
        r.append(x[0]), t.append(x[1]), w.append(x[2])
    return np.array(r, np.uint32), np.array(t, np.uint32), np.array(w, bool)


def test_one_word_that_cannot_fit_as_a_word(chain):
    """64 requests of one word spread along the chain need 79872 list slots, more than the
    65536 the lists hold, while each alone needs at most Ni + 1: the word is run in passes
    over halves of its requests (split_word).
    Before split_word: KetoError ENOMEM "frontier list overflow for a single 64-request word"."""
    r, t, want = spread_word(chain)
    need = M.round_cost(chain.graph, r, t)["slots"]
    assert need == 64 * CHAIN - 8 * 2016 == 79872 > chain.cap
    plan = M.plan_rounds(chain.graph, r, t, chain.width(), chain.cap)
    assert plan["split_words"] == 1 and plan["retries"] == 1 and plan["rounds"] == 2
    eng = check.Engine(chain.snap, state_budget_bytes=BUDGET)
    for _ in range(2):
        got, flags = eng.check_ids(r, t, with_flags=True)  # a host batch in pageable memory
        np.testing.assert_array_equal(got, want)
        assert not flags.any()
        st = eng.last_stats()
        assert (st["overflow_retries"], st["rounds"]) == (plan["retries"], plan["rounds"])
    q = eng.upload(r, t)  # HBM-resident
    for _ in range(2):
        q.run()
        np.testing.assert_array_equal(q.download(), want)
    # the word between words that fit, and as a short last word (its bits past n stay zero)
    ok = chain.word([700, 1400])
    r3, t3, w3 = chain.batch([ok, (list(r), list(t), list(want)), ok, (list(r[:41]), list(t[:41]), list(want[:41]))])
    plan3 = M.plan_rounds(chain.graph, r3, t3, chain.width(), chain.cap)
    assert plan3["split_words"] >= 1
    got = eng.check_ids(r3, t3)
    np.testing.assert_array_equal(got, w3)
    assert eng.last_stats()["overflow_retries"] == plan3["retries"]
    q3 = eng.upload(r3, t3)
    q3.run()
    ab, fb = q3.download_words()
    assert int(ab[-1]) >> 41 == 0 and not fb.any()


def test_one_word_split_after_the_spill_stages(monkeypatch):
    """the same 64 requests reach the global path as the spill batch of the LDS stages: every
    root top_k holds g_8k and the 9000-wide `top`, the targets T and V are below 9000 groups
    p_i (as test_gpu_parity.py test_unit_spill_to_global_path), so no LDS table holds either
    side; T is also below the chain's end, V is not"""
    monkeypatch.delenv("KETOGPU_PATH")
    monkeypatch.setenv("KETOGPU_UNITS", "bidi")
    monkeypatch.setenv("KETOGPU_HUBS", "0")  # (a hub root is looked up, not searched)
    n = 9000
    rows = chain_rows()
    rows += [(1, "top", "m", None, 1, f"f{i:05d}", "m") for i in range(n)]
    rows += [(1, f"f{i:05d}", "m", f"u{i}", None, None, None) for i in range(n)]
    rows += [(1, f"p{i:05d}", "m", None, 1, "T", "m") for i in range(n)]
    rows += [(1, f"p{i:05d}", "m", None, 1, "V", "m") for i in range(n)]
    rows += [(1, "z", "m", None, 1, f"p{i:05d}", "m") for i in range(n)]
    rows += [(1, f"g{CHAIN:04d}", "m", None, 1, "T", "m"), (1, "T", "m", "bob", None, None, None)]
    for k in range(64):
        rows += [(1, f"top{k:02d}", "m", None, 1, "top", "m"), (1, f"top{k:02d}", "m", None, 1, f"g{8 * k:04d}", "m")]
    snap = Snapshot.from_rows([("n", 1)], rows, sort=True)
    reqs, want = [], []
    for k in range(96):  # T at the end of the whole chain; nothing leads to V
        yes = k % 3 != 1
        reqs.append(("n", f"top{(2 * k // 3) % 64:02d}", "m", rt.SubjectSet("n", "T" if yes else "V", "m")))
        want.append(yes)
    assert len({r[1] for r, w in zip(reqs, want) if w}) == 64  # every root top_k against T once
    roots, targets = snap.resolve_many(reqs)
    assert NONE not in roots and NONE not in targets
    g = snap.graph()
    yes = np.flatnonzero(want)
    assert M.round_cost(g, roots[yes], targets[yes])["slots"] > M.list_capacity(BUDGET)
    eng = check.Engine(snap, state_budget_bytes=BUDGET)
    for _ in range(2):
        got = eng.check_ids(roots, targets)
        st = eng.last_stats()
        print({k: st[k] for k in ("spilled_requests", "overflow_retries", "rounds", "hubs")})
        np.testing.assert_array_equal(got, np.array(want))
        assert st["hubs"] == 0 and st["plan"] == 1
        # both sides 9000 wide: the 64 requests against T are left to the global path (the
        # LDS stages may decide those against V), where the word of spilled requests is split
        assert st["spilled_requests"] >= 64 and st["overflow_retries"] >= 1
