"""The global path's list-use model (tests/global_path_model.py) against closed forms on
graphs small enough to count by hand.  The GPU tests pin the same model to the engine's
own counters (tests/test_global_overflow_gpu.py) before using it to predict overflows."""
import pytest

from keto_amd.snapshot import Snapshot
from tests import global_path_model as M


def chain_snapshot(L):
    """g0 -> g1 -> ... -> gL, gL holds one subject id: g1..gL are the interior nodes"""
    rows = [(1, f"g{i:04d}", "m", None, 1, f"g{i + 1:04d}", "m") for i in range(L)]
    rows.append((1, f"g{L:04d}", "m", "alice", None, None, None))
    return Snapshot.from_rows([("n", 1)], rows, sort=True)


def node(snap, name):
    from keto_amd import relationtuple as rt
    return snap.resolve("n", name, "m", rt.SubjectID("alice"))


@pytest.fixture(scope="module")
def chain():
    L = 300
    snap = chain_snapshot(L)
    g = snap.graph()
    assert g["Ni"] == L
    ids = [node(snap, f"g{i:04d}")[0] for i in range(L + 1)]
    return L, g, ids, node(snap, "g0000")[1]


@pytest.mark.parametrize("a", [0, 1, 17, 298, 299])
def test_one_chain_request_needs_l_minus_a_entries(chain, a):
    L, g, ids, alice = chain
    c = M.round_cost(g, [ids[a]], [alice])
    assert c["slots"] == L - a and c["levels"] == L - a
    assert c["per_level"] == [1] * (L - a)


def test_requests_without_a_search_need_no_entry(chain):
    L, g, ids, alice = chain
    # the chain's end has no interior row; NODE_NONE roots and targets; a subject id as root
    c = M.round_cost(g, [ids[L], M.NODE_NONE, ids[0], alice], [alice, alice, M.NODE_NONE, alice])
    assert c == {"per_level": [], "slots": 0, "levels": 0}


@pytest.mark.parametrize("s", [1, 2, 4])
def test_64_spread_roots_of_one_word(chain, s):
    L, g, ids, alice = chain
    roots = [ids[k * s] for k in range(64)]
    c = M.round_cost(g, roots, [alice] * 64)
    assert c["slots"] == 64 * L - s * 2016  # sum over k of (L - k s)
    assert c["levels"] == L
    assert c["per_level"][0] == 64 and c["per_level"][-1] == 1


def test_words_of_a_round_add_up(chain):
    L, g, ids, alice = chain
    roots = [ids[5]] + [M.NODE_NONE] * 63 + [ids[250]]  # two words
    c = M.round_cost(g, roots, [alice] * 65)
    assert c["slots"] == (L - 5) + (L - 250) and c["levels"] == L - 5
    assert c["per_level"][:50] == [2] * 50 and c["per_level"][50] == 1


def test_diamond_shares_the_entry_of_a_level():
    # a -> b, a -> c, b -> d, c -> d, d -> e, e holds a user; x -> c.  Requests rooted at a
    # and at x, in one word.
    rows = [(1, "a", "m", None, 1, "b", "m"), (1, "a", "m", None, 1, "c", "m"), (1, "b", "m", None, 1, "d", "m"),
            (1, "c", "m", None, 1, "d", "m"), (1, "d", "m", None, 1, "e", "m"), (1, "e", "m", "alice", None, None, None),
            (1, "x", "m", None, 1, "c", "m")]
    snap = Snapshot.from_rows([("n", 1)], rows, sort=True)
    g = snap.graph()
    a, alice = node(snap, "a")
    x = node(snap, "x")[0]
    # one request: seed a; level 1: b, c; level 2: d once (reached from b and c in the same
    # level); level 3: nothing (e has no interior row)
    assert M.round_cost(g, [a], [alice])["per_level"] == [1, 2, 1]
    # both in one word: seeds a, x; level 1: b, c (c gains both requests' bits: one entry);
    # level 2: d gains both bits in the same level: one entry, not two
    assert M.round_cost(g, [a, x], [alice, alice])["per_level"] == [2, 2, 1]
    # in two words the same node is one entry per word
    c = M.round_cost(g, [a] + [M.NODE_NONE] * 63 + [x], [alice] * 65)
    assert c["per_level"] == [2, 3, 2]
    # a request that arrives a level later appends the node again
    b = node(snap, "b")[0]
    # roots a and b: level 0 a, b; level 1: b (from a), c (from a), d (from b); level 2: d
    # again (a's bit, from b and c); level 3: -
    assert M.round_cost(g, [a, b], [alice, alice])["per_level"] == [2, 3, 1]


def test_plan_rounds_halves_and_splits(chain):
    L, g, ids, alice = chain
    # four words of 300 - a slots each (one chain root per word)
    roots, targets = [], []
    for a in (0, 10, 20, 30):
        roots += [ids[a]] + [M.NODE_NONE] * 63
        targets += [alice] * 64
    total = sum(L - a for a in (0, 10, 20, 30))

    def plan(*a):
        p = M.plan_rounds(*a)
        p.pop("widths")
        return p
    assert M.plan_rounds(g, roots, targets, 4, total)["widths"] == [4]
    assert M.plan_rounds(g, roots, targets, 3, 400)["widths"] == [3, 1, 1, 1, 1]
    assert plan(g, roots, targets, 4, total) == {"retries": 0, "rounds": 1, "split_words": 0}
    # one slot short: halves once, two rounds of two words
    assert plan(g, roots, targets, 4, total - 1) == {"retries": 1, "rounds": 2, "split_words": 0}
    # 3 -> 1 over an odd width: [0,1,2] fails, then single words
    assert plan(g, roots, targets, 3, 400) == {"retries": 1, "rounds": 4, "split_words": 0}
    # a word of 64 spread roots that needs more than the lists hold: passes over halves
    roots = [ids[k] for k in range(64)]
    need = 64 * L - 2016
    half = 32 * L - 496  # the first half (roots 0..31) is the larger one
    assert M.round_cost(g, roots[:32], [alice] * 32)["slots"] == half
    assert plan(g, roots, [alice] * 64, 1, need) == {"retries": 0, "rounds": 1, "split_words": 0}
    assert plan(g, roots, [alice] * 64, 1, need - 1) == {"retries": 1, "rounds": 2, "split_words": 1}
    # the first half does not fit either: it is halved again, the second half runs whole
    assert plan(g, roots, [alice] * 64, 1, half - 1) == {"retries": 2, "rounds": 3, "split_words": 1}


def test_round_width_follows_the_constructor():
    # 1 MiB: lists 256 KiB -> 8192 entries, raised to the 65536 floor; 768 KiB of state
    assert M.list_capacity(1 << 20) == 65536
    assert M.round_width(1500, 65536, 1 << 20) == min((768 << 10) // (16 * 1500), 65536 // 1564) == 32
    assert M.round_width(1500, 65536, 1 << 20, max_words_per_round=7) == 7
    assert M.round_width(60000, 65536, 1 << 20) == 1
