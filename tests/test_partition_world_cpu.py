"""The partitioned mode at world 1, 2, 3, 5 and 64 without a GPU: every rank's shard loaded
in this process through the raw id exchange (tests/part_world.py load_world: the
ketogpu_shard_counts / _set_layout / _queries / _answer / _apply / _claims / _check_claims
calls that otherwise only run inside ketogpu_shard_exchange), W Python model ranks
(tests/part_cpu.py) driven in lock-step against the oracle, and the refusals of the raw
exchange calls, each with its error code.  tests/test_partition_world_gpu.py holds the HIP
steps against this model record for record."""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from tests import part_world as PW
from tests.test_partition import _case, _want

WORLDS = [(1, 62), (2, 62), (3, 63), (5, 64), (64, 62)]
WORDS = 3


@functools.lru_cache(maxsize=None)
def world_case(world, seed):
    namespaces, rows, reqs = _case(seed)
    shards = PW.load_world(namespaces, rows, world)
    roots, targets, status = PW.resolve_world(shards, reqs)
    assert not status.any()
    return shards, roots, targets, _want(namespaces, rows, reqs)


@functools.lru_cache(maxsize=None)
def run(world, seed, direction):
    """all requests in rounds of WORDS words -> (answers, records, records to another rank)"""
    shards, roots, targets, _ = world_case(world, seed)
    got, total, crossed = [], 0, 0
    for i in range(0, len(roots), WORDS * 64):
        lock = PW.cpu_world(shards, WORDS)
        tr = lock.round(roots[i:i + WORDS * 64], targets[i:i + WORDS * 64], direction)
        lay = PW.layout(shards[0])
        for k, x in enumerate(tr.levels + [tr.pull]):
            PW.check_exchange(x, lay, world, f"requests {i}.., step {k}")
        got.append(tr.answer())
        total += tr.records()
        crossed += tr.crossed()
    return np.concatenate(got), total, crossed


@pytest.mark.parametrize("direction", [PW.FORWARD, PW.BACKWARD])
@pytest.mark.parametrize("world,seed", WORLDS)
def test_lockstep_model_matches_oracle(world, seed, direction):
    shards, roots, targets, want = world_case(world, seed)
    got, total, crossed = run(world, seed, direction)
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all()
    assert total > 0
    stats = [sh.stats() for sh in shards]
    Ni, Nx, N = PW.layout(shards[0])
    assert all(PW.layout(sh) == (Ni, Nx, N) for sh in shards)
    owned = sum(st["owned_nodes"] for st in stats)
    if world > 1:
        assert crossed > 0  # records really crossed ranks
        assert N > owned    # the layout has ids that no rank owns
    else:
        assert crossed == 0 and N == owned
    # together the ranks hold the whole graph once
    single = world_case(1, seed)[0][0].stats()
    for key in ("owned_nodes", "forward_edges", "reverse_edges"):
        assert sum(st[key] for st in stats) == single[key], key


@pytest.mark.parametrize("direction", [PW.FORWARD, PW.BACKWARD])
def test_record_totals_do_not_depend_on_the_world_size(direction):
    """a record is one (request bit set, node) pair of a level or one pull query: which rank
    sends it changes with the world size, how many there are does not"""
    totals = {w: run(w, 62, direction)[1] for w, s in WORLDS if s == 62}
    assert len(totals) == 3 and len(set(totals.values())) == 1, totals


def test_every_layout_gap_is_denied_without_error():
    """ids of the layout that no rank owns (world 3: the class ranges are padded to the
    largest rank) are valid request ids: denied, not refused"""
    shards, roots, targets, _ = world_case(3, 63)
    Ni, Nx, N = PW.layout(shards[0])
    models = PW.cpu_world(shards, WORDS).steps
    gaps = [v for v in range(N) if models[int(PW.owner(v, Ni, Nx, 3))].p.local(v) is None]
    assert gaps and any(v < Ni for v in gaps) and any(v >= Nx for v in gaps)
    gaps = gaps[:WORDS * 32]
    real = int(roots[roots != PW.NONE][0])
    r = np.array([real] * len(gaps) + [v for v in gaps if v < Nx], dtype=np.uint32)
    t = np.array(gaps + [int(targets[targets != PW.NONE][0])] * (len(r) - len(gaps)), dtype=np.uint32)
    for direction in (PW.FORWARD, PW.BACKWARD):
        assert not PW.cpu_world(shards, WORDS).round(r[:WORDS * 64], t[:WORDS * 64], direction).answer().any()


# ------------------------------------------------------- refusals of the raw exchange
NS = [("a", 1), ("a:b", 2)]
ROWS = [(1, "o", "r", "u", None, None, None), (1, "o", "r", None, 1, "p", "r"), (1, "p", "r", "v", None, None, None),
        (1, "q", "r", None, 1, "o", "r")]


def _code(fn, *a, **kw):
    with pytest.raises(L.KetoError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


@pytest.fixture
def two():
    hs = [PW.build_shard(NS, ROWS, r, 2) for r in range(2)]
    yield hs
    for h in hs:
        L.lib().ketogpu_shard_free(h)


def _set_layout(hs):
    counts = np.concatenate([PW.shard_counts(h) for h in hs])
    for h in hs:
        L.check(L.lib().ketogpu_shard_set_layout(h, counts.ctypes.data))
    return counts


def test_set_layout_refuses_counts_without_the_ranks_own(two):
    counts = np.concatenate([PW.shard_counts(h) for h in two])
    assert counts.sum() == 5  # o#r, p#r, q#r, u, v
    r = int(np.flatnonzero(counts.reshape(2, 3).sum(axis=1))[0])
    bad = counts.copy()
    bad[3 * r:3 * r + 3] += 1
    rc = L.lib().ketogpu_shard_set_layout(two[r], bad.ctypes.data)
    assert rc == L.EINVAL and b"own" in L.lib().ketogpu_last_error()
    L.check(L.lib().ketogpu_shard_set_layout(two[r], counts.ctypes.data))


def test_queries_and_answer_need_the_layout(two):
    code, msg = _code(PW.shard_queries, two[0], 2)
    assert code == L.EINVAL and "set_layout" in msg
    code, msg = _code(PW.shard_answer, two[0], [1])
    assert code == L.EINVAL and "set_layout" in msg


def test_answer_refuses_a_hash_of_another_rank(two):
    _set_layout(two)
    asked = [PW.shard_queries(h, 2) for h in two]
    segs = [PW._segments(q, cnt) for q, cnt in asked]
    # a hash that belongs to rank o, asked of rank 1 - o
    o = next(o for o in range(2) if any(len(s[o]) for s in segs))
    foreign = next(s[o] for s in segs if len(s[o]))
    assert len(PW.shard_answer(two[o], foreign)) == len(foreign)
    code, msg = _code(PW.shard_answer, two[1 - o], foreign[:1])
    assert code == L.EINVAL and "does not own" in msg
    code, msg = _code(PW.shard_answer, two[o], [12345])  # owned by nobody: no such node
    assert code == L.EINVAL


def test_apply_refuses_a_wrong_count_and_an_id_outside_the_layout(two):
    counts = _set_layout(two)
    N = int(2 * counts.reshape(2, 3).max(axis=0).sum())
    asked = [PW.shard_queries(h, 2) for h in two]
    r = next(r for r in range(2) if len(asked[r][0]) >= 2)
    q, cnt = asked[r]
    ids = np.concatenate([PW.shard_answer(two[o], seg) for o, seg in enumerate(PW._segments(q, cnt))])
    assert ids.max() < N
    code, msg = _code(PW.shard_apply, two[r], ids[:-1])
    assert code == L.EINVAL and "do not match" in msg
    bad = ids.copy()
    bad[0] = N
    code, msg = _code(PW.shard_apply, two[r], bad)
    assert code == L.EINVAL and "outside the layout" in msg
    PW.shard_apply(two[r], ids)


def test_query_and_claim_buffers_one_entry_short():
    from tests import randgraph
    h = PW.build_shard(NS, randgraph.backend_sorted(ROWS + [(1, "s", "r", "a:b#c", None, None, None)]), 0, 1)
    try:
        _set_layout([h])
        nq, nc = int(L.lib().ketogpu_shard_query_count(h)), int(L.lib().ketogpu_shard_claim_count(h))
        assert nq >= 2 and nc >= 2
        code, msg = _code(PW.shard_queries, h, 1, capacity=nq - 1)
        assert code == L.ENOMEM and "query buffer" in msg
        assert len(PW.shard_queries(h, 1, capacity=nq)[0]) == nq
        code, msg = _code(PW.shard_claims, h, 1, capacity=nc - 1)
        assert code == L.ENOMEM and "claim buffer" in msg
        assert len(PW.shard_claims(h, 1, capacity=nc)[0]) == nc
    finally:
        L.lib().ketogpu_shard_free(h)


def test_shared_string_key_meets_at_one_owner():
    """the subject id "a:b#c" and the subject set a:b#c are two nodes with one String() key
    (R4): wherever the two live, their claims travel to the key's owner, which counts it"""
    from tests import randgraph
    rows = randgraph.backend_sorted(ROWS + [(1, "s", "r", "a:b#c", None, None, None), (1, "t", "r", None, 1, "b", "c")])
    world = 3
    hs = [PW.build_shard(NS, rows, r, world) for r in range(world)]
    try:
        _set_layout(hs)
        for r, h in enumerate(hs):
            q, cnt = PW.shard_queries(h, world)
            PW.shard_apply(h, np.concatenate([PW.shard_answer(hs[o], seg) for o, seg in enumerate(PW._segments(q, cnt))]))
        claimed = [PW.shard_claims(h, world) for h in hs]
        got = [np.concatenate([PW._segments(p, cnt)[o] for p, cnt in claimed]) for o in range(world)]
        amb = [PW.shard_check_claims(hs[o], got[o]) for o in range(world)]
        assert sorted(amb) == [0, 0, 1]
        shared = got[int(np.argmax(amb))]
        keys, n = np.unique(shared[:, 0], return_counts=True)
        assert (n == 2).sum() == 1  # one key, claimed by two different nodes
        pair = shared[shared[:, 0] == keys[n == 2][0]]
        assert pair[0, 1] != pair[1, 1]
    finally:
        for h in hs:
            L.lib().ketogpu_shard_free(h)
    code, msg = _code(PW.load_world, NS, rows, world)
    assert code == L.EINVAL and "String()" in msg
    assert len(PW.load_world(NS, randgraph.backend_sorted(ROWS), world)) == world


def test_world_65_is_refused_by_the_shard_builder():
    """64 ranks is the size of the LDS histograms in partition.hip's count and scatter
    kernels; the builder already refuses more, so no partition of 65 ranks can be made"""
    code, msg = _code(PW.build_shard, NS, ROWS, 0, 65)
    assert code == L.EINVAL and "world <= 64" in msg
    code, msg = _code(PW.build_shard, NS, ROWS, 64, 64)  # rank < world
    assert code == L.EINVAL
    L.lib().ketogpu_shard_free(PW.build_shard(NS, ROWS, 63, 64))
