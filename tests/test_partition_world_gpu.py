"""The HIP steps of the partitioned mode (partition.hip) at world 1, 2, 3, 5 and 64 in ONE
process, in lock-step with the Python model (tests/part_cpu.py) — see tests/part_world.py.

Every rank is a DevicePartition on device 0; the test plays the round driver, moves the
records between the ranks through the host and compares, per round, level, source rank and
destination rank, the record multisets, the counts, the frontiers and the hit bits with a
fresh set of model ranks fed the same requests.  That makes visible what a comparison of
final answers hides: a vis bit that survives the asynchronous sparse reset, a record in the
wrong destination group, a lost or duplicated record, a wrong mask.

What stays unrun here ("Tests" of the partitioned mode): the grid caps of
part_apply_kernel (8192 blocks) and part_expand_kernel (4096 tiles), which need millions of
records in one step, and RCCL between distinct GPUs.
"""
import functools

import numpy as np
import pytest

from keto_amd import _lib as L
from tests import part_world as PW
from tests import randgraph
from tests.part_cpu import REC, owner
from tests.test_partition import _case, _want

pytestmark = pytest.mark.gpu

F, B = PW.FORWARD, PW.BACKWARD
DIRS = {F: "forward", B: "backward"}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def device_world(shards, record_capacity, max_words_per_round, **kw):
    """explicit sizes for every partition: the default state budget is a quarter of the free
    HBM per partition, and up to 64 partitions share the card here"""
    return PW.device_world(shards, record_capacity, max_words_per_round, **kw)


@functools.lru_cache(maxsize=None)
def world_case(world, seed):
    namespaces, rows, reqs = _case(seed)
    shards = PW.load_world(namespaces, rows, world)
    roots, targets, status = PW.resolve_world(shards, reqs)
    assert not status.any()
    want = _want(namespaces, rows, reqs)
    assert want.any() and not want.all()
    return shards, roots, targets, want


@functools.lru_cache(maxsize=None)
def _model_round(key, direction, words):
    """the reference of one round: a fresh set of model ranks (computed once per request
    slice, shared by the tests that run it, never modified)"""
    shards, roots, targets = _ROUNDS[key]
    return PW.cpu_world(shards, words).round(roots, targets, direction)


_ROUNDS = {}


def model_round(shards, roots, targets, direction, words):
    key = (id(shards[0]), roots.tobytes(), targets.tobytes())
    _ROUNDS[key] = (shards, roots, targets)
    return _model_round(key, direction, words)


class Tally:
    """what the lock-step comparisons of one test covered"""

    KEYS = ("records_sent", "records_received", "queries_answered", "levels")

    def __init__(self, dev):
        self.dev = dev
        self.rounds = self.steps = self.model_levels = self.records = self.crossed = 0
        self.delta = [dict.fromkeys(self.KEYS, 0) for _ in dev.steps]  # the partitions' counters over the rounds

    def round(self, shards, roots, targets, direction, words, where):
        """one round on the device ranks against a fresh model -> (device trace, model trace)"""
        want = model_round(shards, roots, targets, direction, words)
        where = f"{where}, {DIRS[direction]} round {self.rounds} of {len(roots)} requests"
        before = [s.stats() for s in self.dev.steps]
        got = self.dev.round(roots, targets, direction, where)
        for d, b, s in zip(self.delta, before, self.dev.steps):
            now = s.stats()
            for k in self.KEYS:
                d[k] += now[k] - b[k]
        self.steps += PW.compare(got, want, PW.layout(shards[0]), where)
        self.rounds += 1
        self.model_levels += len(want.levels)
        self.records += got.records()
        self.crossed += got.crossed()
        return got, want

    def check(self):
        """per test: the compared steps number at least the model's levels, records crossed
        ranks, and the partitions' own counters agree with the traces: every record a rank
        sent was received by a rank (as a BFS record by apply or as a pull query by
        pull_answer), and every rank made one apply per model level"""
        world = self.dev.world
        assert self.steps >= self.model_levels > 0
        assert self.records > 0 and (self.crossed > 0 or world == 1)
        d = lambda k: sum(x[k] for x in self.delta)
        assert d("records_sent") == d("records_received") + d("queries_answered") == self.records
        assert all(x["levels"] == self.model_levels for x in self.delta)


def run_all(dev, shards, roots, targets, direction, words, where):
    """every request in rounds of `words` words -> (answers, Tally)"""
    tally = Tally(dev)
    got = []
    for i in range(0, len(roots), words * 64):
        tr, _ = tally.round(shards, roots[i:i + words * 64], targets[i:i + words * 64], direction, words, where)
        got.append(tr.answer())
    return np.concatenate(got), tally


# ---------------------------------------------------------------------------- a. worlds
@pytest.mark.parametrize("direction", [F, B])
@pytest.mark.parametrize("world,seed,words", [(1, 62, 4), (1, 62, 8), (2, 62, 4), (3, 63, 4), (5, 64, 4), (64, 62, 4)])
def test_worlds_lockstep(world, seed, words, direction):
    """700 requests in rounds of `words` words (the last round ends in a partial word), one
    pass per direction.  World 64 is kMaxWorld, the size of the LDS histograms of the count
    and scatter kernels: 64 partitions and 128 streams in this process, record capacity 1 << 14."""
    shards, roots, targets, want = world_case(world, seed)
    dev = device_world(shards, 1 << 14, words)
    try:
        assert all(s.part.round_words() == words for s in dev.steps)
        got, tally = run_all(dev, shards, roots, targets, direction, words, f"world {world}")
        np.testing.assert_array_equal(got, want)
        assert len(roots) % 64 and tally.rounds == -(-len(roots) // (words * 64))
        tally.check()
    finally:
        dev.close()


def test_world1_send_buffer_before_and_after_sync():
    """world 1 leaves a step's records where the kernels wrote them (no pack copy): handed
    straight back, apply reads them there; after ketogpu_part_sync they are in the send
    buffer for any reader, and the buffer is the caller's again — apply then reads what the
    caller put into it.  (The lock-step rounds above always sync and apply from a second
    buffer.)"""
    import ctypes as C

    import torch
    shards, roots, targets, want = world_case(1, 62)
    r, t = roots[:256], targets[:256]
    model = model_round(shards, r, t, F, 4)
    assert len(model.levels) > 2
    dev = device_world(shards, 1 << 14, 4)
    try:
        s, lib = dev.steps[0], L.lib()
        dev.begin(r, t, F)
        s.send.fill_(-1)  # whatever the buffer held before
        torch.cuda.synchronize()
        counts, fr = np.zeros(1, dtype=np.uint64), C.c_uint64(0)
        L.check(lib.ketogpu_part_emit(s.part.h, s.send.data_ptr(), s.cap, counts.ctypes.data))
        assert int(counts[0]) == len(model.levels[0].sent[0][0])
        L.check(lib.ketogpu_part_apply(s.part.h, s.send.data_ptr(), int(counts[0]), C.byref(fr)))
        assert fr.value == model.levels[0].frontier[0] > 0
        dev.expand()
        rc, rec, cnt = s.emit()  # syncs: the records are in the send buffer now
        assert rc == 0
        PW._same_records(rec, model.levels[1].sent[0][0], "world 1, level 1 after ketogpu_part_sync")
        # n copies of one of these records in the caller's buffer: that is what apply sees
        n = len(rec)
        mine = np.repeat(rec[:1], n)
        s.send[:2 * n].copy_(torch.from_numpy(mine.view(np.int64).copy()))
        torch.cuda.synchronize()
        L.check(lib.ketogpu_part_apply(s.part.h, s.send.data_ptr(), n, C.byref(fr)))
        ref = PW.cpu_world(shards, 4)
        ref.begin(r, t, F)
        assert ref.apply(ref.emit()) == model.levels[0].frontier[0]
        ref.expand()
        ref.emit()
        rc, fr_model = ref.steps[0].apply(mine)
        assert fr.value == fr_model <= 1 < model.levels[1].frontier[0]
        dev.abort()
        got, _ = Tally(dev).round(shards, r, t, F, 4, "world 1 after the abort")
        np.testing.assert_array_equal(got.answer(), want[:256])
    finally:
        dev.close()


# --------------------------------------------------------------- b. state between rounds
def test_state_between_rounds_world3():
    """ONE set of partitions runs seven rounds — forward, backward, backward, forward, ... —
    over different request slices (a bit slot sees different requests), with a round aborted
    after its first level in the middle; every round against a fresh model, and the last
    round repeats the first: a vis or nxt bit that the sparse reset on the second stream
    (either buffer) or the dense reset of abort leaves behind shows as missing records."""
    shards, roots, targets, want = world_case(3, 63)
    words = 4
    dev = device_world(shards, 1 << 14, words)
    try:
        tally = Tally(dev)
        plan = [(F, 0), (B, 130), (B, 260), None, (F, 390), (F, 444), (B, 77), (F, 0)]
        traces = []
        for step in plan:
            if step is None:  # a round given up after one level: state, frontier and records exist
                dev.begin(roots[200:456], targets[200:456], F)
                x = dev.emit()
                assert dev.apply(x) > 0
                dev.expand()
                dev.abort()
                continue
            d, at = step
            got, model = tally.round(shards, roots[at:at + 256], targets[at:at + 256], d, words, "world 3")
            np.testing.assert_array_equal(got.answer(), want[at:at + 256])
            traces.append(got)
        assert tally.rounds == len(traces) == 7 >= 6
        assert PW.compare(traces[-1], traces[0], PW.layout(shards[0]), "the first round repeated") > 1
        seen = np.concatenate([want[at:at + 256] for _, at in filter(None, plan)])
        assert seen.any() and not seen.all()
        tally.check()
    finally:
        dev.close()


# --------------------------------------------------------------------- c. request edges
LENS = (0, 1, 63, 64, 65, 200)


def edge_rows():
    """one namespace, groups (object, "m"):
      p0..p199   pool groups with one user each (up_i): interior (expandable and a subject)
      L<k>       k in LENS: a root whose forward interior row is p0..p<k-1>; L0 holds only
                 the user u0 (a row of length 0); never a subject: expandable, not interior
      tu<k>      a user in p0..p<k-1>: rev(tu<k>) has k entries, all interior
      u0         in L0 only: rev(u0) has no interior entry;  mix: in L0 and p3
      top -> d0 -> {d1, d2} -> d3 -> ud       a diamond: paths split and merge
      entry -> c0 -> c1 -> c2 -> c0, c1 -> uc  a cycle
      k0 -> k1 -> kt0..kt11                    targets whose owner is on no node of the path
    """
    rows = []
    grp = lambda o, s: rows.append((1, o, "m", None, 1, s, "m"))
    usr = lambda o, u: rows.append((1, o, "m", u, None, None, None))
    for i in range(200):
        usr(f"p{i}", f"up{i}")
    for k in LENS:
        for j in range(k):
            grp(f"L{k}", f"p{j}")
            if k > 0:
                usr(f"p{j}", f"tu{k}")
    usr("L0", "u0")
    usr("L0", "mix")
    usr("p3", "mix")
    grp("top", "d0"), grp("d0", "d1"), grp("d0", "d2"), grp("d1", "d3"), grp("d2", "d3"), usr("d3", "ud"), usr("d0", "x0")
    grp("entry", "c0"), grp("c0", "c1"), grp("c1", "c2"), grp("c2", "c0"), usr("c1", "uc")
    grp("k0", "k1")
    for j in range(12):
        usr("k1", f"kt{j}")
    return [("n", 1)], randgraph.backend_sorted(rows)


def _sid(u):
    return {"subject_id": u}


def _set(o):
    return {"subject_set": {"namespace": "n", "object": o, "relation": "m"}}


def edge_requests():
    """named requests; the first 64 mix rows of every length in LENS on both sides"""
    q = lambda o, s: ("n", o, "m", s)
    reqs = [q(f"L{k}", _sid(f"tu{j}")) for k in LENS for j in LENS[1:]]                # 30: both sides, every length
    reqs += [q(f"L{k}", _set("L0")) for k in LENS]                                     # rev(L0#m) is empty
    reqs += [q("L0", _sid("u0")), q("L1", _sid("u0")), q("L0", _sid("mix")), q("L64", _sid("mix"))]  # r in rev(t), r not interior
    reqs += [q("p5", _sid("up5")), q("p5", _sid("tu1")), q("p0", _sid("tu1")), q("p7", _sid("mix"))]   # r in rev(t), r interior
    reqs += [q("L1", _set("p0")), q("L65", _set("p64")), q("L64", _set("p64"))]        # a rev row without interior entries
    reqs += [q("top", _sid("ud")), q("d0", _sid("ud")), q("d1", _sid("ud")), q("d3", _sid("x0")), q("top", _set("d3")),
             q("d0", _sid("x0")), q("top", _sid("x0"))]
    reqs += [q("entry", _sid("uc")), q("c0", _sid("uc")), q("c2", _sid("uc")), q("c1", _sid("ud")), q("c1", _set("c1")),
             q("entry", _set("c2"))]
    reqs += [q("k0", _sid(f"kt{j}")) for j in range(12)] + [q("k1", _sid("kt3")), q("top", _sid("kt3"))]
    reqs += [q("nothing", _sid("ud")), q("top", _sid("nobody")), q("nothing", _sid("nobody")), ("other", "top", "m", _sid("ud"))]
    reqs += [q(f"L{k}", _sid(f"up{i}")) for k in LENS for i in (0, 62, 63, 64, 199)]   # 30
    reqs += [q(f"p{i}", _sid(f"tu{k}")) for i in (0, 63, 199) for k in LENS[1:]]       # 15: interior roots, one-edge paths only
    return reqs


@functools.lru_cache(maxsize=None)
def edge_case():
    namespaces, rows = edge_rows()
    shards = PW.load_world(namespaces, rows, 3)
    reqs = edge_requests()
    roots, targets, status = PW.resolve_world(shards, reqs)
    assert not status.any()
    want = _want(namespaces, rows, reqs)
    Ni, Nx, N = lay = PW.layout(shards[0])
    models = [s.p for s in PW.cpu_world(shards, 1).steps]
    own = lambda v: int(owner(v, Ni, Nx, 3))
    gaps = [v for v in range(N) if models[own(v)].local(v) is None]
    gap = [next(v for v in gaps if lo <= v < hi) for lo, hi in ((0, Ni), (Ni, Nx), (Nx, N))]  # one per class
    name = {(r[0], r[1], str(r[3])): i for i, r in enumerate(reqs)}
    at = lambda o, s: name[("n", o, str(s))]
    # the cases the graph was built for, checked on the loaded shards
    i = at("p5", _sid("up5"))
    assert roots[i] < Ni and want[i]                                       # r in rev(t), r interior
    i = at("L0", _sid("u0"))
    assert Ni <= roots[i] < Nx and want[i]                                 # r in rev(t), r not interior
    rev = lambda t: models[own(t)]._rev(t)
    assert len(rev(targets[at("L1", _sid("tu200"))])) == 200 and max(rev(targets[at("L1", _sid("tu200"))])) < Ni
    assert rev(targets[i]) and min(rev(targets[i])) >= Ni                 # no interior entry
    assert rev(targets[at("L0", _set("L0"))]) == []
    assert [len(models[own(roots[at(f"L{k}", _sid("tu1"))])]._fint(roots[at(f"L{k}", _sid("tu1"))])) for k in LENS] == list(LENS)
    k0, k1 = roots[at("k0", _sid("kt0"))], roots[at("k1", _sid("kt3"))]
    far = [j for j in range(12) if own(targets[at("k0", _sid(f"kt{j}"))]) not in (own(k0), own(k1))]
    assert far and all(want[at("k0", _sid(f"kt{j}"))] for j in far)       # the target's owner is on no node of the path
    real_r, real_t = int(roots[at("top", _sid("ud"))]), int(targets[at("top", _sid("ud"))])
    special = [(PW.NONE, real_t), (real_r, PW.NONE), (PW.NONE, PW.NONE),
               (gap[0], real_t), (real_r, gap[0]), (gap[1], real_t), (real_r, gap[1]), (real_r, gap[2]), (gap[0], gap[2])]
    edge = [(Nx - 1, real_t), (real_r, N - 1), (Nx - 1, N - 1)]           # the last valid ids: answered
    twice = (int(roots[at("d0", _sid("ud"))]), int(targets[at("d0", _sid("ud"))]))
    r = list(map(int, roots))
    t = list(map(int, targets))
    w = list(map(bool, want))
    # special ids between the named requests of the first word; one request twice in the first
    # word and once more in the second
    for pos, (a, b) in zip((2, 9, 17, 23, 31, 38, 44, 50, 57, 5, 13, 27), special + edge):
        r.insert(pos, a), t.insert(pos, b), w.insert(pos, None if (a, b) in edge else False)
    for pos in (7, 41, 70):
        r.insert(pos, twice[0]), t.insert(pos, twice[1]), w.insert(pos, True)
    while len(r) < 257 + 7:  # longer batches repeat the list
        r, t, w = r + r[:64], t + t[:64], w + w[:64]
    return shards, np.array(r, dtype=np.uint32), np.array(t, dtype=np.uint32), w, lay


@pytest.mark.parametrize("direction", [F, B])
def test_request_edges_world3(direction):
    """batches of 1, 63, 64, 65, 255, 256 and 257 requests over the hand-built graph
    (edge_rows), one set of partitions: rows of 0, 1, 63, 64, 65 and 200 entries inside one
    wave of wave_emit, KETOGPU_NODE_NONE and unowned layout ids as root and target, both
    direct-hit branches, a diamond, a cycle, a repeated request; then ids outside the
    snapshot, which fail the round's first emit with KETOGPU_EINVAL on every rank"""
    shards, roots, targets, want, (Ni, Nx, N) = edge_case()
    words = 5
    dev = device_world(shards, 1 << 14, words)
    try:
        tally = Tally(dev)
        seen = []
        for k, size in enumerate((1, 63, 64, 65, 255, 256, 257)):
            r, t, w = roots[k:k + size], targets[k:k + size], want[k:k + size]
            got, model = tally.round(shards, r, t, direction, words, f"batch of {size}")
            known = np.array([x is not None for x in w])
            np.testing.assert_array_equal(model.answer()[known], np.array([bool(x) for x in w])[known])
            np.testing.assert_array_equal(got.answer(), model.answer())
            seen.append(got.answer())
        seen = np.concatenate(seen)
        assert seen.any() and not seen.all()
        # ids outside the snapshot: refused by the seed kernel, reported by the first emit
        for bad_r, bad_t in ((Nx, None), (None, N)):
            r, t = roots[:130].copy(), targets[:130].copy()
            if bad_r is not None:
                r[77] = bad_r
            else:
                t[77] = bad_t
            dev.begin(r, t, direction)
            for s in dev.steps:
                rc, rec, counts = s.emit()
                assert rc == L.EINVAL and not len(rec) and not counts.any(), (s.rank, rc, counts)
            dev.abort()
            got, model = tally.round(shards, roots[:130], targets[:130], direction, words, "after a refused round")
        tally.check()
    finally:
        dev.close()


# -------------------------------------------------------------------- d. capacity edges
def _drive(dev, roots, targets, direction, level):
    """a round up to the expansion whose records level `level`'s emit packs"""
    dev.begin(roots, targets, direction)
    for _ in range(level):
        x = dev.emit()
        assert dev.apply(x) > 0
        dev.expand()


@pytest.mark.parametrize("direction", [F, B])
def test_capacity_edges_world3(direction):
    """the largest step of a round (level l, rank q) emits n records: an emit capacity of n
    succeeds, n - 1 gives KETOGPU_ENOMEM with all counts zero, and so does a partition whose
    own record capacity is n - 1 (the steps before it fit); after ketogpu_part_abort on every
    rank (the dense reset) the same round with room equals the model record for record"""
    shards, roots, targets, want = world_case(3, 63)
    words = 4
    r, t = roots[:256], targets[:256]
    model = model_round(shards, r, t, direction, words)
    sizes = np.array([[int(c.sum()) for c in x.counts] for x in model.levels])
    n = int(sizes.max())
    level, q = map(int, np.argwhere(sizes == n)[0])  # the first step of that size, in the order the steps run
    assert n > 64
    dev = device_world(shards, 1 << 14, words)
    small = device_world(shards, n - 1, words, buffer_capacity=1 << 14)
    try:
        tally = Tally(dev)
        for cap, code in ((n - 1, L.ENOMEM), (n, 0)):
            _drive(dev, r, t, direction, level)
            rc, rec, counts = dev.steps[q].emit(capacity=cap)
            assert rc == code, (cap, rc)
            if code:
                assert not counts.any() and not len(rec)
            else:
                assert list(counts) == list(model.levels[level].counts[q])
                got = PW._segments(rec, counts)
                for g in range(3):
                    PW._same_records(got[g], model.levels[level].sent[q][g], f"capacity {n}, rank {q} -> rank {g}")
            dev.abort()
        got, _ = tally.round(shards, r, t, direction, words, "after two aborted rounds")
        np.testing.assert_array_equal(got.answer(), want[:256])
        assert want[:256].any() and not want[:256].all()
        tally.check()
        # the partition's own buffer: the kernels flag the record that does not fit
        _drive(small, r, t, direction, level)
        for s in small.steps[:q]:
            assert s.emit(capacity=1 << 14)[0] == 0
        rc, rec, counts = small.steps[q].emit(capacity=1 << 14)
        assert rc == L.ENOMEM and not counts.any()
        small.abort()
        tally = Tally(small)  # a round that fits: 64 requests
        m64 = model_round(shards, r[:64], t[:64], direction, words)
        assert max(int(c.sum()) for x in m64.levels + [m64.pull] for c in x.counts) < n
        tally.round(shards, r[:64], t[:64], direction, words, "record capacity n - 1, after abort")
        tally.check()
    finally:
        dev.close()
        small.close()


# ------------------------------------------ e. scatter tiles and the grid cap of pack
N_MID, FAN, N_BIG, N_STAR = 240, 80, 72, 72


def star_rows():
    """R<k> -> 80 of the groups m0..m239 (interior), T<c> -> one of them; m<j> -> n<j>
    (interior) -> the user w<j>: a second level exists, and it ends the closure"""
    rows = []
    grp = lambda o, s: rows.append((1, o, "m", None, 1, s, "m"))
    for j in range(N_MID):
        grp(f"m{j}", f"n{j}")
        rows.append((1, f"n{j}", "m", f"w{j}", None, None, None))
    for k in range(N_BIG):
        for j in range(FAN):
            grp(f"R{k}", f"m{(7 * k + j) % N_MID}")
    for c in range(N_STAR):
        grp(f"T{c}", f"m{(5 * c) % N_MID}")
    return [("n", 1)], randgraph.backend_sorted(rows)


@functools.lru_cache(maxsize=None)
def star_case():
    namespaces, rows = star_rows()
    shards = PW.load_world(namespaces, rows, 3)
    lay = Ni, Nx, N = PW.layout(shards[0])
    names = [f"R{k}" for k in range(N_BIG)] + [f"T{c}" for c in range(N_STAR)] + [f"m{j}" for j in range(N_MID)] + \
            [f"n{j}" for j in range(N_MID)]
    ids, _, st = PW.resolve_world(shards, [("n", o, "m", _sid("w0")) for o in names])
    _, w, st2 = PW.resolve_world(shards, [("n", "m0", "m", _sid(f"w{j}")) for j in range(N_MID)])
    assert not st.any() and not st2.any() and (ids != PW.NONE).all() and (w != PW.NONE).all()
    R, T = ids[:N_BIG], ids[N_BIG:N_BIG + N_STAR]
    m, n = ids[N_BIG + N_STAR:][:N_MID], ids[N_BIG + N_STAR + N_MID:]
    assert m.max() < Ni and n.max() < Ni and R.min() >= Ni and w.min() >= Nx
    own = lambda v: owner(v, Ni, Nx, 3)
    q = int(np.argmax(np.bincount(own(R), minlength=3)))  # the rank that owns most big roots
    big = np.flatnonzero(own(R) == q)[:16]
    star = np.flatnonzero(own(T) == q)[:17]
    assert len(big) == 16 and len(star) == 17
    return shards, lay, q, R, T, m, n, w, big, star


@pytest.mark.parametrize("direction", [F, B])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_scatter_tiles_world3(n, direction):
    """a step of exactly n records on one rank, one below, at and one above the 256-record
    tile of part_scatter_kernel: three roots of 80 interior successors and n - 240 of one,
    all owned by one rank (forward: the seed step; backward: the pull step)"""
    shards, lay, q, R, T, m, mid, w, big, star = star_case()
    roots = np.concatenate([R[big[:3]], T[star[:n - 240]]]).astype(np.uint32)
    # reachable by construction: the big roots' targets 5 and 79 places into their 80 successors
    # (100: outside), every second star root's own leaf user (the others: its neighbour)
    tj = [(7 * int(big[k]) + (5, 100, 79)[k]) % N_MID for k in range(3)] + \
         [(5 * int(c) + (k + 1) % 2) % N_MID for k, c in enumerate(star[:n - 240])]
    reach = np.array([True, False, True] + [k % 2 == 1 for k in range(n - 240)])
    targets = w[np.array(tj)].astype(np.uint32)
    dev = device_world(shards, 1 << 12, 1)
    try:
        tally = Tally(dev)
        got, model = tally.round(shards, roots, targets, direction, 1, f"a step of {n} records")
        x = model.pull if direction == B else model.levels[0]
        assert [int(c.sum()) for c in x.counts] == [n if s == q else 0 for s in range(3)]
        assert all(int(c) > 0 for c in x.counts[q])  # every destination gets a share of the tile
        np.testing.assert_array_equal(got.answer(), reach)
        tally.check()
    finally:
        dev.close()


def test_pack_grid_cap_world3():
    """one step above 2048 x 256 = 524 288 records on one rank, where part_count_kernel and
    part_scatter_kernel loop over their grid: 8192 requests (128 words) that repeat 16 roots
    of 80 interior successors, all owned by one rank.  The expected seed records come from
    the shard's rows with numpy (not through the model's Python loops); the frontier of the
    following apply is compared as a count and, through the records its expansion emits
    (every frontier node has one successor), as the set of (word, node, mask).  The only
    case with large buffers: 1 << 20 records per rank.  One forward round."""
    shards, lay, q, R, T, m, mid, w, big, star = star_case()
    Ni, Nx, N = lay
    nreq, words = 8192, 128
    i = np.arange(nreq)
    roots = R[big[i % 16]].astype(np.uint32)
    tj = (i * 37 + i // 16) % N_MID
    targets = w[tj].astype(np.uint32)
    reach = (tj - 7 * big[i % 16]) % N_MID < FAN
    assert reach.any() and not reach.all()
    # expected seed records: request i -> (i >> 6, u, 1 << (i & 63)) for u in fint(root), from
    # the owner's forward rows
    view = shards[q].view()
    model = PW.CpuPartition(view, words=words)
    loc = np.array([model.local(int(v)) for v in R[big]])
    off = view["lf_off"].astype(np.int64)
    rows16 = [view["lf_col"][off[l]:off[l + 1]] for l in loc]
    assert all(sorted(row.tolist()) == sorted(m[(7 * int(k) + np.arange(FAN)) % N_MID].tolist()) for row, k in zip(rows16, big))
    seed = np.zeros(nreq * FAN, dtype=REC)
    seed["a"] = np.repeat(i >> 6, FAN)
    seed["b"] = np.concatenate([rows16[k] for k in i % 16])
    seed["m"] = np.repeat(np.uint64(1) << (i & 63).astype(np.uint64), FAN)
    own = lambda v: owner(v, Ni, Nx, 3)
    # expected frontier: (word, m_j) with the bits of the word's requests whose root holds m_j
    has = np.zeros((16, N_MID), dtype=bool)
    for k, b in enumerate(big):
        has[k, (7 * int(b) + np.arange(FAN)) % N_MID] = True
    bits = np.zeros((words, 16), dtype=np.uint64)
    np.bitwise_or.at(bits, (i >> 6, i % 16), np.uint64(1) << (i & 63).astype(np.uint64))
    mask = np.zeros((words, N_MID), dtype=np.uint64)
    for k in range(16):
        mask[:, has[k]] |= bits[:, k:k + 1]
    wd, jj = np.nonzero(mask)
    dev = device_world(shards, 1 << 20, words)
    try:
        before = [s.stats() for s in dev.steps]
        assert all(s.part.round_words() == words for s in dev.steps)
        dev.begin(roots, targets, F)
        x = dev.emit()
        sizes = [int(c.sum()) for c in x.counts]
        assert sizes[q] == nreq * FAN > 2048 * 256 and sum(sizes) == sizes[q]
        PW.check_exchange(x, lay, 3, "seed step")
        for g in range(3):
            PW._same_records(x.sent[q][g], seed[own(seed["b"]) == g], f"seed step, rank {q} -> rank {g}")
        assert x.crossed() > 0
        assert dev.apply(x) == len(wd)
        assert x.frontier == [int((own(m[jj]) == g).sum()) for g in range(3)]
        dev.expand()
        trace = PW.Trace(nreq)
        y = dev.emit()
        PW.check_exchange(y, lay, 3, "level 1")
        nxt = np.zeros(len(wd), dtype=REC)
        nxt["a"], nxt["b"], nxt["m"] = wd, mid[jj], mask[wd, jj]
        for s in range(3):
            for g in range(3):
                PW._same_records(y.sent[s][g], nxt[(own(m[jj]) == s) & (own(mid[jj]) == g)], f"level 1, rank {s} -> rank {g}")
        assert dev.apply(y) == 0  # the n_j have no interior successor: vis-only entries, the closure ends
        trace.levels = [x, y]
        dev.finish(trace)
        assert trace.pull.total() == nreq  # rev(w_j) = {n_j}: one query per request
        np.testing.assert_array_equal(trace.answer(), reach)
        now = [s.stats() for s in dev.steps]
        d = lambda k: sum(a[k] - b[k] for a, b in zip(now, before))
        assert d("records_sent") == d("records_received") + d("queries_answered") == trace.records()
        assert all(a["levels"] - b["levels"] == 2 for a, b in zip(now, before))
    finally:
        dev.close()


# ----------------------------------------------------------------- f. misrouted records
@pytest.mark.parametrize("direction", [F, B])
def test_misrouted_records_are_refused_world3(direction):
    """a record for a node of another rank, for an unowned layout id and for an owned node
    that is not interior, handed to apply: KETOGPU_EINVAL with frontier 0; the same records
    in pull_answer, and a pull record with a >= n: KETOGPU_EINVAL; after abort the next
    round is correct.  Every apply record keeps its word inside the round (the driver's
    contract, include/ketogpu.h ketogpu_part_apply: the kernel indexes the state with it
    unchecked)."""
    shards, roots, targets, want = world_case(3, 63)
    Ni, Nx, N = lay = PW.layout(shards[0])
    words = 4
    r, t = roots[:256], targets[:256]
    models = [s.p for s in PW.cpu_world(shards, 1).steps]
    own = lambda v: int(owner(v, Ni, Nx, 3))
    gap = next(v for v in range(Ni) if models[own(v)].local(v) is None)
    dev = device_world(shards, 1 << 14, words)
    try:
        tally = Tally(dev)
        for case in range(6):
            g = case % 3
            foreign = next(v for v in range(Ni) if own(v) != g and models[own(v)].local(v) is not None)
            mine = next(v for v in range(Ni) if own(v) == g and models[g].local(v) is not None)
            outer = next(v for v in range(Ni, N) if own(v) == g and models[g].local(v) is not None)
            dev.begin(r, t, direction)
            x = dev.emit()
            good = x.received(g)
            if case < 3:  # apply: word 0 of the round, a node that is not this rank's interior node
                bad = PW.records([(0, (foreign, gap, outer)[case], 1)])
                rc, fr = dev.steps[g].apply(np.concatenate([good, bad]))
                assert (rc, fr) == (L.EINVAL, 0), (case, rc, fr)
            else:
                rc, fr = dev.steps[g].apply(good)
                assert rc == 0
                bad = PW.records([[(5, foreign, 0)], [(5, gap, 0)], [(len(r), mine, 0)]][case - 3])
                ok = PW.records([(len(r) - 1, mine, 0)])
                assert dev.steps[g].pull_answer(ok) == 0
                assert dev.steps[g].pull_answer(np.concatenate([ok, bad])) == L.EINVAL, case
            dev.abort()
            if case in (2, 5):
                got, _ = tally.round(shards, r, t, direction, words, f"after refused records (case {case})")
                np.testing.assert_array_equal(got.answer(), want[:256])
        assert want[:256].any() and not want[:256].all()
        tally.check()
    finally:
        dev.close()
