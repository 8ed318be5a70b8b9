"""W ranks of the partitioned mode in ONE process, driven in lock-step (TEST ONLY).

load_world builds every rank's shard through the raw id exchange of include/ketogpu.h
(ketogpu_shard_counts / _set_layout / _queries / _answer / _apply / _claims / _check_claims:
what ketogpu_shard_exchange does over a communicator, here with the arrays moved by hand),
resolve_world resolves requests the way ketogpu_part_resolve_batch combines the ranks, and
Lockstep plays the round driver (part_round.cpp) over W step objects — CpuSteps (the Python
model tests/part_cpu.py) or DeviceSteps (the ketogpu_part_* steps of partition.hip on one
GPU) — and keeps what every step emitted and returned.  compare() then holds two traces
against each other record for record, so a lost, duplicated or misrouted record, a wrong
mask or a stale state bit shows at the level, source and destination rank where it happens
instead of (perhaps) in a final answer.
"""
import ctypes as C

import numpy as np

from keto_amd import _lib as L
from keto_amd import persistence
from tests.part_cpu import REC, CpuPartition, owner

NONE = L.NODE_NONE
SALT = 0x4B45544F
FORWARD, BACKWARD = 0, 1


class RankStub:
    """what keto_amd.partition.Shard and DevicePartition read of a communicator"""

    def __init__(self, rank, world):
        self.rank, self.world, self.cuda, self.group = rank, world, False, None


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


# ------------------------------------------------------------------ the raw id exchange
def build_shard(namespaces, rows, rank, world, page_size=100, salt=SALT, batch=97):
    """ketogpu_shard_builder_new / _append / _finish of one rank -> the shard handle (not yet
    exchanged)"""
    lib = L.lib()
    ns = [(n, int(i)) for n, i in namespaces]
    arr = (L.Namespace * max(len(ns), 1))(*[L.Namespace(i, L.b(n)) for n, i in ns])
    opts = L.ShardOpts(page_size, 0, rank, world, salt)
    b = C.c_void_p()
    L.check(lib.ketogpu_shard_builder_new(arr, len(ns), C.byref(opts), C.byref(b)))
    try:
        for i in range(0, max(len(rows), 1), batch):
            cols = persistence.columnar(rows[i:i + batch])
            L.check(lib.ketogpu_shard_builder_append(b, C.byref(L.row_batch(cols))))
    except BaseException:
        lib.ketogpu_shard_builder_free(b)
        raise
    h = C.c_void_p()
    L.check(lib.ketogpu_shard_builder_finish(b, C.byref(h)))
    return h


def shard_counts(h):
    c = np.zeros(3, dtype=np.uint64)
    L.check(L.lib().ketogpu_shard_counts(h, c.ctypes.data))
    return c


def shard_queries(h, world, capacity=None):
    """(hashes grouped by owner, counts[world]) of one rank"""
    lib = L.lib()
    n = int(lib.ketogpu_shard_query_count(h))
    cap = n if capacity is None else capacity
    q = np.zeros(max(cap, 1), dtype=np.uint64)
    cnt = np.zeros(world, dtype=np.uint64)
    L.check(lib.ketogpu_shard_queries(h, q.ctypes.data, cap, cnt.ctypes.data))
    return q[:n], cnt


def shard_answer(h, hashes):
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    ids = np.zeros(max(len(hashes), 1), dtype=np.uint32)
    L.check(L.lib().ketogpu_shard_answer(h, hashes.ctypes.data, len(hashes), ids.ctypes.data))
    return ids[:len(hashes)]


def shard_apply(h, ids, n=None):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    L.check(L.lib().ketogpu_shard_apply(h, _ptr(ids), len(ids) if n is None else n))


def shard_claims(h, world, capacity=None):
    """((key hash, node hash) pairs grouped by the key's owner, counts[world]) of one rank"""
    lib = L.lib()
    n = int(lib.ketogpu_shard_claim_count(h))
    cap = n if capacity is None else capacity
    p = np.zeros(max(2 * cap, 2), dtype=np.uint64)
    cnt = np.zeros(world, dtype=np.uint64)
    L.check(lib.ketogpu_shard_claims(h, p.ctypes.data, cap, cnt.ctypes.data))
    return p[:2 * n].reshape(-1, 2), cnt


def shard_check_claims(h, pairs):
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1)
    amb = C.c_uint64(0)
    L.check(L.lib().ketogpu_shard_check_claims(h, _ptr(pairs), len(pairs) // 2, C.byref(amb)))
    return int(amb.value)


def _segments(arr, counts):
    at = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    return [arr[at[o]:at[o + 1]] for o in range(len(counts))]


def exchange(handles):
    """the collective part of a load, by hand: layout, node ids, R4 claims -> the number of
    Subject.String() keys shared by two nodes (summed over their owners)"""
    world = len(handles)
    counts = np.concatenate([shard_counts(h) for h in handles])
    for h in handles:
        L.check(L.lib().ketogpu_shard_set_layout(h, counts.ctypes.data))
    asked = [shard_queries(h, world) for h in handles]
    for r, h in enumerate(handles):  # each segment answered by its owner, back in query order
        q, cnt = asked[r]
        ids = [shard_answer(handles[o], seg) for o, seg in enumerate(_segments(q, cnt))]
        shard_apply(h, np.concatenate(ids) if ids else np.zeros(0, np.uint32))
    claimed = [shard_claims(h, world) for h in handles]
    amb = 0
    for o, h in enumerate(handles):
        amb += shard_check_claims(h, np.concatenate([_segments(p, cnt)[o] for p, cnt in claimed]))
    return amb


def load_world(namespaces, rows, world, page_size=100, salt=SALT):
    """every rank's keto_amd.partition.Shard of one network, built in this process"""
    from keto_amd.partition import Shard
    handles = []
    try:
        for r in range(world):
            handles.append(build_shard(namespaces, rows, r, world, page_size, salt))
        amb = exchange(handles)
        if amb:
            raise L.KetoError(L.EINVAL, f"{amb} Subject.String() keys are shared by two nodes (R4)")
    except BaseException:
        for h in handles:
            L.lib().ketogpu_shard_free(h)
        raise
    ns = [(n, int(i)) for n, i in namespaces]
    return [Shard(h, RankStub(r, world), ns) for r, h in enumerate(handles)]


def resolve_world(shards, reqs):
    """requests -> (roots, targets, status): ketogpu_shard_resolve_batch on every rank; per id
    the smallest value wins with "not owned" mapped above "none" (the MIN all-reduce of
    ketogpu_part_resolve_batch), per status the largest"""
    cols = persistence.request_columns(reqs)  # stays referenced: the batch holds raw pointers
    rb = L.request_batch(cols)
    n = len(reqs)
    best = np.full((2, n), 0xFFFFFFFF, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    for sh in shards:
        r, t, st = (np.zeros(max(n, 1), dtype=dt) for dt in (np.uint32, np.uint32, np.int32))
        L.check(L.lib().ketogpu_shard_resolve_batch(sh.h, C.byref(rb), r.ctypes.data, t.ctypes.data, st.ctypes.data))
        for k, x in enumerate((r[:n], t[:n])):
            x = np.where(x == L.NODE_NOT_OWNED, 0xFFFFFFFF, np.where(x == NONE, 0xFFFFFFFE, x)).astype(np.uint32)
            best[k] = np.minimum(best[k], x)
        status = np.maximum(status, st[:n])
    del rb, cols
    best[best >= 0xFFFFFFFE] = NONE
    return best[0].copy(), best[1].copy(), status


def layout(shard):
    st = shard.stats()
    return int(st["num_interior"]), int(st["num_expandable"]), int(st["num_nodes"])


# ------------------------------------------------------------------------- step objects
def sort_records(rec):
    """records ordered by (a, b, m)"""
    return rec[np.lexsort((rec["m"], rec["b"], rec["a"]))] if len(rec) else rec


def records(rows):
    return np.array(rows, dtype=REC) if len(rows) else np.zeros(0, dtype=REC)


class CpuSteps:
    """the step interface of Lockstep over the Python model"""

    def __init__(self, view, words, capacity=1 << 20, model=CpuPartition):
        self.p = model(view, words=words)
        self.rank, self.world, self.cap = self.p.rank, self.p.world, capacity
        self.levels = 0

    def begin(self, roots, targets, direction):
        self.n = len(roots)
        return self.p.begin(roots, targets, direction)

    def emit(self, pull=False, capacity=None):
        cap = self.cap if capacity is None else capacity
        if pull:
            self.p.pull_emit()
        buf = np.zeros(max(min(cap, len(self.p.out)), 1), dtype=REC)  # what does not fit is not written
        counts = (C.c_uint64 * self.world)()
        rc = self.p.emit(0, buf.ctypes.data, cap, counts)
        counts = np.array(list(counts), dtype=np.int64)
        return rc, buf[:int(counts.sum())].copy(), counts

    def apply(self, rec):
        rec = np.ascontiguousarray(rec)
        fr = (C.c_uint64 * 1)()
        rc = self.p.apply(rec.ctypes.data, len(rec), fr)
        self.levels += 1
        return rc, int(fr[0])

    def expand(self):
        return self.p.expand()

    def pull_answer(self, rec):
        rec = np.ascontiguousarray(rec)
        return self.p.pull_answer(rec.ctypes.data, len(rec))

    def end(self):
        bits = (C.c_uint64 * max((self.n + 63) // 64, 1))()
        rc = self.p.end(bits)
        return rc, np.array(list(bits), dtype=np.uint64)

    def abort(self):
        return self.p.abort()

    def close(self):
        pass


class DeviceSteps:
    """the step interface of Lockstep over one rank's HIP partition: the ketogpu_part_*
    steps called directly, records in torch tensors on the GPU (int64, two words per
    record), downloaded after emit and uploaded before apply / pull_answer"""

    def __init__(self, shard, record_capacity, max_words_per_round, state_budget_bytes=32 << 20, device=0,
                 buffer_capacity=None):
        import torch
        from keto_amd.partition import DevicePartition
        self.torch = torch
        self.lib = L.lib()
        self.part = DevicePartition(shard, device, record_capacity=record_capacity,
                                    max_words_per_round=max_words_per_round, state_budget_bytes=state_budget_bytes)
        self.rank, self.world = shard.comm.rank, shard.comm.world
        self.cap = buffer_capacity or record_capacity
        dev = torch.device("cuda", device)
        self.send = torch.zeros(2 * self.cap, dtype=torch.int64, device=dev)
        self.recv = torch.zeros(2 * self.cap, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    @property
    def levels(self):
        return self.part.stats()["levels"]

    def begin(self, roots, targets, direction):
        self._roots = np.ascontiguousarray(roots, dtype=np.uint32)  # copied by the call; kept anyway
        self._targets = np.ascontiguousarray(targets, dtype=np.uint32)
        self.n = len(self._roots)
        return self.lib.ketogpu_part_begin_dir(self.part.h, _ptr(self._roots), _ptr(self._targets), self.n, direction)

    def emit(self, pull=False, capacity=None):
        cap = self.cap if capacity is None else capacity
        assert cap <= self.cap
        counts = np.zeros(self.world, dtype=np.uint64)
        fn = self.lib.ketogpu_part_pull_emit if pull else self.lib.ketogpu_part_emit
        rc = fn(self.part.h, self.send.data_ptr(), cap, counts.ctypes.data)
        counts = counts.astype(np.int64)
        n = int(counts.sum())
        if rc or not n:
            return rc, np.zeros(0, dtype=REC), counts
        assert n <= cap, f"rank {self.rank}: emit returned {n} records for a capacity of {cap}"
        if self.world == 1:  # the records are still where the kernels wrote them
            L.check(self.lib.ketogpu_part_sync(self.part.h))
        return rc, self.send[:2 * n].cpu().numpy().view(REC).copy(), counts

    def _upload(self, rec):
        rec = np.ascontiguousarray(rec)
        assert len(rec) <= self.cap
        if len(rec):
            self.recv[:2 * len(rec)].copy_(self.torch.from_numpy(rec.view(np.int64).copy()))
        self.torch.cuda.synchronize()  # the steps run on the partition's own stream
        return len(rec)

    def apply(self, rec):
        n = self._upload(rec)
        fr = C.c_uint64(0)
        rc = self.lib.ketogpu_part_apply(self.part.h, self.recv.data_ptr(), n, C.byref(fr))
        return rc, int(fr.value)

    def expand(self):
        return self.lib.ketogpu_part_expand(self.part.h)

    def pull_answer(self, rec):
        n = self._upload(rec)
        return self.lib.ketogpu_part_pull_answer(self.part.h, self.recv.data_ptr(), n)

    def end(self):
        bits = np.zeros(max((self.n + 63) // 64, 1), dtype=np.uint64)
        rc = self.lib.ketogpu_part_end(self.part.h, bits.ctypes.data)
        return rc, bits

    def abort(self):
        return self.lib.ketogpu_part_abort(self.part.h)

    def stats(self):
        return self.part.stats()

    def close(self):
        self.part.close()


# ----------------------------------------------------------------------------- the round
class Exchange:
    """one emit of every rank: sent[s][g] = the records rank s emitted for rank g, counts[s] =
    the per-destination counts its step returned, and what the receivers answered"""

    def __init__(self, sent, counts):
        self.sent, self.counts = sent, counts
        self.frontier = None

    def received(self, g):
        parts = [s[g].view(np.uint64) for s in self.sent if len(s[g])]  # (plain words: cheap to join)
        return np.concatenate(parts).view(REC) if parts else np.zeros(0, dtype=REC)

    def total(self):
        return int(sum(int(c.sum()) for c in self.counts))

    def crossed(self):
        """records whose destination is another rank"""
        return int(sum(int(c.sum()) - int(c[s]) for s, c in enumerate(self.counts)))


class Trace:
    """what one round's steps emitted and returned"""

    def __init__(self, n):
        self.n = n
        self.levels = []  # Exchange per BFS level
        self.pull = None
        self.bits = []    # per rank: the hit words of end

    def answer(self):
        w = np.bitwise_or.reduce(np.stack(self.bits), axis=0)
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:self.n].astype(bool)

    def records(self):
        return sum(x.total() for x in self.levels + [self.pull])

    def crossed(self):
        return sum(x.crossed() for x in self.levels + [self.pull])


class StepFailed(AssertionError):
    def __init__(self, what, rank, code, where=""):
        super().__init__(f"{where}{what} failed on rank {rank} with code {code}")
        self.what, self.rank, self.code = what, rank, code


class Lockstep:
    """W step objects driven through rounds the way ketogpu_part_check_ids drives them:
    begin_dir, then { emit, route by owner, apply, sum of frontiers, expand } until no rank
    has a frontier, then pull_emit, route, pull_answer, end.  With `lay` (Ni, Nx, N) every
    emit is held against itself at once (check_exchange), so a record in the wrong group is
    named where it is emitted, before its receiver refuses it."""

    def __init__(self, steps, lay=None):
        self.steps = steps
        self.world = len(steps)
        self.lay = lay
        self.where = ""  # of the step being run, for the messages
        assert [s.rank for s in steps] == list(range(self.world)) and all(s.world == self.world for s in steps)

    def _ok(self, what, rank, rc):
        if rc:
            raise StepFailed(what, rank, rc, self.where and self.where + ": ")

    def begin(self, roots, targets, direction):
        for s in self.steps:
            self._ok("begin", s.rank, s.begin(roots, targets, direction))

    def emit(self, pull=False, capacity=None):
        """every rank's emit -> Exchange (the groups split by the counts the step returned)"""
        sent, counts = [], []
        for s in self.steps:
            rc, rec, cnt = s.emit(pull, capacity)
            self._ok("pull_emit" if pull else "emit", s.rank, rc)
            sent.append(_segments(rec, cnt))
            counts.append(cnt)
        x = Exchange(sent, counts)
        if self.lay:
            check_exchange(x, self.lay, self.world, self.where or ("pull" if pull else "emit"))
        return x

    def apply(self, x):
        x.frontier = []
        for s in self.steps:
            rc, fr = s.apply(x.received(s.rank))
            self._ok("apply", s.rank, rc)
            x.frontier.append(fr)
        return sum(x.frontier)

    def expand(self):
        for s in self.steps:
            self._ok("expand", s.rank, s.expand())

    def abort(self):
        for s in self.steps:
            self._ok("abort", s.rank, s.abort())

    def finish(self, trace, where=""):
        self.where = f"{where}, pull"
        trace.pull = self.emit(pull=True)
        for s in self.steps:
            self._ok("pull_answer", s.rank, s.pull_answer(trace.pull.received(s.rank)))
        for s in self.steps:
            rc, bits = s.end()
            self._ok("end", s.rank, rc)
            trace.bits.append(bits)
        self.where = ""
        return trace

    def round(self, roots, targets, direction, where="round", max_levels=1000):
        trace = Trace(len(roots))
        self.where = f"{where}, begin"
        self.begin(roots, targets, direction)
        while True:
            assert len(trace.levels) < max_levels, f"{where}: the closure does not end"
            self.where = f"{where}, level {len(trace.levels)}"
            x = self.emit()
            trace.levels.append(x)
            if not self.apply(x):
                break
            self.expand()
        return self.finish(trace, where)

    def close(self):
        for s in self.steps:
            s.close()


def cpu_world(shards, words, model=CpuPartition):
    """a fresh set of model ranks"""
    return Lockstep([CpuSteps(sh.view(), words, model=model) for sh in shards], layout(shards[0]))


def device_world(shards, record_capacity, max_words_per_round, **kw):
    return Lockstep([DeviceSteps(sh, record_capacity, max_words_per_round, **kw) for sh in shards], layout(shards[0]))


# ------------------------------------------------------------------------------ compare
def _same_records(got, want, where):
    if not len(got) and not len(want):
        return
    got, want = sort_records(got), sort_records(want)
    if len(got) == len(want) and (got == want).all():
        return
    g, w = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
    fmt = lambda s: ", ".join(f"(a={a}, b={b}, m={m:#x})" for a, b, m in sorted(s)[:4])
    raise AssertionError(f"{where}: {len(got)} records, expected {len(want)}; only in got: {fmt(g - w) or '-'}; "
                         f"only in expected: {fmt(w - g) or '-'}")


def check_exchange(x, lay, world, where):
    """one trace against itself: the counts are the group sizes, every record of group g is
    owned by g"""
    Ni, Nx, _ = lay
    for s in range(world):
        for g in range(world):
            at = f"{where}, rank {s} -> rank {g}"
            assert int(x.counts[s][g]) == len(x.sent[s][g]), f"{at}: count {x.counts[s][g]} for {len(x.sent[s][g])} records"
            if len(x.sent[s][g]):
                o = owner(x.sent[s][g]["b"], Ni, Nx, world)
                assert (o == g).all(), f"{at}: {int((o != g).sum())} records belong to another rank"


def compare(got, want, lay, where="round"):
    """two traces of the same round, level by level and rank pair by rank pair: equal record
    multisets, counts, frontiers and hit bits.  The message names the round, the level and
    the (source, destination) ranks of the first difference."""
    world = len(want.bits)
    pairs = [(f"level {i}", a, b) for i, (a, b) in enumerate(zip(got.levels, want.levels))]
    for name, a, b in pairs + [("pull", got.pull, want.pull)]:
        at = f"{where}, {name}"
        if name == "pull":  # the levels before it matched: a different count shows here, not as a cut list
            assert len(got.levels) == len(want.levels), f"{where}: {len(got.levels)} levels, expected {len(want.levels)}"
        check_exchange(a, lay, world, at)
        for s in range(world):
            for g in range(world):
                _same_records(a.sent[s][g], b.sent[s][g], f"{at}, rank {s} -> rank {g}")
            assert list(a.counts[s]) == list(b.counts[s]), f"{at}, rank {s}: counts {a.counts[s]}, expected {b.counts[s]}"
        if b.frontier is not None:
            for s in range(world):
                assert a.frontier[s] == b.frontier[s], f"{at}, rank {s}: frontier {a.frontier[s]}, expected {b.frontier[s]}"
    for s in range(world):
        assert (got.bits[s] == want.bits[s]).all(), \
            f"{where}, end, rank {s}: hit bits {got.bits[s]}, expected {want.bits[s]}"
    return len(pairs) + 1  # compared steps
