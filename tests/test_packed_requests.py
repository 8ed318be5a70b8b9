"""Packed 24-bit request batches (ketogpu_check_ids_packed24): 6 bytes per request, root
then target, three bytes each little-endian, 0xFFFFFF = NONE, in one 8-byte aligned buffer
of ketogpu_packed24_bytes(n) bytes.

CPU: the layout byte for byte, the host pack / unpack pair against a numpy formula, ids the
format cannot hold.  GPU: the packed call against the oracle and, word for word, against the
u32 call, on both device paths (unpack24_kernel ahead of any plan's first stage;
label_host_packed_kernel reading a pinned buffer in place), ids outside the snapshot,
pointers into the middle of a pinned buffer and the multi-GPU split."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check, synth
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import randgraph

NONE = 0xFFFFFFFF


def np_pack24(roots, targets):
    """the format restated in numpy, independent of ketogpu_pack24"""
    r = np.where(roots == NONE, 0xFFFFFF, roots).astype(np.uint32)
    t = np.where(targets == NONE, 0xFFFFFF, targets).astype(np.uint32)
    cols = [r & 255, (r >> 8) & 255, (r >> 16) & 255, t & 255, (t >> 8) & 255, (t >> 16) & 255]
    body = np.stack(cols, axis=1).astype(np.uint8).ravel()
    return np.concatenate([body, np.zeros((6 * len(r) + 7) // 8 * 8 - 6 * len(r), dtype=np.uint8)])


# ------------------------------------------------------------------------------- CPU
def test_layout_byte_for_byte():
    p = check.pack24(np.array([0x010203], dtype=np.uint32), np.array([0xA0B0C0], dtype=np.uint32))
    assert p.dtype == np.uint8 and p.tolist() == [0x03, 0x02, 0x01, 0xC0, 0xB0, 0xA0, 0, 0]
    p = check.pack24(np.array([NONE, 5], dtype=np.uint32), np.array([7, NONE], dtype=np.uint32))
    assert p.tolist() == [0xFF, 0xFF, 0xFF, 7, 0, 0, 5, 0, 0, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0]  # padding: 0
    r, t = check.unpack24(p, 2)
    assert r.tolist() == [NONE, 5] and t.tolist() == [7, NONE]
    for n in (0, 1, 2, 3, 4, 5, 64, 65):
        assert L.lib().ketogpu_packed24_bytes(n) == check.packed24_bytes(n) == (6 * n + 7) // 8 * 8
    assert len(check.pack24(np.zeros(0, np.uint32), np.zeros(0, np.uint32))) == 0


def test_round_trip_against_numpy():
    rng = np.random.default_rng(24)
    roots = rng.integers(0, 0xFFFFFF, 1000, dtype=np.uint32)  # [0, 0xFFFFFE]
    targets = rng.integers(0, 0xFFFFFF, 1000, dtype=np.uint32)
    roots[[0, 999]] = 0xFFFFFE
    targets[[1, 998]] = 0
    roots[rng.integers(0, 1000, 60)] = NONE
    targets[rng.integers(0, 1000, 60)] = NONE
    for n in (1000, 999, 3, 1):
        p = check.pack24(roots[:n], targets[:n])
        assert len(p) == check.packed24_bytes(n) and p.ctypes.data % 8 == 0
        np.testing.assert_array_equal(p, np_pack24(roots[:n], targets[:n]))
        r, t = check.unpack24(p, n)
        np.testing.assert_array_equal(r, roots[:n])
        np.testing.assert_array_equal(t, targets[:n])


@pytest.mark.parametrize("bad", [0xFFFFFF, 0xFFFFFFFE])
def test_pack24_rejects_ids_past_24_bits(bad):
    for side in (0, 1):
        ids = [np.arange(20, dtype=np.uint32), np.arange(20, dtype=np.uint32)]
        ids[side][13] = bad
        with pytest.raises(L.KetoError) as e:
            check.pack24(*ids)
        assert e.value.code == L.EINVAL and "request 13 " in str(e.value)


def test_small_snapshot_is_packed24_ok():
    """(the false case needs a snapshot of more than 16.7 M nodes and is not tested)"""
    snap = Snapshot.from_rows([("n", 1)], [(1, "o", "r", "u", None, None, None)])
    assert snap.packed24_ok() is True
    assert L.lib().ketogpu_snapshot_packed24_ok(None) == 0


def test_profile_family_of_the_packed_first_stage():
    """tools/pmc_traffic.py attributes the packed first stage's counters to a family of its
    own, not to none and not to label_host_kernel's"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "pmc_traffic", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "pmc_traffic.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    ns = "(anonymous namespace)::"
    assert m.family(f"void {ns}label_host_packed_kernel<32, 32>({ns}DevGraph)") == \
        "label_host_packed_kernel (host batches, packed24 requests)"
    assert m.family(f"void {ns}label_host_kernel<32, 32>({ns}DevGraph)") == "label_host_kernel (host batches)"


# ------------------------------------------------------------------------------- GPU
def _gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.fixture(scope="module")
def rbac():
    w = synth.rbac(users=30000, groups=2000, docs=80000, tuples=300000, checks=20000, seed=21)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    roots, targets = w.resolve(snap)
    want = randgraph.oracle_store_columns(w.namespaces, w.columns).check_batch(
        w.requests(range(len(roots))), nthreads=8)
    # every byte of an id is exercised, NONE on both sides
    assert (roots == NONE).any() and (targets == NONE).any()
    assert ((roots >= 65536) & (roots != NONE)).any() and (roots < 65536).any()
    assert ((targets >= 65536) & (targets != NONE)).any()
    assert snap.stats()["num_nodes"] < 2 ** 17 and snap.packed24_ok()
    roots.setflags(write=False)
    targets.setflags(write=False)
    return snap, roots, targets, np.asarray(want, dtype=bool)


class Packed:
    """a packed24 batch in a pinned buffer (read in place by the device) or a pageable one"""

    def __init__(self, nmax, pinned):
        self.buf = check.PinnedBuffer(check.packed24_bytes(nmax), np.uint8) if pinned else None
        self.array = self.buf.array if pinned else np.zeros(check.packed24_bytes(nmax) // 8 + 1,
                                                            dtype=np.uint64).view(np.uint8)
        assert self.array.ctypes.data % 8 == 0

    def fill(self, roots, targets):
        p = check.pack24(roots, targets)
        self.array[:len(p)] = p  # (bytes past it keep the previous, larger batch)
        return self.array.ctypes.data


SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _words(call, n):
    """result and flag words of one raw call, with a sentinel word after each"""
    words = (n + 63) // 64
    ab = np.full(words + 1, SENTINEL, dtype=np.uint64)
    fb = np.full(words + 1, SENTINEL, dtype=np.uint64)
    call(n, ab.ctypes.data, fb.ctypes.data)
    assert ab[words] == SENTINEL and fb[words] == SENTINEL
    return ab[:words], fb[:words]


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("mode", ["direct", "chunks"])
@pytest.mark.parametrize("plan", ["label", "lite", "bidi", "core"])
def test_packed_matches_oracle_and_u32_call(rbac, plan, mode, pinned, monkeypatch):
    """one engine, batch sizes around the unit (16), the workgroup (64) and the 8-byte tail,
    smaller batches after a larger one: oracle answers, the u32 call's result and flag words,
    and the path the requests took"""
    _gpu()
    snap, roots, targets, want = rbac
    monkeypatch.setenv("KETOGPU_UNITS", plan)
    monkeypatch.setenv("KETOGPU_PIPE_MODE", mode)
    eng = check.Engine(snap)
    N = len(roots)
    pk = Packed(N, pinned)
    u32 = [check.pinned(roots), check.pinned(targets)] if pinned else None
    for n in (N, 0, 1, 15, 16, 17, 63, 64, 65, 777, N):
        ptr = pk.fill(roots[:n], targets[:n])
        ab, fb = _words(lambda m, a, f: eng.check_ids_packed_raw(ptr, m, a, f), n)
        in_place = plan == "label" and mode == "direct" and pinned and n > 0  # (n = 0: nothing is read)
        assert eng.last_request_path() == (2 if in_place else 1), n
        np.testing.assert_array_equal(check.unpack_bits(ab.copy(), n), want[:n])
        rp, tp = ((u32[0].array.ctypes.data, u32[1].array.ctypes.data) if pinned else
                  (roots.ctypes.data, targets.ctypes.data))
        ab32, fb32 = _words(lambda m, a, f: eng.check_ids_raw(rp, tp, m, a, f), n)
        assert eng.last_request_path() == 0
        np.testing.assert_array_equal(ab, ab32)
        np.testing.assert_array_equal(fb, fb32)
    # the array form
    got, flags = eng.check_ids_packed(check.pack24(roots, targets), N, with_flags=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(flags, check.unpack_bits(fb32.copy(), N))


@pytest.mark.gpu
@pytest.mark.parametrize("heads,permille,stat", [("8,8", 0, "full_requests"), ("8,16", 250, "rest_requests")])
def test_later_label_stages_read_the_fused_kernels_ids(heads, permille, stat, monkeypatch):
    """plan label's dense pass and second stage read the u32 ids from HBM, and with a pinned
    packed buffer only label_host_packed_kernel writes them: short heads send requests to the
    dense pass, unlabelled heads to the second stage"""
    _gpu()
    monkeypatch.setenv("KETOGPU_UNITS", "label")
    monkeypatch.setenv("KETOGPU_LABEL_HEADS", heads)
    monkeypatch.setenv("KETOGPU_LABEL_REST_PERMILLE", str(permille))
    namespaces, rows, reqs = randgraph.make_family_graph(92)
    snap = Snapshot.from_rows(namespaces, rows, sort=True)
    want = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(x)) for ns, o, r, x in reqs])
    n = len(roots)
    pk = Packed(n, True)
    ptr = pk.fill(roots, targets)
    eng = check.Engine(snap)
    for _ in range(2):
        ab, _ = _words(lambda m, a, f: eng.check_ids_packed_raw(ptr, m, a, f), n)
        np.testing.assert_array_equal(check.unpack_bits(ab.copy(), n), want)
        assert eng.last_request_path() == 2
        st = eng.last_stats()
        assert st["plan"] == 7 and st[stat] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("plan,pinned", [("label", True), ("bidi", False)], ids=["in-place", "unpacked"])
def test_packed_call_rejects_ids_outside_the_snapshot(rbac, plan, pinned, monkeypatch):
    """both paths validate as the u32 call does and name the first bad request; an id with
    any of bits 17..23 set is outside this snapshot (a decode that dropped high bits would
    accept it); a misaligned buffer is refused; the engine stays exact afterwards"""
    _gpu()
    snap, roots, targets, want = rbac
    monkeypatch.setenv("KETOGPU_UNITS", plan)
    eng = check.Engine(snap)
    st = snap.stats()
    N = len(roots)
    pk = Packed(N, pinned)

    def rejected(r, t, at):
        ptr = pk.fill(r, t)
        with pytest.raises(L.KetoError) as e:
            _words(lambda m, a, f: eng.check_ids_packed_raw(ptr, m, a, f), N)
        assert e.value.code == L.EINVAL and f"request {at} " in str(e.value), str(e.value)
        assert eng.last_request_path() == (2 if pinned else 1)

    for bad_at, which in ((0, "root"), (5000, "target"), (N - 1, "root")):
        r, t = roots.copy(), targets.copy()
        if which == "root":
            r[bad_at] = st["num_expandable"]  # not an expandable node
        else:
            t[bad_at] = st["num_nodes"] + 7
        rejected(r, t, bad_at)
    good_r = int(roots[roots != NONE][0])
    good_t = int(targets[targets != NONE][0])
    for bit in range(17, 24):
        r, t = roots.copy(), targets.copy()
        r[33], t[33] = good_r | 1 << bit, good_t
        rejected(r, t, 33)
        r[33], t[33] = good_r, good_t | 1 << bit
        rejected(r, t, 33)
    ptr = pk.fill(roots, targets)
    with pytest.raises(L.KetoError) as e:
        _words(lambda m, a, f: eng.check_ids_packed_raw(ptr + 2, m, a, f), N - 1)
    assert e.value.code == L.EINVAL and "aligned" in str(e.value)
    # still exact, packed and u32
    for _ in range(2):
        ab, _ = _words(lambda m, a, f: eng.check_ids_packed_raw(ptr, m, a, f), N)
        np.testing.assert_array_equal(check.unpack_bits(ab.copy(), N), want)
    np.testing.assert_array_equal(eng.check_ids(roots, targets), want)


@pytest.mark.gpu
def test_packed_subrange_pointers_engine_and_multi(rbac):
    """a packed pointer 40 bytes into a ketogpu_host_alloc buffer and result words at an
    offset, through Engine and through MultiEngine over every device (each range begins at a
    multiple of 64 requests, 384 bytes, and reads through its own device's view)"""
    _gpu()
    snap, roots, targets, want = rbac
    n = len(roots)
    off = 8 * 5
    p = check.pack24(roots, targets)
    buf = check.PinnedBuffer(off + len(p) + 8, np.uint8)
    buf.array[:] = 0xEE
    buf.array[off:off + len(p)] = p
    words = (n + 63) // 64
    out = check.PinnedBuffer(words + 3, np.uint64)
    ndev = L.lib().ketogpu_device_count()
    for eng in (check.Engine(snap), check.MultiEngine(snap, list(range(ndev)))):
        for _ in range(3):  # a fresh registry view on the first call, cached after
            out.array[:] = 0
            eng.check_ids_packed_raw(buf.p.value + off, n, out.p.value + 8 * 3)
            np.testing.assert_array_equal(check.unpack_bits(out.array[3:3 + words].copy(), n), want)
            assert not out.array[:3].any()
    multi = check.MultiEngine(snap, list(range(ndev)))
    got, flags = multi.check_ids_packed(p, n, with_flags=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(flags, multi.check_ids(roots, targets, with_flags=True)[1])
