"""The listing handles on WRITABLE snapshots, no writes: the boundary shapes of the read-only
suites (wide chunks, the LDS set, pages, depth, via, the wide expand graph) laid out as a serving
process has them: forward rows in the arena with an `end` array and free words behind every row,
reverse rows padded with placeholder ids, reserved ids behind N, three placeholder nodes.

Yardsticks and fixtures: tests/writable_cases.py, whose sizes test_writable_layout_host.py proves
on the CPU.  Answers are asserted, and that the wide tier / tier 2 / the copy queue was used at
all; routing counts are not, where the placeholders change them."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import expand, lookup
from tests import expand_cases as EC
from tests import expand_wide_cases as WC
from tests import test_list_refresh_gpu as RG
from tests import wide_gpu_suite as W
from tests import wide_page_gpu_suite as WP
from tests import writable_cases as WR

pytestmark = pytest.mark.gpu
ANY, NONE_F, ALL = WR.ANY, WR.NONE_F, WR.ALL
SIDES = ("subjects", "lookup")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    W.need_gpu()


@pytest.fixture(params=["default", "tier2"])
def tiers(request, monkeypatch):
    return WR.set_tiers(monkeypatch, request.param)


def same_cursor(got, want, what):
    """one cursor call (out, begin, count, needed) against the host twin's: the same markers,
    counts and total, every written list the same set of ids, segments apart"""
    (out, begin, count, needed), (wout, wbegin, wcount, wneeded) = got, want
    assert needed == wneeded and np.array_equal(count, wcount), what
    marks = (lookup.INVALID, lookup.TRUNCATED)
    assert np.array_equal(begin == lookup.INVALID, wbegin == lookup.INVALID), what
    for b, wb, c in zip(begin, wbegin, count):  # (an empty list is never cut off, wherever the twin's cursor stands)
        assert not c or (b == lookup.TRUNCATED) == (wb == lookup.TRUNCATED), what
    used = np.zeros(len(out) + 1, dtype=np.int32)
    for b, c, wb in zip(begin, count, wbegin):
        if b in marks or not c:
            continue
        b, c, wb = int(b), int(c), int(wb)
        assert np.array_equal(np.sort(out[b:b + c]), np.sort(wout[wb:wb + c])), what
        used[b:b + c] += 1
    assert (used <= 1).all(), what


# ---------------------------------------------------------------------- chunks and the LDS set
@pytest.mark.parametrize("which", ["chunk", "set"])
@pytest.mark.parametrize("side", SIDES)
def test_chunk_and_set_boundaries(side, which, monkeypatch):
    """stars and split stars of C-1, C, C+1, 2C+1 entries under forced routing, and of
    set_capacity -1, +0, +1 under the default one: every start alone and all in one call, three
    filters, plain and wide, count-only and with exactly the capacity needed"""
    S = W.SIDES[side]
    if which == "chunk":
        S.force(monkeypatch)
    t, starts = WR.boundary_twin(side, which)
    rw = t.rw
    every = np.array(list(starts.values()), dtype=np.uint32)
    with S.handle(rw) as h:
        assert h.wide_stats()["chunk"] == WR.CHUNK and h.stats()["set_capacity"] == WR.SET_CAP
        for f in (ANY, S.view_filter(rw), NONE_F):
            lists = dict(zip(every.tolist(), S.host(rw, every, f)))
            for ids in [every[i:i + 1] for i in range(len(every))] + [every]:
                want = [lists[int(x)] for x in ids]
                total = sum(len(w) for w in want)
                for wide in (False, True):
                    W.assert_call_matches(S, h, ids, f, want, wide=wide)
                    out, begin, count, needed = S.raw(h, ids, f, 0, wide=wide)
                    assert needed == total and [int(c) for c in count] == [len(w) for w in want]
                    assert all(b == lookup.TRUNCATED for b, w in zip(begin, want) if len(w))
            if f == NONE_F:
                assert not any(len(w) for w in lists.values())
        for name, x in starts.items():
            assert len(S.host(rw, [x])[0]) == int(name.lstrip("starsplit"))
        # the read-only snapshot of the same rows lists the same nodes, by name
        to = t.map(every)
        for got, y in zip(S.lists(h, every), to):
            assert np.array_equal(WR.mapped(t, got), S.host(t.ro, [int(y)])[0])
        ws = h.wide_stats()
        assert ws["wide_requests"] > 0 and ws["items"] > 0
        if which == "set":
            assert ws["tier1_requests"] > 0  # both tiers answered


# ---------------------------------------------------------------------- pages
@pytest.mark.parametrize("side", SIDES)
def test_pages_of_the_largest_star(side, tiers):
    """plain and wide pages of the star of 2C+1: limits 1, 50 and 4096; `from` at 0, the first
    and last member, one past it, n_cap - 1, a reserved id and a placeholder; after every wide
    page call a plain full-list call finds the bitmaps clean"""
    S = WP.SIDES[side]
    t, starts = WR.boundary_twin(side, "chunk")
    rw = t.rw
    r = np.array([starts[f"star{2 * WR.CHUNK + 1}"]], dtype=np.uint32)
    ms = S.host(rw, r)
    n = rw.stats()["num_nodes"]
    froms = [0, int(ms[0][0]), int(ms[0][-1]), int(ms[0][-1]) + 1, t.n_cap - 1, n, n + 5, t.placeholders()[-1]]
    assert n + 5 < t.n_cap - 1
    hh = S.host_twin(rw)
    with S.handle(rw) as h:
        for limit in (1, 50, 4096):
            for lo in froms:
                lo = np.array([lo], dtype=np.uint32)
                what = (side, limit, int(lo[0]))
                got = WP.check_page(S, h, rw, r, None, lo, ANY, limit, what)  # wide, against the twin and the plain call
                W.assert_call_matches(S.side, h, r, ANY, ms, wide=False)    # ... which left the bitmaps clean
                want = getattr(hh, S._plain_page)(r, lo, ANY, limit)
                RG.same_pages(S.plain_page(h, r, lo, ANY, limit, wide=False), want, what)
                RG.same_pages(S.plain_page(h, r, lo, ANY, limit, wide=True), want, what)
                W.assert_call_matches(S.side, h, r, ANY, ms, wide=False)    # ... and so did this wide page call
                assert got[2][0] == 2 * WR.CHUNK + 1
                if lo[0] > ms[0][-1]:
                    assert got[1][0] == 0 and got[3][0] == 0
        assert h.wide_stats()["wide_requests"] > 0


# ---------------------------------------------------------------------- depth and via
@pytest.mark.parametrize("side", SIDES)
def test_depth_and_via(side, tiers):
    """the writable chains, the joined chain and the split star at depth 1, 2 and ALL, plain and
    wide; via with the "one hop nearer" rule"""
    S = WP.SIDES[side]
    t, starts = WR.depth_twin(side)
    rw, ro = t.rw, t.ro
    hh = S.host_twin(rw)
    kind = "subject" if side == "subjects" else "lookup"
    host_depth = lookup.host_subjects_depth if side == "subjects" else lookup.host_lookup_depth
    host_via = lookup.host_subjects_via if side == "subjects" else lookup.host_lookup_via
    to = t.map(starts)
    with S.handle(rw) as h:
        for k in (1, 2, ALL):
            depth = np.full(len(starts), k, dtype=np.uint32)
            want = WP.check_lists(S, h, rw, starts, depth, ANY, (side, k))  # wide and plain, lists and frontier
            WP.check_page(S, h, rw, starts, depth, WP.mid_from(want, rw.stats()["num_nodes"]), ANY, 50, (side, k))
            for w, y in zip(want, to):
                assert np.array_equal(WR.mapped(t, w), host_depth(ro, int(y), k)[0]), (side, k)
            got, exp = getattr(h, f"{kind}_via")(starts, k), getattr(hh, f"{kind}_via")(starts, k)
            RG.same_via(got, exp, starts.tolist(), (side, k, "via"))
            for (ids, _, hops), y in zip(got[0], to):
                wi, _, wh, _ = host_via(ro, int(y), k)
                order = np.argsort(t.map(ids), kind="stable")
                assert np.array_equal(t.map(ids)[order], wi) and np.array_equal(hops[order], wh), (side, k, "hops")
        assert h.wide_stats()["wide_requests"] > 0  # the split star of C + 1 under either routing


# ---------------------------------------------------------------------- expand
def test_wide_expand_over_the_arena(tiers):
    """the writable wide-expand graph, wildcard and poison parts included: every root at depths
    2, 3 and ALL against the twin on the writable snapshot, word for word, and at ALL against the
    read-only snapshot's trees through the id map"""
    t = WR.wide_expand_twin()
    rw = t.rw
    ex, ex_ro = expand.Engine(rw), expand.Engine(t.ro)
    roots = WC.roots(rw)
    bad = list(WC.root_names()).index("wbad")
    with expand.DeviceEngine(rw) as dev:
        for d in (2, 3, WC.ALL):
            status = WC.assert_device_wide(dev, ex, roots, d)
            assert status[bad] == L.EXPAND_HOST and (np.delete(status, bad) == L.EXPAND_OK).all()
        trees, status = dev.expand_ids(roots, WC.ALL, wide=True)
        for x, y, (nodes, kids), st in zip(roots, t.map(roots), trees, status):
            wst, wnodes, wkids, _ = EC.twin(ex_ro, y, WC.ALL)
            assert st == wst and np.array_equal(t.map(nodes), wnodes) and np.array_equal(kids, wkids), int(x)
        st = dev.expand_wide_stats()
        assert st["mask_builds"] == 1 and st["mask_words"] > 0
        if tiers == "default":
            assert st["runs_queued"] > 0 and st["items_queued"] > 0 and st["tier1_requests"] > 0
        else:
            assert st["tier2_requests"] > 0 and st["tier2_rounds"] > 0


def test_wide_expand_with_a_queue_of_one(monkeypatch):
    monkeypatch.setenv("KETOGPU_EXPAND_WIDE_QUEUE", "1")
    WR.set_tiers(monkeypatch, "default")
    t = WR.wide_expand_twin()
    ex = expand.Engine(t.rw)
    with expand.DeviceEngine(t.rw) as dev:
        assert dev.expand_wide_stats()["queue_capacity"] == 1
        for d in (3, WC.ALL):
            WC.assert_device_wide(dev, ex, WC.roots(t.rw), d)
        st = dev.expand_wide_stats()
        assert st["runs_queue_full"] > 0 and st["runs_self_copied"] >= st["runs_queue_full"] and st["mask_builds"] == 1


# ---------------------------------------------------------------------- ids that are not nodes
def test_ids_that_are_no_nodes(tiers):
    """a start at each placeholder, at N, n_cap - 1 and n_cap, between two real starts, in every
    kind of call: what the host twin on the writable snapshot answers (an empty list, or INVALID),
    and the real starts' answers undisturbed"""
    for side in SIDES:
        S = WP.SIDES[side]
        t, starts = WR.depth_twin(side)
        rw = t.rw
        kind = "subject" if side == "subjects" else "lookup"
        ids = np.concatenate([starts[:1], WR.non_nodes(t), starts[1:]]).astype(np.uint32)
        second = np.full(len(ids), starts[3], dtype=np.uint32)
        hh = S.host_twin(rw)
        g, w = (lambda name: getattr(h, f"{kind}_{name}")), (lambda name: getattr(hh, f"{kind}_{name}"))
        with S.handle(rw) as h:
            for wide in (False, True):
                cap = w("ids_raw")(ids, ANY, 0)[3]
                same_cursor(g("ids_raw")(ids, ANY, cap, wide=wide), w("ids_raw")(ids, ANY, cap), (side, "ids", wide))
                same_cursor(g("ids_raw")(ids, ANY, 0, wide=wide), w("ids_raw")(ids, ANY, 0), (side, "count", wide))
                WR.same_pages(g("page_raw")(ids, None, ANY, 50, wide=wide), w("page_raw")(ids, None, ANY, 50),
                              (side, "page", wide))
            for k in (1, ALL):
                depth = np.full(len(ids), k, dtype=np.uint32)
                want = WP.check_lists(S, h, rw, ids, depth, ANY, (side, "depth", k))
                assert [m is None for m in want] == [int(x) >= rw.stats()["num_nodes"] for x in ids]
                WP.check_page(S, h, rw, ids, depth, None, ANY, 50, (side, "depth page", k))
            cap = w("via_raw")(ids, None, ANY, 0)[6]
            got, exp = g("via_raw")(ids, None, ANY, cap), w("via_raw")(ids, None, ANY, cap)
            same_cursor((got[0], got[3], got[4], got[6]), (exp[0], exp[3], exp[4], exp[6]), (side, "via"))
            assert np.array_equal(got[5], exp[5])
            host_via = lookup.host_subjects_via if side == "subjects" else lookup.host_lookup_via
            full = [None if int(x) >= rw.stats()["num_nodes"] else host_via(rw, int(x)) for x in ids]
            WR.same_via_page(g("via_page_raw")(ids, None, None, ANY, 50), w("via_page_raw")(ids, None, None, ANY, 50),
                             full, ids.tolist(), (side, "via page"))
            for op in ("and", "andnot", "or"):
                for a, b in ((ids, second), (second, ids)):
                    cap = hh.combine_ids_raw(a, b, op, ANY, 0)[3]
                    same_cursor(h.combine_ids_raw(a, b, op, ANY, cap), hh.combine_ids_raw(a, b, op, ANY, cap),
                                (side, op))
                    WR.same_pages(h.combine_page_raw(a, b, op, None, ANY, 50), hh.combine_page_raw(a, b, op, None, ANY, 50),
                                  (side, op, "page"))
            if side == "lookup":
                roots = np.resize(np.array(h.lookup_ids(starts[:1])[0][:1], dtype=np.uint32), len(ids))
                for a, b in ((roots, ids), (ids, np.resize(starts[:1], len(ids)))):
                    got, exp = h.path_ids_raw(a, b, 64), hh.path_ids_raw(a, b, 64)
                    assert got[3] == exp[3] and np.array_equal(got[2], exp[2]), "path"  # lengths: any shortest path
                    assert np.array_equal(got[1] == lookup.INVALID, exp[1] == lookup.INVALID)
            else:
                ex = expand.Engine(rw)
                with expand.DeviceEngine(rw, subjects=h) as dev:
                    for d in (2, WC.ALL):
                        EC.assert_device(dev, ex, ids, d)
                        WC.assert_device_wide(dev, ex, ids, d)
