"""Fixtures and the yardstick of the tests that look at the listing handles on WRITABLE snapshots
(test_writable_layout_host.py on the CPU; test_writable_layout_gpu.py, test_writable_moves_gpu.py
and test_list_fallbacks_gpu.py on the device).

A writable snapshot lays its rows out differently from the read-only snapshots every boundary
suite builds: the subjects handle keeps forward rows in an arena (row v is col[off[v] .. end[v]),
room for len + len / 4 + 4 entries, free words behind it, rows that outgrow their room at the
arena's tail), the lookup handle's reverse rows are padded with placeholder ids and ids
[N, n_cap) are reserved rows of four placeholders, and three placeholder nodes shift every id.

Two yardsticks.  The first is the host twin on the READ-ONLY snapshot of the same rows, which
test_subjects_host.py, test_lookup_host.py and test_expand_*_host.py pin against the oracle: a
list from the writable snapshot, mapped through `to_ro` and compared as a set, equals the
read-only one; so do the lists per depth, the hop counts, combined lists and expand trees (node
arrays mapped, child counts equal).  The frontier of a depth call is NOT compared this way: it
counts interior members, and a writable snapshot treats every expandable node as interior
(depth_cases.Truth), so it is compared with the second yardstick only.  The second is the host
twin on the writable snapshot itself, word for word: pages, `from` bounds, `remaining`, tree
preorder, path lengths, frontiers.

The id map is order-preserving on real nodes for a snapshot without writes
(test_writable_layout_host.py asserts it).  After a write that names a new subject it is not:
the new node takes a reserved id behind every older one, whatever its name.  So paged answers are
compared with the writable twin alone, everywhere.

Rows are raw rows as in lookup_cases (NS1)."""
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import expand, lookup
from keto_amd.snapshot import Snapshot
from tests import depth_cases as DC
from tests import expand_cases as EC
from tests import expand_wide_cases as WC
from tests import lookup_cases as LC
from tests import refresh_cases as RC
from tests import test_list_refresh_gpu as RG  # (its helpers: importing it runs nothing)
from tests import wide_gpu_suite as W
from tests import wide_page_gpu_suite as WP

ANY, IDS, NONE_F = lookup.TYPE_ANY, lookup.CLASS_SUBJECT_ID, lookup.TYPE_NONE
ALL = lookup.DEPTH_ALL
INVALID = np.uint32(L.NODE_NONE)
CHUNK = 2048     # wide.hpp kChunk, wide_stats()["chunk"]: the GPU tests assert it
SET_CAP = 1024   # closure.hpp kSetCap, stats()["set_capacity"]: likewise
CHUNK_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SET_SIZES = (SET_CAP - 1, SET_CAP, SET_CAP + 1)


# ---------------------------------------------------------------------- twins and the id map
def is_placeholder(snap, v):
    return snap.subject_class(int(v)) == L.TYPE_NONE


class Twin:
    """a writable snapshot `rw`, the mirror of its row table, and the read-only snapshot `ro` of
    the same rows with the id map, rebuilt after every applied write"""

    def __init__(self, rows, namespaces=LC.NS1):
        self.namespaces, self.rows = namespaces, set(rows)
        self.rw = Snapshot.from_rows(namespaces, list(self.rows), writable=True)  # (from_rows sorts)
        self.n0 = self.rw.stats()["num_nodes"]
        self.n_cap = self.n0 + max(1024, self.n0 // 8)  # snapshot_write.cpp make_writable
        self._ro, self._map, self._holes, self._names = None, {}, None, {}

    def write(self, ins=(), dele=()):
        """an in-place write, mirrored in the row table when the snapshot took it -> its result"""
        ins, dele = list(ins), list(dele)
        res = self.rw.write(ins, dele)
        if res["applied"]:
            self.rows |= set(ins)
            self.rows -= set(dele)
            self._ro, self._map = None, {}
        return res

    @property
    def ro(self):
        if self._ro is None:
            self._ro = Snapshot.from_rows(self.namespaces, list(self.rows))
        return self._ro

    def map(self, ids):
        """rw ids -> ro ids, by name: one describe() per id ever asked for (a node keeps its id and
        its name), one resolve per id not seen since the last write; placeholders, reserved ids and
        ids outside the snapshot -> INVALID"""
        ids = np.asarray(ids, dtype=np.uint32)
        n = self.rw.stats()["num_nodes"]
        new = [int(v) for v in np.unique(ids) if int(v) not in self._map]
        real = [v for v in new if v < n and not is_placeholder(self.rw, v)]
        for v in new:
            self._map[v] = INVALID
        if real:
            for v in real:
                if v not in self._names:
                    self._names[v] = self.rw.describe(v)
            to = lookup.resolve_subjects(self.ro, [self._names[v] for v in real])
            self._map.update(zip(real, to))
        return np.array([self._map[int(v)] for v in ids], dtype=np.uint32)

    @property
    def to_ro(self):
        """the whole map: uint32[num_nodes of rw]"""
        return self.map(np.arange(self.rw.stats()["num_nodes"], dtype=np.uint32))

    def placeholders(self):
        """the placeholder nodes: expandable ids, which no write moves"""
        if self._holes is None:
            self._holes = [v for v in range(self.rw.stats()["num_expandable"]) if is_placeholder(self.rw, v)]
        return list(self._holes)


def twin(rows, namespaces=LC.NS1):
    """-> (rw, ro, to_ro) of one row set"""
    t = Twin(rows, namespaces)
    return t.rw, t.ro, t.to_ro


def mapped(t, ids):
    """a device or host list of rw as the sorted ro ids it stands for: every id is a real node"""
    m = t.map(ids)
    assert not (m == INVALID).any(), "a list names a placeholder or a reserved id"
    return np.sort(m)


def non_nodes(t):
    """ids that are no node of rw: every placeholder, N, n_cap - 1, n_cap (N as it stands now)"""
    n = t.rw.stats()["num_nodes"]
    return np.array(t.placeholders() + [n, t.n_cap - 1, t.n_cap], dtype=np.uint32)


# ---------------------------------------------------------------------- the ro yardstick, host only
def host_equal(t, roots, targets, depths=(1, 2, ALL)):
    """the rw host lists equal the ro ones through the map, per depth and hop count, for these
    expandable starts (subjects) and these nodes (lookup) -> the number of lists compared"""
    rw, ro, n = t.rw, t.ro, 0
    for side, ids, full, depth, via in (
            ("subjects", roots, lookup.host_subjects, lookup.host_subjects_depth, lookup.host_subjects_via),
            ("lookup", targets, lookup.host_lookup, lookup.host_lookup_depth, lookup.host_lookup_via)):
        ids = np.asarray(ids, dtype=np.uint32)
        to = t.map(ids)
        for x, y in zip(ids, to):
            if y == INVALID:  # a placeholder: nothing reaches it and it reaches nothing
                assert not len(full(rw, int(x))), (side, int(x))
                continue
            assert np.array_equal(mapped(t, full(rw, int(x))), full(ro, int(y))), (side, int(x))
            for k in depths:
                assert np.array_equal(mapped(t, depth(rw, int(x), k)[0]), depth(ro, int(y), k)[0]), (side, int(x), k)
            gi, _, gh, _ = via(rw, int(x))
            wi, _, wh, _ = via(ro, int(y))
            order = np.argsort(t.map(gi), kind="stable")
            assert np.array_equal(t.map(gi)[order], wi) and np.array_equal(gh[order], wh), (side, int(x), "hops")
            n += 1
    return n


def trees_equal(t, roots, depths=(2, 3, EC.ALL)):
    """EC.twin of rw equals EC.twin of ro: status and child counts equal, node arrays mapped"""
    ex_rw, ex_ro = expand.Engine(t.rw), expand.Engine(t.ro)
    to = t.map(roots)
    for x, y in zip(np.asarray(roots, dtype=np.uint32), to):
        if y == INVALID:
            continue
        for d in depths:
            st, nodes, kids, inv = EC.twin(ex_rw, x, d)
            wst, wnodes, wkids, winv = EC.twin(ex_ro, y, d)
            assert (st, inv) == (wst, winv), (int(x), d)
            assert np.array_equal(t.map(nodes), wnodes) and np.array_equal(kids, wkids), (int(x), d)


# ---------------------------------------------------------------------- the call matrix
def same_pages(got, want, what):
    """test_list_refresh_gpu.same_pages for calls with ids outside the snapshot: a row marked
    PAGE_INVALID holds nothing to compare"""
    out, ret, cnt, rem = got[:4]
    wout, wret, wcnt, wrem = want[:4]
    assert np.array_equal(ret, wret) and np.array_equal(cnt, wcnt) and np.array_equal(rem, wrem), what
    for i, r in enumerate(ret):
        if r != lookup.PAGE_INVALID:
            assert np.array_equal(out[i][:int(r)], wout[i][:int(r)]), (what, i)


def same_via_page(got, want, full, starts, what):
    """one *_via_page_raw answer against the host's: ids, hops and the counters equal; every via
    is the start or a member of the whole list one hop nearer (test_list_refresh_gpu.same_via)"""
    out, via, hops, ret, cnt, rem, fr = got
    wout, _, whops, wret, wcnt, wrem, wfr = want
    assert np.array_equal(ret, wret) and np.array_equal(cnt, wcnt) and np.array_equal(rem, wrem), what
    assert np.array_equal(fr, wfr), what
    for i, r in enumerate(ret):
        if r == lookup.PAGE_INVALID:
            continue
        r = int(r)
        assert np.array_equal(out[i, :r], wout[i, :r]) and np.array_equal(hops[i, :r], whops[i, :r]), (what, i)
        level = dict(zip(full[i][0].tolist(), full[i][2].tolist()))
        for v, h in zip(via[i, :r].tolist(), hops[i, :r].tolist()):
            assert (h == 1 and v == starts[i]) or level[v] == h - 1, (what, i)


def _side_calls(snap, h, hh, kind, ids, second, what, t):
    """what check_every_call lacks, for one handle `h` against its host twin `hh` on rw; with a
    Twin `t`, the device's lists against the read-only snapshot too"""
    g = lambda name: getattr(h, f"{kind}_{name}")
    w = lambda name: getattr(hh, f"{kind}_{name}")
    host_full = lookup.host_subjects if kind == "subject" else lookup.host_lookup
    ids = np.asarray(ids, dtype=np.uint32)
    want = [host_full(snap, int(x)) for x in ids]
    RG.same(g("ids")(ids, ANY, wide=True), want, f"{what}: {kind} wide ids")
    for wide in (False, True):
        RG.same_pages(g("page_raw")(ids, None, ANY, 50, wide=wide), w("page_raw")(ids, None, ANY, 50),
                      f"{what}: {kind} page wide={wide}")
        for k in (1, 2):
            got, exp = g("depth")(ids, k, wide=wide), w("depth")(ids, k)
            RG.same(got[0], exp[0], f"{what}: {kind} depth {k} wide={wide}")
            assert np.array_equal(got[1], exp[1]), f"{what}: {kind} frontier {k} wide={wide}"
            lo = WP.mid_from(exp[0], snap.stats()["num_nodes"])
            WP.assert_page_equal(g("depth_page_raw")(ids, k, lo, ANY, 50, wide=wide),
                                 w("depth_page_raw")(ids, k, lo, ANY, 50), f"{what}: {kind} depth page {k} wide={wide}")
    full = [(lookup.host_subjects_via if kind == "subject" else lookup.host_lookup_via)(snap, int(x)) for x in ids]
    same_via_page(g("via_page_raw")(ids, None, None, ANY, 50), w("via_page_raw")(ids, None, None, ANY, 50), full,
                  ids.tolist(), f"{what}: {kind} via page")
    b = np.full(len(ids), second, dtype=np.uint32)
    for op in ("andnot", "or"):
        RG.same(h.combine_ids(ids, b, op), hh.combine_ids(ids, b, op), f"{what}: {kind} {op}")
    RG.same_pages(h.combine_page_raw(ids, b, "or", None, ANY, 50), hh.combine_page_raw(ids, b, "or", None, ANY, 50),
                  f"{what}: {kind} or page")
    if t is None:
        return
    # the first yardstick: the device's lists, mapped, are the read-only snapshot's
    ro = t.ro
    to, to_b = t.map(ids), t.map([second])[0]
    host_depth = lookup.host_subjects_depth if kind == "subject" else lookup.host_lookup_depth
    host_via = lookup.host_subjects_via if kind == "subject" else lookup.host_lookup_via
    hro = (lookup.HostSubjects if kind == "subject" else lookup.HostLookup)(ro)
    real = [i for i, y in enumerate(to) if y != INVALID]
    sub, sto = ids[real], to[real]
    for got, y in zip(g("ids")(sub, ANY, wide=True), sto):
        assert np.array_equal(mapped(t, got), host_full(ro, int(y))), f"{what}: {kind} wide ids, read-only"
    for got, y in zip(g("depth")(sub, 2, wide=True)[0], sto):
        assert np.array_equal(mapped(t, got), host_depth(ro, int(y), 2)[0]), f"{what}: {kind} depth 2, read-only"
    for (gi, _, gh), y in zip(g("via")(sub)[0], sto):
        wi, _, wh, _ = host_via(ro, int(y))
        order = np.argsort(t.map(gi), kind="stable")
        assert np.array_equal(t.map(gi)[order], wi) and np.array_equal(gh[order], wh), f"{what}: {kind} hops, read-only"
    if to_b != INVALID and len(sub):
        for op in ("and", "andnot"):
            got = h.combine_ids(sub, b[real], op)
            exp = hro.combine_ids(sto, np.full(len(sto), to_b, dtype=np.uint32), op)
            for a, e in zip(got, exp):
                assert np.array_equal(mapped(t, a), e), f"{what}: {kind} {op}, read-only"


def all_calls(snap, lk, sj, dev, roots, second, targets, path_roots, what, xroots=None, t=None):
    """test_list_refresh_gpu.check_every_call (plain, paged, depth, via, `and`, path) plus the
    wide full lists, wide pages, wide depth lists, depth pages plain and wide, via pages, `andnot`
    and `or`, combined pages, and the expand calls plain and wide through `dev`
    (expand.DeviceEngine over sj), every one against its host twin on the writable snapshot; with
    a Twin `t` (t.rw is snap) also against the read-only snapshot of the same rows"""
    RG.check_every_call(snap, lk, sj, roots, second, targets, path_roots, what)
    _side_calls(snap, sj, lookup.HostSubjects(snap), "subject", roots, second, what, t)
    _side_calls(snap, lk, lookup.HostLookup(snap), "lookup", targets, targets[0], what, t)
    if dev is None:
        return
    xroots = np.asarray(roots if xroots is None else xroots, dtype=np.uint32)
    ex = expand.Engine(snap)
    for d in (2, EC.ALL):
        EC.assert_device(dev, ex, xroots, d)
        WC.assert_device_wide(dev, ex, xroots, d)
    if t is not None:
        trees, status = dev.expand_ids(xroots, EC.ALL, wide=True)
        ex_ro = expand.Engine(t.ro)
        for x, y, (nodes, kids), st in zip(xroots, t.map(xroots), trees, status):
            if y == INVALID:
                continue
            wst, wnodes, wkids, _ = EC.twin(ex_ro, y, EC.ALL)
            assert st == wst and np.array_equal(t.map(nodes), wnodes) and np.array_equal(kids, wkids), \
                f"{what}: expand {int(x)}, read-only"


def set_tiers(monkeypatch, param):
    """the body of a `tiers` fixture: the default tiers, or every request through tier 2"""
    for knob in ("KETOGPU_LOOKUP_TIER", "KETOGPU_SUBJECTS_TIER"):
        if param == "tier2":
            monkeypatch.setenv(knob, "2")
        else:
            monkeypatch.delenv(knob, raising=False)
    return param


# ---------------------------------------------------------------------- fixtures of the layout tests
def boundary_rows(side, sizes):
    """wide_gpu_suite's chunk / set boundary graph of one side: a star and a split per size"""
    S = W.SIDES[side]
    rows = []
    for k in sizes:
        rows += S.star(f"star{k}", k, f"a{k}_") + S.split(f"split{k}", k, f"b{k}_")
    return rows


@functools.lru_cache(maxsize=None)
def boundary_twin(side, which):
    """-> (Twin, {name: start}) of the chunk ("chunk") or set ("set") boundary graph of one side"""
    S, sizes = W.SIDES[side], CHUNK_SIZES if which == "chunk" else SET_SIZES
    t = Twin(boundary_rows(side, sizes))
    return t, {f"{shape}{k}": S.start(t.rw, f"{shape}{k}") for shape in ("star", "split") for k in sizes}


def depth_rows(side):
    """depth_cases.writable_chains' two chains, a third chain hung under the first, and the split
    star of CHUNK + 1: a start with members at 1 and 2 hops, half of them reached twice"""
    s, ss = LC.sid, LC.sset
    rows = DC.writable_chain_rows()
    rows += [s("j0", "member", "uj"), ss("j1", "member", "j0", "member"), ss("j2", "member", "j1", "member"),
             ss("j0", "member", "a1", "member")]
    return rows + W.SIDES[side].split("dsplit", CHUNK + 1, "ds_")


@functools.lru_cache(maxsize=None)
def depth_twin(side):
    """-> (Twin, starts): a chain end, the joined chain's end, the split star"""
    S = W.SIDES[side]
    t = Twin(depth_rows(side))
    if side == "subjects":
        names = [("n", "b2", "member"), ("n", "j2", "member"), ("n", "spare", "member"), ("n", "dsplit", "view")]
        starts = lookup.resolve_roots(t.rw, names)
    else:
        starts = np.array([S.start(t.rw, u) for u in ("u1", "uj", "u0", "dsplit")], dtype=np.uint32)
    assert not (starts == INVALID).any()
    return t, starts


@functools.lru_cache(maxsize=None)
def wide_expand_twin():
    """the writable WC.wide_rows() graph, wildcard and poison parts included"""
    return Twin(WC.wide_rows())


# ---------------------------------------------------------------------- the graph of the moves tests
FILLER = 2000


def filler_rows(n=FILLER, groups=40):
    """n users spread over `groups` groups that one document names: rows that only add bytes to
    a full upload, so that the writes of a scenario stay under the backlog threshold"""
    rows = [LC.sid(f"fill_g{i % groups:02d}", "member", f"fill_u{i}") for i in range(n)]
    return rows + [LC.sset("fill_doc", "view", f"fill_g{g:02d}", "member") for g in range(groups)]


def moves_rows():
    """the chunk stars of both sides (the lookup side's with the prefix `l`), the wide-expand
    graph without its wildcard part (wgdup, wg_o: a snapshot with a wildcard node refuses every
    write) and without the poison part (wbad: likewise), a row of 300 with an opening child at 63
    whose names leave room before and behind it, and the filler"""
    rows = []
    for k in CHUNK_SIZES:
        rows += W.SUBJECTS.star(f"star{k}", k, f"a{k}_") + W.LOOKUP.star(f"lstar{k}", k, f"la{k}_")
    skip = ("wgdup", "wg_o", "wg_g", "wbad")
    rows += [r for r in WC.wide_rows() if not r[1].startswith(skip)]
    # a small user whose reverse row has exactly its two free slots (2 + 1 / 8)
    rows += [LC.sid("la2047_0", "view", "small")]
    return rows + filler_rows()


def new_sets(prefix, at, n):
    """n subject sets without rows whose names sort at `at` within the row of <prefix>r#view"""
    return [LC.sset(f"{prefix}r", "view", f"{prefix}{at}{i:04d}", "member") for i in range(n)]


def moves_script():
    """the moves series -> [(label, inserts, deletes, expect)]; expect: "applied" or a refusal's
    reason.  Every row it names exists, or is new, when its turn comes."""
    C = CHUNK
    star = f"star{C - 1}"
    grown = [LC.sid(star, "view", f"zz_new{i}") for i in range(602)]
    wl = new_sets("WL4095_", "x9", 1102)  # behind the last x0...: appended to the row
    wp = new_sets("WP63_", "x00062z", 80)  # between x00062 and x00063: the opening child moves by 80
    joins = [LC.sid(f"la{C}_{i}", "view", f"lstar{C - 1}") for i in range(2)]
    small = [LC.sid(f"la{C}_{i}", "view", "small") for i in range(3)]
    return [
        ("star C-1 +2: two chunks, in its room", grown[:2], [], "applied"),
        ("star C-1 +600: to the tail", grown[2:], [], "applied"),
        ("WL4095 +1: 4096", wl[:1], [], "applied"),
        ("WL4095 +1: 4097", wl[1:2], [], "applied"),
        ("WL4095 +1100: to the tail", wl[2:], [], "applied"),
        ("WP63 +80 before the opening child: to the tail", wp, [], "applied"),
        ("the opening child's own row +1", [LC.sid("WP63_x00063", "member", "WP63_u_more")], [], "applied"),
        ("the moved star loses what it gained", [], grown, "applied"),
        ("the moved star +1: fits its larger room", grown[:1], [], "applied"),
        ("a user of C-1 documents joins two more", joins, [], "applied"),
        ("a user of 1 document takes its two free slots", small[:2], [], "applied"),
        ("... and finds none for a third", small[2:], [], "full"),
        ("a new subject joins the 2C+1 star", [LC.sid(f"star{2 * C + 1}", "view", "somebody new")], [], "applied"),
        # 379 entries fill the row's room exactly: patched where it lies, the opening child 79 entries
        # later, in the third 64-entry window instead of the second (a mask that was not rebuilt
        # would pass it as a leaf inside a run)
        ("WP64 +79 before the opening child: in its room", new_sets("WP64_", "x00063z", 79), [], "applied"),
    ]


def moves_starts(t):
    """-> dict of the start ids the moves scenario calls"""
    rw, C = t.rw, CHUNK
    sub = lambda name: int(lookup.resolve_roots(rw, [("n", name, "view")])[0])
    usr = lambda name: W.LOOKUP.start(rw, name)
    d = {"stars": [sub(f"star{k}") for k in CHUNK_SIZES], "lstars": [usr(f"lstar{k}") for k in CHUNK_SIZES],
         "wl": sub("WL4095_r"), "wl96": sub("WL4096_r"), "wp": sub("WP63_r"), "wp64": sub("WP64_r"),
         "wp_child": EC.node_of(rw, EC.member("WP63_x00063")), "small": usr("small"), "fill": sub("fill_doc"),
         "wres": sub("wres000"), "a_user": usr(f"a{C - 1}_0"), "fill_user": usr("fill_u0")}
    assert L.NODE_NONE not in [x for v in d.values() for x in (v if isinstance(v, list) else [v])]
    return d


# ---------------------------------------------------------------------- sizes of the fallback tests
def row_len(ex, v):
    """the entries of v's forward row: the root's child count at depth 2 (0: no row)"""
    try:
        _, kids, _ = ex.expand_ids(int(v), 2)
    except expand.NotFound:
        return 0
    return int(kids[0]) if len(kids) else 0


def lookup_full_bytes(snap, n0):
    """what the lookup handle's full upload copies: rev_off over n_cap + 1 ids, rev_col with four
    words per reserved id, a type per expandable id.  n0: the nodes at build time"""
    st, g = snap.stats(), snap.graph()
    n_cap = n0 + max(1024, n0 // 8)
    rev_words = int(g["rev_off"][-1]) + 4 * (n_cap - st["num_nodes"])
    return 8 * (n_cap + 1) + 4 * rev_words + 4 * st["num_expandable"], rev_words


def rev_row_words(snap, v):
    g = snap.graph()
    return int(g["rev_off"][int(v) + 1] - g["rev_off"][int(v)])


def backlog(words, full_bytes):
    """ListHandle::try_patch: the patched rows' words take the fallback"""
    return words * 4 > full_bytes // 4


def fallback_rows(users=1500, groups=30):
    """the series' base rows and `users` more users with three groups each (600 users with two
    groups each stay under the lookup threshold: the reserved ids alone are 30 KB of a full upload): one write that gives every group one more user and every
    user one more group rewrites every row of both handles"""
    rows = set(RC.base_rows())
    for u in range(users):
        for j in range(3):
            rows.add(RC.user_row(f"g{(u + 7 * j) % groups}", f"w{u}"))
    return sorted(rows, key=repr)


def fallback_write(users=1500, groups=30):
    """every user w<u> joins one more group: every group gains users, every user a group"""
    return [RC.user_row(f"g{(u + 21) % groups}", f"w{u}") for u in range(users)]


# ---------------------------------------------------------------------- the refresh state machine, on the host
COUNTERS = ("full_uploads", "patched_refreshes", "rows_moved", "compactions", "fallbacks_backlog", "fallbacks_trimmed")


class HandleModel:
    """ListHandle::try_patch and the two upload() functions (hip_host.hpp, subjects.hip,
    lookup.hip) replayed on the host from the snapshot's patch log: which path serves each
    refresh of a handle created now, and the counters it ends with.  The GPU tests assert the
    handles' refresh statistics against it; the CPU test proves every scenario's outcome with it.
    (A model is a reader of the log: close it where a test looks at the log's trimming.)"""

    def __init__(self, snap, kind, n0=None, slack=None, garbage=None):
        self.snap, self.kind, self.slack, self.garbage = snap, kind, slack, garbage
        self.n0 = snap.stats()["num_nodes"] if n0 is None else n0
        self.reader = snap.patch_reader()
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.uploads = 0
        self.margin = None  # the smallest factor by which a refresh missed or passed the backlog threshold
        self._upload()

    def close(self):
        self.reader.close()

    def _upload(self):
        self.stats["full_uploads"] += 1
        self.uploads += 1
        if self.kind == "lookup":
            self.full_bytes = lookup_full_bytes(self.snap, self.n0)[0]
            return
        st = self.snap.stats()
        ex = expand.Engine(self.snap)
        lens = [row_len(ex, v) for v in range(st["num_expandable"])]
        self.cap = [n + n // 4 + 4 for n in lens]
        self.tail, self.dirty = sum(self.cap), 0
        slack = max(st["num_edges"] // 8, 1 << 16) if self.slack is None else self.slack
        self.col_words = self.tail + slack
        self.full_bytes = (len(lens) + 1) * 16 + 4 * self.tail + 4 * st["num_nodes"]
        self.moved_at = {}  # row -> where its last move put it

    def refresh(self):
        """the first call of the handle behind one or more applied writes -> "patch",
        "compaction" or "backlog" (None: no write since the last call)"""
        entries = self.reader.read()
        if not entries:
            return None
        want = L.PATCH_REVERSE if self.kind == "lookup" else L.PATCH_FORWARD_FULL
        nodes = sorted({v for k, v in entries if k == want})
        words, tail, moves = 0, None, []
        if self.kind == "lookup":
            g = self.snap.graph()["rev_off"]
            words = sum(int(g[v + 1] - g[v]) for v in nodes)
        else:
            ex = expand.Engine(self.snap)
            tail, dirty = self.tail, self.dirty
            for v in nodes:
                n = row_len(ex, v)
                if n > self.cap[v]:
                    cap = n + n // 4 + 4
                    if tail + cap > self.col_words:
                        return self._fall("compactions", "compaction")
                    moves.append((v, cap, tail))
                    tail, dirty = tail + cap, dirty + self.cap[v]
                words += n
            bound = max(self.snap.stats()["num_edges"] // 4, 1 << 20) if self.garbage is None else self.garbage
            if dirty > bound:
                return self._fall("compactions", "compaction")
        ratio = (words * 4) / (self.full_bytes // 4)
        over = backlog(words, self.full_bytes)
        factor = ratio if over else (1 / ratio if ratio else float("inf"))
        self.margin = factor if self.margin is None else min(self.margin, factor)
        if over:
            return self._fall("fallbacks_backlog", "backlog")
        if self.kind != "lookup":
            self.tail, self.dirty = tail, dirty
            for v, cap, at in moves:
                self.cap[v], self.moved_at[v] = cap, at
        self.stats["patched_refreshes"] += 1
        self.stats["rows_moved"] += len(moves)
        self.uploads += 1
        return "patch"

    def _fall(self, counter, name):
        self.stats[counter] += 1
        self._upload()
        return name

    def assert_handle(self, h, what=""):
        """the handle's refresh statistics are the model's, counter for counter"""
        rs = h.refresh_stats()
        assert {k: rs[k] for k in COUNTERS} == self.stats, (what, self.kind, rs, self.stats)
        assert h.stats()["uploads"] == self.uploads, (what, self.kind)


# ---------------------------------------------------------------------- the fallback scenarios
FB_USERS, FB_GROUPS = 4000, RC.N_GROUPS


def fb_rows():
    return fallback_rows(FB_USERS, FB_GROUPS)


def fb_large_write():
    return fallback_write(FB_USERS, FB_GROUPS)


def fb_small_write(k=0):
    """one new subject in one group: a write every handle patches"""
    return [RC.user_row("g3", f"late{k}")]


def fb_idle_writes(count=15, per=400, step=250):
    """`count` small writes: write k gives group g<k> the users w<k * step> .. that are not its
    members yet.  Each stays far under the backlog threshold; together they pass it"""
    out = []
    for k in range(count):
        users = [u for u in range(k * step, k * step + per) if k not in {(u + 7 * j) % FB_GROUPS for j in range(3)}]
        out.append([RC.user_row(f"g{k}", f"w{u}") for u in users])
    return out


def rc_starts(snap, users=("u1", "u2", "u3")):
    """(roots, second, targets, path_roots) of a graph over the series' rows for all_calls"""
    node = lambda s: RC.node_of(snap, s)
    g = [node(lookup.SubjectSet("groups", f"g{i}", "member")) for i in (0, 3, 4)]
    docs = [node(lookup.SubjectSet("docs", f"d{d}", "viewer")) for d in range(3)]
    return [g[0], g[1], docs[0]], g[2], [node(lookup.SubjectID(u)) for u in users] + [g[1]], docs + [g[0]]


def rc_equal(t, users=("u1", "u2", "u3"), more_roots=()):
    """a Twin over the series' rows: its host lists and trees equal the read-only snapshot's on
    the starts the scenarios call, and the mirror holds as many rows as the snapshot"""
    roots, second, targets, path_roots = rc_starts(t.rw, users)
    roots = roots + [second] + path_roots + list(more_roots)
    host_equal(t, roots, targets)
    trees_equal(t, roots)
    assert t.rw.stats()["num_rows"] == t.ro.stats()["num_rows"] == len(t.rows)


def growth_rows():
    """the rows of test_list_refresh_gpu.growth_snapshot (test_writable_layout_host.py holds the
    two snapshots next to each other)"""
    rows = set(RC.base_rows())
    rows |= {RC.user_row(f"g{k % RC.N_GROUPS}", f"x{k}") for k in range(400)}
    rows |= {RC.user_row("grow", f"u{u}") for u in (1, 2, 3)} | {RC.nest_row("g0", "grow")}
    return sorted(rows, key=repr)


def garbage_rows():
    """the series' rows, 400 more users, and a group `grow` of 20 members inside g0"""
    rows = set(RC.base_rows())
    rows |= {RC.user_row(f"g{k % RC.N_GROUPS}", f"x{k}") for k in range(400)}
    rows |= {RC.user_row("grow", f"u{u}") for u in range(20)} | {RC.nest_row("g0", "grow")}
    return sorted(rows, key=repr)


GARBAGE_KNOB = 64


def garbage_writes():
    """grow has 20 entries in a room of 29.  +10: 30 entries move to the tail with room for 41, 29
    words of garbage.  +12: 42 entries want to move again, 29 + 41 = 70 words of garbage pass the
    knob's 64: a compaction, after which the row has room for 56 in a fresh arena.  +15: 57 entries
    move once more, 56 words of garbage from zero: no compaction"""
    out, k = [], 0
    for n in (10, 12, 15):
        out.append([RC.user_row("grow", f"m{k + i}") for i in range(n)])
        k += n
    return out


LIFE_KNOBS = {"KETOGPU_LIST_ARENA_SLACK": "40", "KETOGPU_LIST_ARENA_GARBAGE": "200", "KETOGPU_LIST_BOUND_STEP": "1"}
LIFE_GROW_TO = 24  # entries: room for 34 words, within a fresh tail of 40


def life_rows():
    """RC.base_rows() plus test_list_refresh_gpu.growth_snapshot's 400 filler users"""
    rows = set(RC.base_rows())
    rows |= {RC.user_row(f"g{k % RC.N_GROUPS}", f"x{k}") for k in range(400)}
    return sorted(rows, key=repr)


def life_tail(rows):
    """two scripted writes behind the series: the viewers of d1, then of d2, grow to LIFE_GROW_TO
    entries.  Whatever the series left of the tail, the first of them moves its row or finds the
    tail exhausted, which lays a fresh tail out, and the second does the other"""
    out = []
    for d in ("d1", "d2"):
        have = sum(1 for r in rows if r[:3] == (2, d, "viewer"))
        assert have <= 15  # (so the room the row has, whenever it was laid out, is under LIFE_GROW_TO)
        out.append([(2, d, "viewer", f"life_{d}_{i}", None, None, None) for i in range(LIFE_GROW_TO - have)])
    return out


def life_writes(rows):
    """the whole life -> yields (label, inserts, deletes, refused); `rows` is the mirror the
    caller folds applied writes into (RC.Writes.rows)"""
    writes = RC.Writes(rows, seed=5)
    for k in range(RC.Writes.COUNT):
        ins, dele, refused = writes.write(k)
        yield f"write {k}", ins, dele, refused, writes
    for k, ins in enumerate(life_tail(writes.rows)):
        yield f"scripted {k}", ins, [], False, writes
