"""Reverse lookup and subject listing: every object a subject can reach (include/ketogpu.h
ketogpu_lookup_*), every subject that can reach an object (ketogpu_subjects_*).

"Which documents can this user view?" — OpenFGA's ListObjects, SpiceDB's LookupResources.
lookup(t, T) is the set of expandable nodes r of object type T with SubjectIsAllowed(r, t):
the backward closure B(t) over the snapshot's reverse rows (DESIGN.md "Reverse lookup").
`host_lookup` walks the rows on the CPU; `Lookup` is the device handle (keto_amd/csrc/lookup.hip).

"Who can view this document?" — OpenFGA's ListUsers, SpiceDB's LookupSubjects.
subjects(r, C) is the set of nodes t of class C with SubjectIsAllowed(r, t): the forward
closure F(r) over the rows the check engine sees (DESIGN.md "Subject listing").
`host_subjects` walks the rows on the CPU; `Subjects` is the device handle
(keto_amd/csrc/subjects.hip).

"Why is this check allowed?" — SpiceDB's check trace.  `host_path` / `Lookup.Explain` return one
path root ... target with the fewest hops over the same reverse rows (ketogpu_snapshot_path,
ketogpu_lookup_paths on the lookup handle; DESIGN.md "Explain").

Both questions also come sorted and paged (ketogpu_lookup_page / ketogpu_subjects_page,
DESIGN.md "Sorted, paged lists"): `*_page_raw` on ids, `list_*_page` on names with Keto's
page_size / page_token convention.  The order is by node id.  `HostLookup` / `HostSubjects` are
the CPU twins with the same methods: the yardstick of the device calls, and a backend for the
HTTP routes where there is no GPU.

Two lists under an operator — who can both submit and approve, what one user sees that another
does not — come from one call as well (ketogpu_lookup_combine / ketogpu_subjects_combine and their
_page forms, DESIGN.md "Combined listings"): `combine_ids`, `combine_page_raw`,
`ListObjectsCombined` / `ListSubjectsCombined` with op "and" | "andnot" | "or", on the device
handles and, as numpy set algebra over the host lists, on the CPU twins.

A listing also comes cut at a number of hops — who holds this document directly, who through one
group (ketogpu_*_ids_depth / ketogpu_*_page_depth, DESIGN.md "Depth-limited listings"):
`lookup_depth` / `subject_depth` and their `_raw` and `_page_raw` forms take one `max_depth` per
request (DEPTH_ALL: no limit) and also return `frontier`, the interior members at exactly that
distance; `list_*_depth_batch` return names and `complete`, and the named calls take a keyword
`max_depth`.  `host_lookup_depth` / `host_subjects_depth` are the level-by-level CPU twins.

The full-list calls take a keyword `wide` (ketogpu_*_ids_wide, DESIGN.md "Chip-wide closures"): the
same lists, with the closures too large for one wave spread over the whole device instead of one
workgroup each; `wide_stats()` counts them.  The CPU twins accept and ignore it.  The paged and the
depth calls take it too (ketogpu_*_page_wide / ketogpu_*_ids_depth_wide, DESIGN.md "Chip-wide pages
and depths"): `*_page_raw`, `*_depth_raw`, `*_depth_page_raw`, `list_*_page`, `list_*_page_batch` and
`list_*_depth_batch`, with or without `max_depth`; together with `with_via` it raises ValueError.
`list_*_batch` / `ListObjects` / `ListSubjects` keep refusing `wide` with `max_depth`: the depth
lists by name are `list_*_depth_batch(..., wide=True)`.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from . import persistence
from .relationtuple import SubjectID, SubjectSet

TYPE_ANY, TYPE_NONE = L.TYPE_ANY, L.TYPE_NONE
TRUNCATED, INVALID = L.LOOKUP_TRUNCATED, L.LOOKUP_INVALID
CLASS_SUBJECT_ID, CLASS_UNTYPED_SET = L.CLASS_SUBJECT_ID, L.CLASS_UNTYPED_SET
PAGE_LIMIT_MAX, PAGE_INVALID = L.PAGE_LIMIT_MAX, L.PAGE_INVALID
DEPTH_ALL = L.DEPTH_ALL


# ---- pages: tokens and sizes, shared by the device handles and their CPU twins
def parse_page_token(token):
    """"" (the first page) -> 0; otherwise the decimal string of the next lower bound: at most
    10 digits and <= 0xFFFFFFFF, anything else raises KetoError(EINVAL)"""
    if token == "":
        return 0
    if not isinstance(token, str) or len(token) > 10 or not (token.isascii() and token.isdigit()) \
            or int(token) > 0xFFFFFFFF:
        raise L.KetoError(L.EINVAL, f"malformed page token {token!r}")
    return int(token)


def check_page_size(page_size):
    if isinstance(page_size, bool) or not isinstance(page_size, (int, np.integer)) \
            or not 1 <= page_size <= PAGE_LIMIT_MAX:
        raise L.KetoError(L.EINVAL, f"page size {page_size!r} is outside [1, {PAGE_LIMIT_MAX}]")
    return int(page_size)


def next_page_token(ids, returned, remaining):
    """"" exactly when nothing remains after this page, else the id after the page's last"""
    return "" if int(remaining) == int(returned) else str(int(ids[int(returned) - 1]) + 1)


def _page_of(ids, lo, limit):
    """one request of a CPU twin: the page of an ascending list -> (ids, count, remaining)"""
    k = int(np.searchsorted(ids, lo, side="left"))
    return ids[k:k + limit], len(ids), len(ids) - k


def _host_pages(lists, invalid, from_ids, limit):
    """(out[n, limit], returned, count, remaining) as the device calls return them"""
    limit = check_page_size(limit)
    n = len(lists)
    lo = np.zeros(n, dtype=np.uint32) if from_ids is None else np.ascontiguousarray(from_ids, dtype=np.uint32)
    if len(lo) != n:
        raise L.KetoError(L.EINVAL, "one lower bound per request")
    out = np.zeros((n, limit), dtype=np.uint32)
    returned = np.zeros(n, dtype=np.uint32)
    count, remaining = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i, ids in enumerate(lists):
        if invalid[i]:
            returned[i] = PAGE_INVALID
            continue
        page, count[i], remaining[i] = _page_of(ids, lo[i], limit)
        out[i, :len(page)] = page
        returned[i] = len(page)
    return out, returned, count, remaining


def _page_args(ids, from_ids, limit):
    """the arrays of one ketogpu_*_page call (the library itself judges `limit`)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n = len(ids)
    lo = None if from_ids is None else np.ascontiguousarray(from_ids, dtype=np.uint32)
    if lo is not None and len(lo) != n:
        raise L.KetoError(L.EINVAL, "one lower bound per request")
    limit = int(limit)
    width = limit if 1 <= limit <= PAGE_LIMIT_MAX else 1
    out = np.empty((max(n, 1), width), dtype=np.uint32)
    returned = np.empty(max(n, 1), dtype=np.uint32)
    count = np.empty(max(n, 1), dtype=np.uint64)
    remaining = np.empty(max(n, 1), dtype=np.uint64)
    return ids, lo, n, limit, out, returned, count, remaining


def _no_wide_via(wide, with_via):
    """there is no wide via call (DESIGN.md "Chip-wide pages and depths")"""
    if wide and with_via:
        raise ValueError("wide=True does not take with_via")


class _ObjectPages:
    """list_objects_page over self.lookup_page_raw and self.snapshot"""

    def list_objects_page_batch(self, namespace, relation, requests, page_size=100, max_depth=None, with_via=False,
                                wide=False):
        """requests: (subject, page_token) pairs, one device call for all of them -> per
        request (object names in node-id order, next_page_token, total).  max_depth (one number,
        or one per request): the objects within that many hops, and a fourth element `complete`.
        with_via: every item is (name, via, hops), via the subject the granting node stands for.
        wide: the large closures run in the wide tier (not with with_via: ValueError)"""
        _no_wide_via(wide, with_via)
        if with_via:
            return self._list_objects_page_via(namespace, relation, list(requests), page_size, max_depth)
        if max_depth is not None:
            return self._list_objects_page_depth(namespace, relation, list(requests), page_size, max_depth, wide)
        page_size = check_page_size(page_size)
        requests = list(requests)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, [s for s, _ in requests])
        if ty == TYPE_NONE:  # unknown namespace or unused pair: nothing (check answers false there)
            return [([], "", 0) for _ in requests]
        out, returned, count, remaining = self.lookup_page_raw(targets, lo, ty, page_size, wide=wide)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            names = [self.snapshot.node_info(int(v))["id"] for v in out[i, :k]]
            res.append((names, next_page_token(out[i], k, remaining[i]), int(count[i])))
        return res

    def list_objects_page(self, namespace, relation, subject, page_size=100, page_token="", max_depth=None,
                          with_via=False, wide=False):
        """-> (items, next_page_token, total): at most page_size object names o with
        Check(namespace:o#relation@subject), in node-id order from the token on.  With max_depth:
        of the objects within that many hops, -> (items, next_page_token, total, complete).  With
        with_via the items are (name, via, hops).  wide: as in list_objects_page_batch"""
        return self.list_objects_page_batch(namespace, relation, [(subject, page_token)], page_size, max_depth,
                                            with_via, wide)[0]

    def _list_objects_page_via(self, namespace, relation, requests, page_size, max_depth):
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        depth = depth_array(max_depth, len(requests))
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, [s for s, _ in requests])
        tail = lambda complete: () if max_depth is None else (complete,)
        if ty == TYPE_NONE:
            return [([], "", 0) + tail(True) for _ in requests]
        out, via, hops, returned, count, remaining, frontier = self.lookup_via_page_raw(targets, depth, lo, ty,
                                                                                        page_size)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            items = [(self.snapshot.node_info(int(v))["id"], self.snapshot.describe(int(w)), int(h))
                     for v, w, h in zip(out[i, :k], via[i, :k], hops[i, :k])]
            res.append((items, next_page_token(out[i], k, remaining[i]), int(count[i])) + tail(not frontier[i]))
        return res

    def _list_objects_page_depth(self, namespace, relation, requests, page_size, max_depth, wide=False):
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        depth = depth_array(max_depth, len(requests))
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, [s for s, _ in requests])
        if ty == TYPE_NONE:
            return [([], "", 0, True) for _ in requests]
        out, returned, count, remaining, frontier = self.lookup_depth_page_raw(targets, depth, lo, ty, page_size,
                                                                               wide=wide)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            names = [self.snapshot.node_info(int(v))["id"] for v in out[i, :k]]
            res.append((names, next_page_token(out[i], k, remaining[i]), int(count[i]), not frontier[i]))
        return res


class _SubjectPages:
    """list_subjects_page over self.subject_page_raw and self.snapshot"""

    def list_subjects_page_batch(self, requests, kind="ids", page_size=100, max_depth=None, with_via=False,
                                 wide=False):
        """requests: ((namespace, object, relation), page_token) pairs, one device call for all
        of them -> per request (SubjectID / SubjectSet in node-id order, next_page_token, total).
        max_depth (one number, or one per request): the subjects within that many hops, and a
        fourth element `complete`.  with_via: every item is (subject, via, hops), via the subject
        set whose tuple grants it.  wide: the large closures run in the wide tier (not with
        with_via: ValueError)"""
        _no_wide_via(wide, with_via)
        if with_via:
            return self._list_subjects_page_via(list(requests), kind, page_size, max_depth)
        if max_depth is not None:
            return self._list_subjects_page_depth(list(requests), kind, page_size, max_depth, wide)
        page_size = check_page_size(page_size)
        requests = list(requests)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        cls = _class_of_kind(self.snapshot, kind)
        roots = resolve_roots(self.snapshot, [tuple(r) for r, _ in requests])
        if cls == TYPE_NONE:
            return [([], "", 0) for _ in requests]
        out, returned, count, remaining = self.subject_page_raw(roots, lo, cls, page_size, wide=wide)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            subs = [self.snapshot.describe(int(v)) for v in out[i, :k]]
            res.append((subs, next_page_token(out[i], k, remaining[i]), int(count[i])))
        return res

    def list_subjects_page(self, namespace, object, relation, kind="ids", page_size=100, page_token="",
                           max_depth=None, with_via=False, wide=False):
        """-> (items, next_page_token, total): at most page_size subjects s with
        Check(namespace:object#relation@s), in node-id order from the token on.  With max_depth:
        of the subjects within that many hops, -> (items, next_page_token, total, complete).  With
        with_via the items are (subject, via, hops).  wide: as in list_subjects_page_batch"""
        return self.list_subjects_page_batch([((namespace, object, relation), page_token)], kind, page_size,
                                             max_depth, with_via, wide)[0]

    def _list_subjects_page_via(self, requests, kind, page_size, max_depth):
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        depth = depth_array(max_depth, len(requests))
        cls = _class_of_kind(self.snapshot, kind)
        roots = resolve_roots(self.snapshot, [tuple(r) for r, _ in requests])
        tail = lambda complete: () if max_depth is None else (complete,)
        if cls == TYPE_NONE:
            return [([], "", 0) + tail(True) for _ in requests]
        out, via, hops, returned, count, remaining, frontier = self.subject_via_page_raw(roots, depth, lo, cls,
                                                                                         page_size)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            items = [(self.snapshot.describe(int(v)), self.snapshot.describe(int(w)), int(h))
                     for v, w, h in zip(out[i, :k], via[i, :k], hops[i, :k])]
            res.append((items, next_page_token(out[i], k, remaining[i]), int(count[i])) + tail(not frontier[i]))
        return res

    def _list_subjects_page_depth(self, requests, kind, page_size, max_depth, wide=False):
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(tok) for _, tok in requests], dtype=np.uint32)
        depth = depth_array(max_depth, len(requests))
        cls = _class_of_kind(self.snapshot, kind)
        roots = resolve_roots(self.snapshot, [tuple(r) for r, _ in requests])
        if cls == TYPE_NONE:
            return [([], "", 0, True) for _ in requests]
        out, returned, count, remaining, frontier = self.subject_depth_page_raw(roots, depth, lo, cls, page_size,
                                                                                wide=wide)
        res = []
        for i in range(len(requests)):
            k = int(returned[i])
            subs = [self.snapshot.describe(int(v)) for v in out[i, :k]]
            res.append((subs, next_page_token(out[i], k, remaining[i]), int(count[i]), not frontier[i]))
        return res


# ---- depth-limited listings (include/ketogpu.h "depth-limited listings", DESIGN.md
# "Depth-limited listings"), shared by the device handles and their CPU twins
def depth_array(max_depth, n):
    """one limit for every request, or one per request -> uint32[n]; None -> None (no limit for
    any request).  DEPTH_ALL (0) is no limit; a limit that is no integer in [0, 2^32) raises
    KetoError(EINVAL)"""
    if max_depth is None:
        return None
    try:
        d = np.asarray(max_depth)
        if d.dtype == bool or not np.issubdtype(d.dtype, np.integer):
            raise ValueError
        d = np.broadcast_to(d, (n,)) if d.ndim == 0 else d
        if d.shape != (n,) or (n and (d.min() < 0 or d.max() > 0xFFFFFFFF)):
            raise ValueError
    except (ValueError, TypeError):
        raise L.KetoError(L.EINVAL, f"max_depth {max_depth!r}: expected one integer in [0, 2^32) for all requests "
                                    "or one per request") from None
    return np.ascontiguousarray(d, dtype=np.uint32)


def _depth_lists(raw, ids, max_depth, cap, invalid):
    """_all_lists over a depth call raw(ids, depth, cap) -> (out, begin, count, frontier, needed)
    -> (ascending lists, frontier).  The frontier of a request does not depend on the capacity."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    depth = depth_array(max_depth, len(ids))
    frontier = np.zeros(len(ids), dtype=np.uint64)

    def call(idx, c):
        out, begin, count, fr, needed = raw(ids[idx], None if depth is None else depth[idx], c)
        frontier[idx] = fr
        return out, begin, count, needed
    lists = _all_lists(call, len(ids), 64 * len(ids) if cap is None else int(cap), True,
                       lambda k: f"id {int(ids[k])} is outside the snapshot")
    return lists, frontier


def _host_cursor(lists, capacity):
    """(out, begin, count, needed) as a cursor call lays its lists out (None: INVALID)"""
    n = len(lists)
    out = np.zeros(int(capacity), dtype=np.uint32)
    begin, count = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    cursor = 0
    for i, ids in enumerate(lists):
        if ids is None:
            begin[i] = INVALID
            continue
        count[i] = len(ids)
        if cursor + len(ids) <= capacity:
            out[cursor:cursor + len(ids)] = ids
            begin[i] = cursor
        else:
            begin[i] = TRUNCATED
        cursor += len(ids)  # every list reserves, written or not
    return out, begin, count, cursor


class _HostDepth:
    """the depth calls of a CPU twin over self._depth_members(x, k, filter_id) -> (ascending ids,
    frontier), laid out as the device calls lay their results out"""

    def _depth_all(self, ids, max_depth, filter_id):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        depth = depth_array(max_depth, len(ids))
        n_nodes = self.snapshot.stats()["num_nodes"]
        lists, frontier = [], np.zeros(len(ids), dtype=np.uint64)
        for i, x in enumerate(ids):
            if x >= n_nodes and x != L.NODE_NONE:
                lists.append(None)
                continue
            m, frontier[i] = self._depth_members(int(x), DEPTH_ALL if depth is None else int(depth[i]), filter_id)
            lists.append(m)
        return lists, frontier

    def _ids_depth_raw(self, ids, max_depth, filter_id=TYPE_ANY, capacity=0):
        lists, frontier = self._depth_all(ids, max_depth, filter_id)
        out, begin, count, needed = _host_cursor(lists, capacity)
        return out, begin, count, frontier, needed

    def _page_depth_raw(self, ids, max_depth, from_ids=None, filter_id=TYPE_ANY, limit=100):
        lists, frontier = self._depth_all(ids, max_depth, filter_id)
        return _host_pages(lists, [m is None for m in lists], from_ids, limit) + (frontier,)


class _ObjectsDepth:
    """the depth-limited object lists over self.lookup_depth_raw and self.snapshot"""

    def lookup_depth(self, targets, max_depth, type_id=TYPE_ANY, capacity=None, wide=False):
        """-> (one ascending uint32 array per target, frontier): lookup_ids within max_depth hops
        (one number, or one per target; DEPTH_ALL: no limit), with lookup_ids' re-issue of
        truncated lists.  frontier[i] == 0: list i is the whole closure.  wide: the large closures
        run in the wide tier."""
        return _depth_lists(lambda t, d, c: self.lookup_depth_raw(t, d, type_id, c, wide=wide), targets, max_depth,
                            capacity, None)

    def list_objects_depth_batch(self, namespace, relation, subjects, max_depth, wide=False):
        """per subject: the sorted object names o with Check(namespace:o#relation@subject) that
        are within max_depth hops of the subject -> (lists, complete); complete[i]: no deeper
        level was cut off, list i is what list_objects_batch gives.  wide: as in lookup_depth"""
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, list(subjects))
        depth = depth_array(max_depth, len(targets))
        if ty == TYPE_NONE:  # unknown namespace or unused pair: nothing (check answers false there)
            return [[] for _ in targets], [True] * len(targets)
        lists, frontier = self.lookup_depth(targets, depth, ty, wide=wide)
        return ([sorted(self.snapshot.node_info(int(v))["id"] for v in ids) for ids in lists],
                [not f for f in frontier])


class _SubjectsDepth:
    """the depth-limited subject lists over self.subject_depth_raw and self.snapshot"""

    def subject_depth(self, roots, max_depth, cls=TYPE_ANY, capacity=None, wide=False):
        """-> (one ascending uint32 array per root, frontier): subject_ids within max_depth hops
        (one number, or one per root; DEPTH_ALL: no limit), with subject_ids' re-issue of
        truncated lists.  frontier[i] == 0: list i is the whole closure.  wide: the large closures
        run in the wide tier."""
        return _depth_lists(lambda r, d, c: self.subject_depth_raw(r, d, cls, c, wide=wide), roots, max_depth,
                            capacity, None)

    def list_subjects_depth_batch(self, roots, max_depth, kind="ids", wide=False):
        """per (namespace, object, relation) root: the subjects s with Check(root@s) that are
        within max_depth hops of the root -> (lists, complete), as list_subjects_batch lists them.
        wide: as in subject_depth"""
        roots = list(roots)
        cls = _class_of_kind(self.snapshot, kind)
        ids = resolve_roots(self.snapshot, roots)
        depth = depth_array(max_depth, len(ids))
        if cls == TYPE_NONE:
            return [[] for _ in roots], [True] * len(roots)
        lists, frontier = self.subject_depth(ids, depth, cls, wide=wide)
        return [_subjects_of(self.snapshot, v) for v in lists], [not f for f in frontier]


# ---- listings that say why (include/ketogpu.h "listings that say why", DESIGN.md "Grant
# trees"), shared by the device handles and their CPU twins
def grant_chain(ids, via, start, u):
    """one member's chain to the start over an answer under TYPE_ANY (ids ascending, via parallel
    to them) -> [u, via(u), via(via(u)), ..., start]: hops(u) + 1 nodes.  Only an ANY answer is a
    complete tree; a via that is neither the start nor a listed member raises KeyError"""
    ids = np.asarray(ids)
    chain, cur = [int(u)], int(u)
    for _ in range(len(ids) + 1):
        k = int(np.searchsorted(ids, cur))
        if k >= len(ids) or int(ids[k]) != cur:
            raise KeyError(f"node {cur} is not a member of this answer")
        cur = int(via[k])
        chain.append(cur)
        if cur == int(start):
            return chain
    raise KeyError(f"the chain of {int(u)} does not end at {int(start)}")


def _via_lists(raw, ids, max_depth, cap):
    """every list of a via call raw(ids, depth, cap) -> (out, via, hops, begin, count, frontier,
    needed), with _all_lists' re-issue of truncated lists -> (per request (ids ascending, via,
    hops), frontier)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    depth = depth_array(max_depth, len(ids))
    n = len(ids)
    frontier = np.zeros(n, dtype=np.uint64)
    res = [None] * n
    idx = np.arange(n)
    cap = 64 * n if cap is None else int(cap)
    while len(idx):
        out, via, hops, begin, count, fr, _ = raw(ids[idx], None if depth is None else depth[idx], cap)
        frontier[idx] = fr
        if (begin == INVALID).any():
            raise L.KetoError(L.EINVAL, f"id {int(ids[idx[begin == INVALID][0]])} is outside the snapshot")
        done = begin != TRUNCATED
        for k in np.nonzero(done)[0]:
            b, c = int(begin[k]), int(count[k])
            order = np.argsort(out[b:b + c], kind="stable")
            res[idx[k]] = (out[b:b + c][order], via[b:b + c][order], hops[b:b + c][order])
        cap = int(count[~done].sum())  # exactly what the rest needs: nothing is truncated twice
        idx = idx[~done]
    return res, frontier


def _host_via(snapshot, call, x, filter_id, max_depth):
    """one ketogpu_snapshot_*_via call -> (ids ascending, via, hops (uint32 each), frontier)"""
    p, pv, ph, n, fr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    lib = snapshot.L
    L.check(getattr(lib, call)(snapshot.h, int(x), int(filter_id), int(max_depth), C.byref(p), C.byref(pv),
                               C.byref(ph), C.byref(n), C.byref(fr)))
    try:
        return tuple(np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_uint32)), (n.value,)).copy() if n.value
                     else np.zeros(0, dtype=np.uint32) for q in (p, pv, ph)) + (fr.value,)
    finally:
        for q in (p, pv, ph):
            lib.ketogpu_free(q)


def host_lookup_via(snapshot, target, max_depth=DEPTH_ALL, type_id=TYPE_ANY):
    """ketogpu_snapshot_lookup_via: (host_lookup_depth's ids, via, hops, frontier).  No GPU."""
    return _host_via(snapshot, "ketogpu_snapshot_lookup_via", target, type_id, max_depth)


def host_subjects_via(snapshot, root, max_depth=DEPTH_ALL, cls=TYPE_ANY):
    """ketogpu_snapshot_subjects_via: (host_subjects_depth's ids, via, hops, frontier).  No GPU."""
    return _host_via(snapshot, "ketogpu_snapshot_subjects_via", root, cls, max_depth)


class _HostVia:
    """the via calls of a CPU twin over self._via_members(x, k, filter_id) -> (ascending ids,
    via, hops, frontier), laid out as the device calls lay their results out"""

    def _via_all(self, ids, max_depth, filter_id):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        depth = depth_array(max_depth, len(ids))
        n_nodes = self.snapshot.stats()["num_nodes"]
        empty = np.zeros(0, dtype=np.uint32)
        lists, frontier = [], np.zeros(len(ids), dtype=np.uint64)
        for i, x in enumerate(ids):
            if x >= n_nodes and x != L.NODE_NONE:
                lists.append(None)
            elif x == L.NODE_NONE:
                lists.append((empty, empty, empty))
            else:
                m = self._via_members(int(x), DEPTH_ALL if depth is None else int(depth[i]), filter_id)
                lists.append(m[:3])
                frontier[i] = m[3]
        return lists, frontier

    def _ids_via_raw(self, ids, max_depth, filter_id=TYPE_ANY, capacity=0):
        lists, frontier = self._via_all(ids, max_depth, filter_id)
        out, begin, count, needed = _host_cursor([m if m is None else m[0] for m in lists], capacity)
        via, hops = np.zeros(int(capacity), dtype=np.uint32), np.zeros(int(capacity), dtype=np.uint32)
        for m, b, c in zip(lists, begin, count):
            if m is not None and b != TRUNCATED:
                via[int(b):int(b) + int(c)], hops[int(b):int(b) + int(c)] = m[1], m[2]
        return out, via, hops, begin, count, frontier, needed

    def _page_via_raw(self, ids, max_depth, from_ids=None, filter_id=TYPE_ANY, limit=100):
        lists, frontier = self._via_all(ids, max_depth, filter_id)
        invalid = [m is None for m in lists]
        out, returned, count, remaining = _host_pages([m if m is None else m[0] for m in lists], invalid, from_ids,
                                                      limit)
        via, hops = np.zeros_like(out), np.zeros_like(out)
        for i, m in enumerate(lists):
            if m is None:
                continue
            k = int(np.searchsorted(m[0], 0 if from_ids is None else from_ids[i], side="left"))
            r = int(returned[i])
            via[i, :r], hops[i, :r] = m[1][k:k + r], m[2][k:k + r]
        return out, via, hops, returned, count, remaining, frontier


class _ObjectsVia:
    """the object lists that say why over self.lookup_via_raw and self.snapshot"""

    def lookup_via(self, targets, max_depth=None, type_id=TYPE_ANY, capacity=None):
        """-> (per target (ids ascending, via, hops), frontier): lookup_depth's lists with, for
        every member, the node whose reverse row it was first seen in (an entry of the member's
        own row, one hop nearer the target) and its hop count.  Truncated lists are issued again."""
        return _via_lists(lambda t, d, c: self.lookup_via_raw(t, d, type_id, c), targets, max_depth, capacity)

    def list_objects_via_batch(self, namespace, relation, subjects, max_depth=None):
        """per subject: (object name, via, hops) for the objects o with
        Check(namespace:o#relation@subject), sorted by name; via is the subject (a subject set,
        or the subject itself at one hop) that o holds directly on its way to the subject"""
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, list(subjects))
        if ty == TYPE_NONE:  # unknown namespace or unused pair: nothing (check answers false there)
            return [[] for _ in targets]
        lists, _ = self.lookup_via(targets, max_depth, ty)
        return [sorted(((self.snapshot.node_info(int(v))["id"], self.snapshot.describe(int(w)), int(h))
                        for v, w, h in zip(*m)), key=lambda e: e[0]) for m in lists]


class _SubjectsVia:
    """the subject lists that say why over self.subject_via_raw and self.snapshot"""

    def subject_via(self, roots, max_depth=None, cls=TYPE_ANY, capacity=None):
        """-> (per root (ids ascending, via, hops), frontier): subject_depth's lists with, for
        every member, the node whose row holds it (one hop nearer the root) and its hop count.
        Truncated lists are issued again."""
        return _via_lists(lambda r, d, c: self.subject_via_raw(r, d, cls, c), roots, max_depth, capacity)

    def list_subjects_via_batch(self, roots, kind="ids", max_depth=None):
        """per (namespace, object, relation) root: (subject, via, hops) in list_subjects_batch's
        order; via is the subject set whose tuple names the subject"""
        roots = list(roots)
        cls = _class_of_kind(self.snapshot, kind)
        ids = resolve_roots(self.snapshot, roots)
        if cls == TYPE_NONE:
            return [[] for _ in roots]
        lists, _ = self.subject_via(ids, max_depth, cls)
        res = []
        for m in lists:
            why = {self.snapshot.describe(int(v)): (self.snapshot.describe(int(w)), int(h)) for v, w, h in zip(*m)}
            res.append([(sub,) + why[sub] for sub in _subjects_of(self.snapshot, m[0])])
        return res


# ---- combined listings: M(a) op M(b) (include/ketogpu.h "combined listings", DESIGN.md
# "Combined listings"), shared by the device handles and their CPU twins
OP_AND, OP_ANDNOT, OP_OR = L.COMBINE_AND, L.COMBINE_ANDNOT, L.COMBINE_OR
_OP_NAMES = {"and": OP_AND, "andnot": OP_ANDNOT, "or": OP_OR}


def op_id(op):
    """"and" | "andnot" | "or" -> OP_AND | OP_ANDNOT | OP_OR; a number passes as it is (the
    library judges it); any other name raises KetoError(EINVAL)"""
    if isinstance(op, str):
        if op not in _OP_NAMES:
            raise L.KetoError(L.EINVAL, f"operator {op!r}: expected 'and', 'andnot' or 'or'")
        return _OP_NAMES[op]
    return int(op)


def _pair_args(a, b):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if len(a) != len(b):
        raise L.KetoError(L.EINVAL, "one second id per first id")
    return a, b


class _CombineIds:
    """combine_ids over self.combine_ids_raw"""

    def combine_ids(self, a, b, op, filter_id=TYPE_ANY, capacity=None):
        """-> one ascending uint32 array per pair (a[i], b[i]): M(a) op M(b) under the type /
        class filter.  The first call uses `capacity` ids (default 64 per pair); only the pairs
        whose lists were truncated are issued again, with capacity = what they need.  An id
        outside the snapshot raises EINVAL."""
        a, b = _pair_args(a, b)
        op = op_id(op)
        return _all_lists(lambda idx, cap: self.combine_ids_raw(a[idx], b[idx], op, filter_id, cap), len(a),
                          64 * len(a) if capacity is None else int(capacity), True,
                          lambda k: f"pair ({int(a[k])}, {int(b[k])}) is outside the snapshot")


class _ObjectsCombined(_CombineIds):
    """the named forms of the combined object lists over self.combine_ids / combine_page_raw"""

    def list_objects_combined_batch(self, namespace, relation, subject_pairs, op):
        """per (subject_a, subject_b): the sorted object names o with
        Check(namespace:o#relation@subject_a) op Check(namespace:o#relation@subject_b)"""
        op = op_id(op)
        pairs = list(subject_pairs)
        ty = self.snapshot.type_id(namespace, relation)
        a = resolve_subjects(self.snapshot, [p[0] for p in pairs])
        b = resolve_subjects(self.snapshot, [p[1] for p in pairs])
        if ty == TYPE_NONE:  # unknown namespace or unused pair: nothing (check answers false there)
            return [[] for _ in pairs]
        return [sorted(self.snapshot.node_info(int(v))["id"] for v in ids) for ids in self.combine_ids(a, b, op, ty)]

    def ListObjectsCombined(self, namespace, relation, subject_a, subject_b, op):
        return self.list_objects_combined_batch(namespace, relation, [(subject_a, subject_b)], op)[0]

    def list_objects_combined_page(self, namespace, relation, subject_a, subject_b, op, page_size=100, page_token=""):
        """-> (items, next_page_token, total): list_objects_page of the combined list"""
        op = op_id(op)
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(page_token)], dtype=np.uint32)
        ty = self.snapshot.type_id(namespace, relation)
        a = resolve_subjects(self.snapshot, [subject_a])
        b = resolve_subjects(self.snapshot, [subject_b])
        if ty == TYPE_NONE:
            return [], "", 0
        out, returned, count, remaining = self.combine_page_raw(a, b, op, lo, ty, page_size)
        k = int(returned[0])
        names = [self.snapshot.node_info(int(v))["id"] for v in out[0, :k]]
        return names, next_page_token(out[0], k, remaining[0]), int(count[0])


class _SubjectsCombined(_CombineIds):
    """the named forms of the combined subject lists over self.combine_ids / combine_page_raw;
    roots are (namespace, object, relation) triples"""

    def list_subjects_combined_batch(self, root_pairs, op, kind="ids"):
        """per (root_a, root_b): the subjects s with Check(root_a@s) op Check(root_b@s),
        SubjectIDs then SubjectSets, each sorted"""
        op = op_id(op)
        pairs = list(root_pairs)
        cls = _class_of_kind(self.snapshot, kind)
        a = resolve_roots(self.snapshot, [tuple(p[0]) for p in pairs])
        b = resolve_roots(self.snapshot, [tuple(p[1]) for p in pairs])
        if cls == TYPE_NONE:
            return [[] for _ in pairs]
        return [_subjects_of(self.snapshot, v) for v in self.combine_ids(a, b, op, cls)]

    def ListSubjectsCombined(self, root_a, root_b, op, kind="ids"):
        return self.list_subjects_combined_batch([(root_a, root_b)], op, kind)[0]

    def list_subjects_combined_page(self, root_a, root_b, op, kind="ids", page_size=100, page_token=""):
        """-> (items, next_page_token, total): list_subjects_page of the combined list"""
        op = op_id(op)
        page_size = check_page_size(page_size)
        lo = np.array([parse_page_token(page_token)], dtype=np.uint32)
        cls = _class_of_kind(self.snapshot, kind)
        a = resolve_roots(self.snapshot, [tuple(root_a)])
        b = resolve_roots(self.snapshot, [tuple(root_b)])
        if cls == TYPE_NONE:
            return [], "", 0
        out, returned, count, remaining = self.combine_page_raw(a, b, op, lo, cls, page_size)
        k = int(returned[0])
        subs = [self.snapshot.describe(int(v)) for v in out[0, :k]]
        return subs, next_page_token(out[0], k, remaining[0]), int(count[0])


class _HostCombine:
    """the combined calls of a CPU twin: numpy set algebra over self._members(x, filter_id), the
    ascending host list of one side (None: an id outside the snapshot), laid out as the device
    calls lay their results out"""

    def _combined(self, a, b, op, filter_id):
        a, b = _pair_args(a, b)
        op = op_id(op)
        if op not in (OP_AND, OP_ANDNOT, OP_OR):
            raise L.KetoError(L.EINVAL, f"unknown combine operator {op}")
        fn = {OP_AND: np.intersect1d, OP_ANDNOT: np.setdiff1d, OP_OR: np.union1d}[op]
        lists = []
        for x, y in zip(a, b):
            ma, mb = self._members(int(x), filter_id), self._members(int(y), filter_id)
            lists.append(None if ma is None or mb is None else fn(ma, mb).astype(np.uint32))
        return lists

    def _side(self, x, filter_id, host):
        if x >= self.snapshot.stats()["num_nodes"]:
            return np.zeros(0, dtype=np.uint32) if x == L.NODE_NONE else None
        return host(self.snapshot, x, filter_id)

    def combine_ids_raw(self, a, b, op, filter_id=TYPE_ANY, capacity=0):
        lists = self._combined(a, b, op, filter_id)
        n = len(lists)
        out = np.zeros(int(capacity), dtype=np.uint32)
        begin, count = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        cursor = 0
        for i, ids in enumerate(lists):
            if ids is None:
                begin[i] = INVALID
                continue
            count[i] = len(ids)
            if cursor + len(ids) <= capacity:
                out[cursor:cursor + len(ids)] = ids
                begin[i] = cursor
            else:
                begin[i] = TRUNCATED
            cursor += len(ids)  # every list reserves, written or not
        return out, begin, count, cursor

    def combine_page_raw(self, a, b, op, from_ids=None, filter_id=TYPE_ANY, limit=100):
        lists = self._combined(a, b, op, filter_id)
        return _host_pages(lists, [ids is None for ids in lists], from_ids, limit)


def _host_ids(snapshot, call, *args, frontier=None):
    """one ketogpu_snapshot_* call that answers with a malloc'ed id array -> its copy (uint32);
    frontier: a c_uint64 for the trailing output of a depth call"""
    p, n = C.c_void_p(), C.c_uint64()
    lib = snapshot.L
    tail = () if frontier is None else (C.byref(frontier),)
    L.check(getattr(lib, call)(snapshot.h, *args, C.byref(p), C.byref(n), *tail))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n.value,)).copy() if n.value \
            else np.zeros(0, dtype=np.uint32)
    finally:
        lib.ketogpu_free(p)


def host_lookup(snapshot, target, type_id=TYPE_ANY):
    """ketogpu_snapshot_lookup: ascending node ids (uint32).  No GPU."""
    return _host_ids(snapshot, "ketogpu_snapshot_lookup", int(target), int(type_id))


def _host_ids_depth(snapshot, call, x, filter_id, max_depth):
    """one ketogpu_snapshot_*_depth call -> (ascending ids (uint32), frontier)"""
    fr = C.c_uint64()
    return _host_ids(snapshot, call, int(x), int(filter_id), int(max_depth), frontier=fr), fr.value


def host_lookup_depth(snapshot, target, max_depth, type_id=TYPE_ANY):
    """ketogpu_snapshot_lookup_depth: (host_lookup within max_depth hops, frontier).  No GPU."""
    return _host_ids_depth(snapshot, "ketogpu_snapshot_lookup_depth", target, type_id, max_depth)


def resolve_subjects(snapshot, subjects):
    """subjects (SubjectID / SubjectSet / their dict forms) -> target node ids (NODE_NONE for a
    subject no tuple names)"""
    if not len(subjects):
        return np.zeros(0, dtype=np.uint32)
    # the root side of the requests is unused: a concrete query that resolves without error
    cols = persistence.request_columns([("-", "-", "-", s) for s in subjects])
    _, targets, status = snapshot.resolve_batch(cols)
    if (status == L.EINVAL).any():
        raise L.KetoError(L.EINVAL, "subject is not allowed to be nil")
    return targets.copy()


def host_path(snapshot, root, target):
    """ketogpu_snapshot_path: the node ids (uint32) of one path root ... target with the fewest
    hops, empty when the check is denied.  No GPU."""
    return _host_ids(snapshot, "ketogpu_snapshot_path", int(root), int(target))


class _Paths:
    """"why is this check allowed?" over self.path_ids_raw and self.snapshot (DESIGN.md
    "Explain")"""

    def path_ids(self, roots, targets):
        """-> one uint32 array per pair: the node ids root ... target of a path with the fewest
        hops, empty for a denied pair.  The first call uses 8 ids per pair; only the pairs whose
        paths were truncated are issued again, with capacity = what they need.  An id outside
        the snapshot raises EINVAL."""
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        return _all_lists(lambda idx, cap: self.path_ids_raw(roots[idx], targets[idx], cap), len(roots),
                          8 * len(roots), False,
                          lambda k: f"pair ({int(roots[k])}, {int(targets[k])}) is outside the snapshot")

    def explain_batch(self, tuples):
        """tuples: (namespace, object, relation, subject) -> per tuple the path that allows the
        check, as the subjects its nodes stand for: the SubjectSet namespace:object#relation
        first, the subject last, [] when the check is denied.  Each consecutive pair is one hop:
        the later subject is held by the earlier subject set.  Under wildcard rows (R5) a hop
        may stand for a wildcard match rather than a literal tuple.  A wildcard query without a
        snapshot node raises KetoError(EINVAL), as in resolve_roots."""
        tuples = [tuple(t) for t in tuples]
        roots = resolve_roots(self.snapshot, [t[:3] for t in tuples])
        targets = resolve_subjects(self.snapshot, [t[3] for t in tuples])
        return [[self.snapshot.describe(int(v)) for v in ids] for ids in self.path_ids(roots, targets)]

    def Explain(self, namespace, object, relation, subject):
        return self.explain_batch([(namespace, object, relation, subject)])[0]


def _all_lists(raw, n, cap, sort, invalid):
    """every list of n requests over a cursor call: raw(idx, cap) -> (out, begin, count, needed)
    for the requests idx.  Only the requests whose lists were truncated are issued again, with
    capacity = what they need.  sort: ascending lists (a path keeps its order).  An id outside
    the snapshot raises EINVAL with the text invalid(request)."""
    res = [None] * n
    idx = np.arange(n)
    while len(idx):
        out, begin, count, _ = raw(idx, cap)
        if (begin == INVALID).any():
            raise L.KetoError(L.EINVAL, invalid(idx[begin == INVALID][0]))
        done = begin != TRUNCATED
        for k in np.nonzero(done)[0]:
            b, c = int(begin[k]), int(count[k])
            res[idx[k]] = np.sort(out[b:b + c]) if sort else out[b:b + c].copy()
        cap = int(count[~done].sum())  # exactly what the rest needs: nothing is truncated twice
        idx = idx[~done]
    return res


class _Handle:
    """a listing handle of the library over a snapshot: ketogpu_<ABI>_new / _free / _stats_get
    with the structs OPTS and STATS.  A write to a writable snapshot is seen by the next call:
    the handle replays the snapshot's patch log and rewrites the rows the write touched on the
    GPU (refresh_stats() tells how; KETOGPU_LIST_REFRESH=full uploads everything instead)."""

    def __init__(self, snapshot, device=0, state_budget_bytes=0):
        self.L = L.lib()
        self.snapshot = snapshot
        opts = self.OPTS(device, state_budget_bytes)
        h = C.c_void_p()
        L.check(self._abi("new")(snapshot.h, C.byref(opts), C.byref(h)))
        self.h = h

    def _abi(self, call):
        return getattr(self.L, f"ketogpu_{self.ABI}_{call}")

    def close(self):
        if getattr(self, "h", None):
            self._abi("free")(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _stats(self, st, call):
        L.check(self._abi(call)(self.h, C.byref(st)))
        return st.as_dict()

    def stats(self):
        return self._stats(self.STATS(), "stats_get")

    def refresh_stats(self):
        """how the handle followed the snapshot's writes (ketogpu_list_refresh_stats): full
        uploads, patched refreshes, rows patched and moved, words uploaded, the fallbacks"""
        return self._stats(L.ListRefreshStats(), "refresh_stats_get")

    def _ids_raw(self, call, requests, filters, capacity):
        """one cursor call ketogpu_<ABI>_<call>(handle, *request arrays, n, *filters, ...) ->
        (out, begin, count, needed): count[i] exact, begin[i] the offset of list i in out, or
        TRUNCATED / INVALID; capacity 0 only counts"""
        requests = [np.ascontiguousarray(r, dtype=np.uint32) for r in requests]
        n = len(requests[0])
        out = np.empty(max(int(capacity), 1), dtype=np.uint32)
        begin = np.empty(max(n, 1), dtype=np.uint64)
        count = np.empty(max(n, 1), dtype=np.uint64)
        needed = C.c_uint64()
        L.check(self._abi(call)(self.h, *[r.ctypes.data for r in requests], n, *filters,
                                out.ctypes.data if capacity else None, int(capacity), begin.ctypes.data,
                                count.ctypes.data, C.byref(needed)))
        return out[:int(capacity)], begin[:n], count[:n], needed.value

    def _page_raw(self, requests, from_ids, filter_id, limit, wide=False):
        """one ketogpu_<ABI>_page call -> (out[n, limit], returned, count, remaining): row i
        holds the returned[i] smallest members >= from_ids[i], ascending; count[i] the whole
        list's size; returned[i] PAGE_INVALID for an id outside the snapshot.  wide: one
        ketogpu_<ABI>_page_wide call without a depth limit, the same results"""
        if wide:
            return self._page_depth_raw(requests, None, from_ids, filter_id, limit, wide=True)[:4]
        requests, lo, n, limit, out, returned, count, remaining = _page_args(requests, from_ids, limit)
        L.check(self._abi("page")(self.h, requests.ctypes.data, None if lo is None else lo.ctypes.data, n,
                                  int(filter_id), limit, out.ctypes.data, returned.ctypes.data, count.ctypes.data,
                                  remaining.ctypes.data))
        return out[:n], returned[:n], count[:n], remaining[:n]

    # ---- depth-limited listings
    def depth_stats(self):
        return self._stats(L.DepthStats(), "depth_stats_get")

    def _ids_depth_raw(self, requests, max_depth, filter_id=TYPE_ANY, capacity=0, wide=False):
        """one ketogpu_<ABI>_ids_depth call -> (out, begin, count, frontier, needed): _ids_raw's
        results within max_depth hops (None: no limit; one number for all requests, or one per
        request), and frontier[i], the interior members at exactly that distance.  wide: one
        ketogpu_<ABI>_ids_depth_wide call, the same results"""
        requests = np.ascontiguousarray(requests, dtype=np.uint32)
        n = len(requests)
        depth = depth_array(max_depth, n)
        out = np.empty(max(int(capacity), 1), dtype=np.uint32)
        begin = np.empty(max(n, 1), dtype=np.uint64)
        count = np.empty(max(n, 1), dtype=np.uint64)
        frontier = np.zeros(max(n, 1), dtype=np.uint64)
        needed = C.c_uint64()
        call = self._abi("ids_depth_wide" if wide else "ids_depth")
        L.check(call(self.h, requests.ctypes.data, None if depth is None else depth.ctypes.data, n, int(filter_id),
                     out.ctypes.data if capacity else None, int(capacity), begin.ctypes.data, count.ctypes.data,
                     frontier.ctypes.data, C.byref(needed)))
        return out[:int(capacity)], begin[:n], count[:n], frontier[:n], needed.value

    def _page_depth_raw(self, requests, max_depth, from_ids=None, filter_id=TYPE_ANY, limit=100, wide=False):
        """one ketogpu_<ABI>_page_depth call -> (out[n, limit], returned, count, remaining,
        frontier): _page_raw's results within max_depth hops.  wide: one ketogpu_<ABI>_page_wide
        call, the same results"""
        requests, lo, n, limit, out, returned, count, remaining = _page_args(requests, from_ids, limit)
        depth = depth_array(max_depth, n)
        frontier = np.zeros(max(n, 1), dtype=np.uint64)
        call = self._abi("page_wide" if wide else "page_depth")
        L.check(call(self.h, requests.ctypes.data, None if depth is None else depth.ctypes.data,
                     None if lo is None else lo.ctypes.data, n, int(filter_id), limit, out.ctypes.data,
                     returned.ctypes.data, count.ctypes.data, remaining.ctypes.data, frontier.ctypes.data))
        return out[:n], returned[:n], count[:n], remaining[:n], frontier[:n]

    # ---- listings that say why
    def via_stats(self):
        return self._stats(L.ViaStats(), "via_stats_get")

    def _ids_via_raw(self, requests, max_depth, filter_id=TYPE_ANY, capacity=0, want_via=True, want_hops=True):
        """one ketogpu_<ABI>_ids_via call -> (out, via, hops, begin, count, frontier, needed):
        _ids_depth_raw's results with via[k] and hops[k] belonging to out[k].  want_via /
        want_hops False: that array is passed as NULL and comes back as None"""
        requests = np.ascontiguousarray(requests, dtype=np.uint32)
        n = len(requests)
        depth = depth_array(max_depth, n)
        cap = int(capacity)
        out = np.empty(max(cap, 1), dtype=np.uint32)
        via = np.empty(max(cap, 1), dtype=np.uint32) if want_via else None
        hops = np.empty(max(cap, 1), dtype=np.uint32) if want_hops else None
        begin = np.empty(max(n, 1), dtype=np.uint64)
        count = np.empty(max(n, 1), dtype=np.uint64)
        frontier = np.zeros(max(n, 1), dtype=np.uint64)
        needed = C.c_uint64()
        ptr = lambda a: a.ctypes.data if cap and a is not None else None
        L.check(self._abi("ids_via")(self.h, requests.ctypes.data, None if depth is None else depth.ctypes.data, n,
                                     int(filter_id), ptr(out), ptr(via), ptr(hops), cap, begin.ctypes.data,
                                     count.ctypes.data, frontier.ctypes.data, C.byref(needed)))
        cut = lambda a: None if a is None else a[:cap]
        return out[:cap], cut(via), cut(hops), begin[:n], count[:n], frontier[:n], needed.value

    def _page_via_raw(self, requests, max_depth, from_ids=None, filter_id=TYPE_ANY, limit=100):
        """one ketogpu_<ABI>_page_via call -> (out[n, limit], via[n, limit], hops[n, limit],
        returned, count, remaining, frontier): _page_depth_raw's results with via and hops at the
        same stride, valid for the first returned[i] entries of row i"""
        requests, lo, n, limit, out, returned, count, remaining = _page_args(requests, from_ids, limit)
        depth = depth_array(max_depth, n)
        via, hops = np.empty_like(out), np.empty_like(out)
        frontier = np.zeros(max(n, 1), dtype=np.uint64)
        L.check(self._abi("page_via")(self.h, requests.ctypes.data, None if depth is None else depth.ctypes.data,
                                      None if lo is None else lo.ctypes.data, n, int(filter_id), limit,
                                      out.ctypes.data, via.ctypes.data, hops.ctypes.data, returned.ctypes.data,
                                      count.ctypes.data, remaining.ctypes.data, frontier.ctypes.data))
        return out[:n], via[:n], hops[:n], returned[:n], count[:n], remaining[:n], frontier[:n]

    # ---- combined listings
    def combine_stats(self):
        return self._stats(L.CombineStats(), "combine_stats_get")

    def combine_ids_raw(self, a, b, op, filter_id=TYPE_ANY, capacity=0):
        """one ketogpu_<ABI>_combine call -> (out, begin, count, needed) as _ids_raw returns them,
        one list per pair (a[i], b[i]); filter_id: the handle's type / class filter"""
        a, b = _pair_args(a, b)
        return self._ids_raw("combine", [a, b], [op_id(op), int(filter_id)], capacity)

    def combine_page_raw(self, a, b, op, from_ids=None, filter_id=TYPE_ANY, limit=100):
        """one ketogpu_<ABI>_combine_page call -> (out[n, limit], returned, count, remaining) as
        _page_raw returns them, one page per pair (a[i], b[i])"""
        a, b = _pair_args(a, b)
        a, lo, n, limit, out, returned, count, remaining = _page_args(a, from_ids, limit)
        L.check(self._abi("combine_page")(self.h, a.ctypes.data, b.ctypes.data, None if lo is None else lo.ctypes.data,
                                          n, op_id(op), int(filter_id), limit, out.ctypes.data, returned.ctypes.data,
                                          count.ctypes.data, remaining.ctypes.data))
        return out[:n], returned[:n], count[:n], remaining[:n]


def _no_wide_with(wide, max_depth, with_via):
    """wide=True lists whole closures (ketogpu_*_ids_wide): there is no wide depth or via call"""
    if wide and (max_depth is not None or with_via):
        raise ValueError("wide=True takes neither max_depth nor with_via")


class _ObjectLists:
    """the full object lists over self.lookup_ids_raw and self.snapshot.  wide: the device
    handle runs large closures in the wide tier (DESIGN.md "Chip-wide closures"); the CPU twin
    accepts and ignores it"""

    def lookup_ids(self, targets, type_id=TYPE_ANY, capacity=None, wide=False):
        """-> one ascending uint32 array per target.  The first call uses `capacity` ids
        (default 64 per target); only the targets whose lists were truncated are issued
        again, with capacity = what they need.  An id outside the snapshot raises EINVAL."""
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        return _all_lists(lambda idx, cap: self.lookup_ids_raw(targets[idx], type_id, cap, wide=wide), len(targets),
                          64 * len(targets) if capacity is None else int(capacity), True,
                          lambda k: f"target {int(targets[k])} is outside the snapshot")

    def _objects(self, ids):
        return sorted(self.snapshot.node_info(int(v))["id"] for v in ids)

    def list_objects_batch(self, namespace, relation, subjects, max_depth=None, with_via=False, wide=False):
        """per subject: the sorted object names o with Check(namespace:o#relation@subject); with
        max_depth, those within that many hops (list_objects_depth_batch's lists); with_via:
        (name, via, hops) instead of names (list_objects_via_batch)"""
        _no_wide_with(wide, max_depth, with_via)
        if with_via:
            return self.list_objects_via_batch(namespace, relation, subjects, max_depth)
        if max_depth is not None:
            return self.list_objects_depth_batch(namespace, relation, subjects, max_depth)[0]
        ty = self.snapshot.type_id(namespace, relation)
        targets = resolve_subjects(self.snapshot, list(subjects))
        if ty == TYPE_NONE:  # unknown namespace or unused pair: nothing (check answers false there)
            return [[] for _ in targets]
        return [self._objects(ids) for ids in self.lookup_ids(targets, ty, wide=wide)]

    def ListObjects(self, namespace, relation, subject, max_depth=None, with_via=False, wide=False):
        return self.list_objects_batch(namespace, relation, [subject], max_depth, with_via, wide)[0]


class _SubjectLists:
    """the full subject lists over self.subject_ids_raw and self.snapshot; wide as in _ObjectLists"""

    def subject_ids(self, roots, cls=TYPE_ANY, capacity=None, wide=False):
        """-> one ascending uint32 array per root.  The first call uses `capacity` ids (default
        64 per root); only the roots whose lists were truncated are issued again, with
        capacity = what they need.  An id outside the snapshot raises EINVAL."""
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        return _all_lists(lambda idx, cap: self.subject_ids_raw(roots[idx], cls, cap, wide=wide), len(roots),
                          64 * len(roots) if capacity is None else int(capacity), True,
                          lambda k: f"root {int(roots[k])} is outside the snapshot")

    def list_subjects_batch(self, roots, kind="ids", max_depth=None, with_via=False, wide=False):
        """per (namespace, object, relation) root: the subjects s with Check(root@s), SubjectIDs
        then SubjectSets, each sorted.  kind: "ids" (subject ids only), "any", or a
        (namespace, relation) pair (subject sets of that type; an unknown pair lists nothing).
        With max_depth: those within that many hops (list_subjects_depth_batch's lists); with_via:
        (subject, via, hops) instead of subjects (list_subjects_via_batch)"""
        _no_wide_with(wide, max_depth, with_via)
        if with_via:
            return self.list_subjects_via_batch(roots, kind, max_depth)
        if max_depth is not None:
            return self.list_subjects_depth_batch(roots, max_depth, kind)[0]
        roots = list(roots)
        cls = _class_of_kind(self.snapshot, kind)
        ids = resolve_roots(self.snapshot, roots)
        if cls == TYPE_NONE:
            return [[] for _ in roots]
        return [_subjects_of(self.snapshot, v) for v in self.subject_ids(ids, cls, wide=wide)]

    def ListSubjects(self, namespace, object, relation, kind="ids", max_depth=None, with_via=False, wide=False):
        return self.list_subjects_batch([(namespace, object, relation)], kind, max_depth, with_via, wide)[0]


class Lookup(_Handle, _ObjectPages, _Paths, _ObjectsCombined, _ObjectsDepth, _ObjectsVia, _ObjectLists):
    """device handle over a snapshot's reverse rows"""
    ABI, OPTS, STATS = "lookup", L.LookupOpts, L.LookupStats

    def lookup_via_raw(self, targets, max_depth=None, type_id=TYPE_ANY, capacity=0, **want):
        """one ketogpu_lookup_ids_via call (_ids_via_raw)"""
        return self._ids_via_raw(targets, max_depth, type_id, capacity, **want)

    def lookup_via_page_raw(self, targets, max_depth=None, from_ids=None, type_id=TYPE_ANY, limit=100):
        """one ketogpu_lookup_page_via call (_page_via_raw)"""
        return self._page_via_raw(targets, max_depth, from_ids, type_id, limit)

    def lookup_depth_raw(self, targets, max_depth, type_id=TYPE_ANY, capacity=0, wide=False):
        """one ketogpu_lookup_ids_depth call (_ids_depth_raw); wide: ketogpu_lookup_ids_depth_wide"""
        return self._ids_depth_raw(targets, max_depth, type_id, capacity, wide=wide)

    def lookup_depth_page_raw(self, targets, max_depth, from_ids=None, type_id=TYPE_ANY, limit=100, wide=False):
        """one ketogpu_lookup_page_depth call (_page_depth_raw); wide: ketogpu_lookup_page_wide"""
        return self._page_depth_raw(targets, max_depth, from_ids, type_id, limit, wide=wide)

    def lookup_ids_raw(self, targets, type_id=TYPE_ANY, capacity=0, wide=False):
        """one ketogpu_lookup_ids call (_ids_raw); wide: one ketogpu_lookup_ids_wide call, the
        same results with the large closures spread over the whole device"""
        return self._ids_raw("ids_wide" if wide else "ids", [targets], [int(type_id)], capacity)

    def wide_stats(self):
        return self._stats(L.WideStats(), "wide_stats_get")

    def path_stats(self):
        return self._stats(L.LookupPathStats(), "path_stats_get")

    def path_ids_raw(self, roots, targets, capacity=0):
        """one ketogpu_lookup_paths call -> (out, begin, count, needed): count[i] the exact
        number of nodes on path i (0: denied), begin[i] its offset in out, or TRUNCATED /
        INVALID; capacity 0 only counts"""
        if len(targets) != len(roots):
            raise L.KetoError(L.EINVAL, "one target per root")
        return self._ids_raw("paths", [roots, targets], [], capacity)

    def lookup_page_raw(self, targets, from_ids=None, type_id=TYPE_ANY, limit=100, wide=False):
        """one ketogpu_lookup_page call (_page_raw); wide: ketogpu_lookup_page_wide without a limit"""
        return self._page_raw(targets, from_ids, type_id, limit, wide=wide)


def host_list_objects(snapshot, namespace, relation, subject):
    """ListObjects on the CPU (host_lookup)"""
    ty = snapshot.type_id(namespace, relation)
    t = int(resolve_subjects(snapshot, [subject])[0])
    if ty == TYPE_NONE or t == L.NODE_NONE:
        return []
    return sorted(snapshot.node_info(int(v))["id"] for v in host_lookup(snapshot, t, ty))


class HostLookup(_ObjectPages, _Paths, _HostCombine, _ObjectsCombined, _HostDepth, _ObjectsDepth, _HostVia,
                 _ObjectsVia, _ObjectLists):
    """Lookup's full-list, paged, path, combined, depth and via calls on the CPU: host_lookup's
    ascending lists, whole, sliced or combined, host_path's paths laid out as the device call lays
    them out, host_lookup_depth's lists and host_lookup_via's"""

    def __init__(self, snapshot):
        self.snapshot = snapshot

    def lookup_ids_raw(self, targets, type_id=TYPE_ANY, capacity=0, wide=False):
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        return _host_cursor([self._members(int(t), type_id) for t in targets], capacity)

    def _via_members(self, x, k, type_id):
        return host_lookup_via(self.snapshot, x, k, type_id)

    def lookup_via_raw(self, targets, max_depth=None, type_id=TYPE_ANY, capacity=0):
        return self._ids_via_raw(targets, max_depth, type_id, capacity)

    def lookup_via_page_raw(self, targets, max_depth=None, from_ids=None, type_id=TYPE_ANY, limit=100):
        return self._page_via_raw(targets, max_depth, from_ids, type_id, limit)

    def _depth_members(self, x, k, type_id):
        if x == L.NODE_NONE:
            return np.zeros(0, dtype=np.uint32), 0
        return host_lookup_depth(self.snapshot, x, k, type_id)

    def lookup_depth_raw(self, targets, max_depth, type_id=TYPE_ANY, capacity=0, wide=False):
        return self._ids_depth_raw(targets, max_depth, type_id, capacity)

    def lookup_depth_page_raw(self, targets, max_depth, from_ids=None, type_id=TYPE_ANY, limit=100, wide=False):
        return self._page_depth_raw(targets, max_depth, from_ids, type_id, limit)

    def _members(self, x, type_id):
        return self._side(x, type_id, host_lookup)

    def path_ids_raw(self, roots, targets, capacity=0):
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        n = len(roots)
        if len(targets) != n:
            raise L.KetoError(L.EINVAL, "one target per root")
        n_nodes = self.snapshot.stats()["num_nodes"]
        out = np.zeros(int(capacity), dtype=np.uint32)
        begin, count = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        cursor = 0
        for i, (r, t) in enumerate(zip(roots, targets)):
            if any(v >= n_nodes and v != L.NODE_NONE for v in (r, t)):
                begin[i] = INVALID
                continue
            ids = host_path(self.snapshot, int(r), int(t))
            count[i] = len(ids)
            if not len(ids):
                continue
            if cursor + len(ids) <= capacity:
                out[cursor:cursor + len(ids)] = ids
                begin[i] = cursor
            else:
                begin[i] = TRUNCATED
            cursor += len(ids)  # every path reserves, written or not
        return out, begin, count, cursor

    def lookup_page_raw(self, targets, from_ids=None, type_id=TYPE_ANY, limit=100, wide=False):
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        n_nodes = self.snapshot.stats()["num_nodes"]
        invalid = [t >= n_nodes and t != L.NODE_NONE for t in targets]
        lists = [None if bad else host_lookup(self.snapshot, int(t), type_id) for t, bad in zip(targets, invalid)]
        return _host_pages(lists, invalid, from_ids, limit)


def host_subjects(snapshot, root, cls=TYPE_ANY):
    """ketogpu_snapshot_subjects: ascending node ids (uint32).  No GPU."""
    return _host_ids(snapshot, "ketogpu_snapshot_subjects", int(root), int(cls))


def host_subjects_depth(snapshot, root, max_depth, cls=TYPE_ANY):
    """ketogpu_snapshot_subjects_depth: (host_subjects within max_depth hops, frontier).  No GPU."""
    return _host_ids_depth(snapshot, "ketogpu_snapshot_subjects_depth", root, cls, max_depth)


def resolve_roots(snapshot, objects):
    """(namespace, object, relation) triples -> root node ids (NODE_NONE for an unknown
    namespace or a query no tuple matches).  A wildcard query without a snapshot node (a
    dynamic root) cannot be listed and raises KetoError(EINVAL)."""
    if not len(objects):
        return np.zeros(0, dtype=np.uint32)
    # the subject side of the requests is unused: any non-nil subject resolves without error
    cols = persistence.request_columns([(ns, obj, rel, {"subject_id": "-"}) for ns, obj, rel in objects])
    roots, _, status = snapshot.resolve_batch(cols)
    if (status == L.ENOTFOUND).any():
        ns, obj, rel = objects[int(np.nonzero(status == L.ENOTFOUND)[0][0])]
        raise L.KetoError(L.EINVAL, f"{ns}:{obj}#{rel} is a wildcard query without a node: its subjects cannot be "
                                    "listed")
    return roots.copy()


def _class_of_kind(snapshot, kind):
    """kind "ids" / "any" / (namespace, relation) -> class filter"""
    if isinstance(kind, str):
        if kind == "ids":
            return CLASS_SUBJECT_ID
        if kind == "any":
            return TYPE_ANY
        raise ValueError(f"kind {kind!r}: expected 'ids', 'any' or a (namespace, relation) pair")
    namespace, relation = kind
    return snapshot.type_id(namespace, relation)  # TYPE_NONE for a pair without a type id: nothing


def _subjects_of(snapshot, ids):
    """node ids -> SubjectIDs, then SubjectSets, each sorted"""
    subs = [snapshot.describe(int(v)) for v in ids]
    users = sorted((s for s in subs if isinstance(s, SubjectID)), key=lambda s: s.id)
    sets = sorted((s for s in subs if isinstance(s, SubjectSet)), key=lambda s: (s.namespace, s.object, s.relation))
    return users + sets


class Subjects(_Handle, _SubjectPages, _SubjectsCombined, _SubjectsDepth, _SubjectsVia, _SubjectLists):
    """device handle over a snapshot's forward rows"""
    ABI, OPTS, STATS = "subjects", L.SubjectsOpts, L.SubjectsStats

    def subject_via_raw(self, roots, max_depth=None, cls=TYPE_ANY, capacity=0, **want):
        """one ketogpu_subjects_ids_via call (_ids_via_raw)"""
        return self._ids_via_raw(roots, max_depth, cls, capacity, **want)

    def subject_via_page_raw(self, roots, max_depth=None, from_ids=None, cls=TYPE_ANY, limit=100):
        """one ketogpu_subjects_page_via call (_page_via_raw)"""
        return self._page_via_raw(roots, max_depth, from_ids, cls, limit)

    def subject_depth_raw(self, roots, max_depth, cls=TYPE_ANY, capacity=0, wide=False):
        """one ketogpu_subjects_ids_depth call (_ids_depth_raw); wide: ketogpu_subjects_ids_depth_wide"""
        return self._ids_depth_raw(roots, max_depth, cls, capacity, wide=wide)

    def subject_depth_page_raw(self, roots, max_depth, from_ids=None, cls=TYPE_ANY, limit=100, wide=False):
        """one ketogpu_subjects_page_depth call (_page_depth_raw); wide: ketogpu_subjects_page_wide"""
        return self._page_depth_raw(roots, max_depth, from_ids, cls, limit, wide=wide)

    def subject_ids_raw(self, roots, cls=TYPE_ANY, capacity=0, wide=False):
        """one ketogpu_subjects_ids call (_ids_raw); wide: one ketogpu_subjects_ids_wide call, the
        same results with the large closures spread over the whole device"""
        return self._ids_raw("ids_wide" if wide else "ids", [roots], [int(cls)], capacity)

    def wide_stats(self):
        return self._stats(L.WideStats(), "wide_stats_get")

    def subject_page_raw(self, roots, from_ids=None, cls=TYPE_ANY, limit=100, wide=False):
        """one ketogpu_subjects_page call (_page_raw); wide: ketogpu_subjects_page_wide without a limit"""
        return self._page_raw(roots, from_ids, cls, limit, wide=wide)


class HostSubjects(_SubjectPages, _HostCombine, _SubjectsCombined, _HostDepth, _SubjectsDepth, _HostVia,
                   _SubjectsVia, _SubjectLists):
    """Subjects' full-list, paged, combined, depth and via calls on the CPU: host_subjects'
    ascending lists, whole, sliced or combined, host_subjects_depth's lists and host_subjects_via's"""

    def __init__(self, snapshot):
        self.snapshot = snapshot

    def subject_ids_raw(self, roots, cls=TYPE_ANY, capacity=0, wide=False):
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        return _host_cursor([self._members(int(r), cls) for r in roots], capacity)

    def _via_members(self, x, k, cls):
        return host_subjects_via(self.snapshot, x, k, cls)

    def subject_via_raw(self, roots, max_depth=None, cls=TYPE_ANY, capacity=0):
        return self._ids_via_raw(roots, max_depth, cls, capacity)

    def subject_via_page_raw(self, roots, max_depth=None, from_ids=None, cls=TYPE_ANY, limit=100):
        return self._page_via_raw(roots, max_depth, from_ids, cls, limit)

    def _depth_members(self, x, k, cls):
        if x == L.NODE_NONE:
            return np.zeros(0, dtype=np.uint32), 0
        return host_subjects_depth(self.snapshot, x, k, cls)

    def subject_depth_raw(self, roots, max_depth, cls=TYPE_ANY, capacity=0, wide=False):
        return self._ids_depth_raw(roots, max_depth, cls, capacity)

    def subject_depth_page_raw(self, roots, max_depth, from_ids=None, cls=TYPE_ANY, limit=100, wide=False):
        return self._page_depth_raw(roots, max_depth, from_ids, cls, limit)

    def _members(self, x, cls):
        return self._side(x, cls, host_subjects)

    def subject_page_raw(self, roots, from_ids=None, cls=TYPE_ANY, limit=100, wide=False):
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        n_nodes = self.snapshot.stats()["num_nodes"]
        invalid = [r >= n_nodes and r != L.NODE_NONE for r in roots]
        lists = [None if bad else host_subjects(self.snapshot, int(r), cls) for r, bad in zip(roots, invalid)]
        return _host_pages(lists, invalid, from_ids, limit)


def host_list_subjects(snapshot, namespace, object, relation, kind="ids"):
    """ListSubjects on the CPU (host_subjects)"""
    cls = _class_of_kind(snapshot, kind)
    r = int(resolve_roots(snapshot, [(namespace, object, relation)])[0])
    if cls == TYPE_NONE or r == L.NODE_NONE:
        return []
    return _subjects_of(snapshot, host_subjects(snapshot, r, cls))


__all__ = ["Lookup", "host_lookup", "host_list_objects", "resolve_subjects", "Subjects", "host_subjects",
           "host_list_subjects", "resolve_roots", "TYPE_ANY", "TYPE_NONE", "CLASS_SUBJECT_ID", "CLASS_UNTYPED_SET",
           "TRUNCATED", "INVALID", "SubjectID", "SubjectSet", "HostLookup", "HostSubjects", "PAGE_LIMIT_MAX",
           "PAGE_INVALID", "parse_page_token", "check_page_size", "next_page_token", "host_path", "OP_AND", "OP_ANDNOT",
           "OP_OR", "op_id", "DEPTH_ALL", "host_lookup_depth", "host_subjects_depth", "depth_array", "host_lookup_via",
           "host_subjects_via", "grant_chain"]
