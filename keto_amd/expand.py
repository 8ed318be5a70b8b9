"""expand.Engine — BuildTree over the snapshot, and the expand.Tree model.

Mirrors internal/expand/engine.go:30-98 (BuildTree) and internal/expand/tree.go
(NodeType, Tree, JSON codec :85-91,156-162).  BuildTree's output order depends on
the backend's row order: children keep it, and one visited map covers the whole tree.

Engine is the host: ketogpu_expand, one tree per call with strings, and its twin
ketogpu_snapshot_expand_ids, the same walk over a root that is a snapshot node, giving the
tree as two preorder arrays (node ids and child counts).  DeviceEngine answers batches with
ketogpu_subjects_expand, an ordered depth-first walk on the GPU that writes the same arrays
(csrc/expand_tree.hpp), or with wide=True with ketogpu_subjects_expand_wide, the same walk with
the copying of its leaf runs spread over the GPU (csrc/expand_wide.hpp).  Subjects that are no snapshot node (dynamic wildcard queries,
unknown names) and requests the device hands back (status HOST: a query with an
unknown-namespace row was met, or the snapshot has shared Subject.String() keys) go through
Engine, so every answer, errors included, is Engine.BuildTree's.
"""
import ctypes as C
import json

import numpy as np
from dataclasses import dataclass, field
from typing import List, Optional

from . import _lib as L
from .relationtuple import Subject, SubjectID, SubjectSet
from .snapshot import Snapshot, subject_struct

Union, Exclusion, Intersection, Leaf = "union", "exclusion", "intersection", "leaf"



def _depth32(d):
    """restDepth for the uint32 argument of the id calls: <= 0 is the nil tree (0), and every
    depth from INT32_MAX on is no limit, as _depth's clamp makes it for ketogpu_expand"""
    d = int(d)
    return 0 if d <= 0 else L.EXPAND_DEPTH_ALL if d >= 2**31 - 1 else d


def _depth(d):
    """restDepth for the int32 argument of ketogpu_expand: every depth <= 0 is the nil
    tree and every depth beyond INT32_MAX exceeds any tree's height, so clamping keeps
    BuildTree's answer (ctypes would silently truncate a wider Go int)"""
    return max(-1, min(int(d), 2**31 - 1))

class NotFound(LookupError):
    """herodot.ErrNotFound (HTTP 404)"""


@dataclass
class Tree:
    type: str
    subject: Subject
    children: List["Tree"] = field(default_factory=list)

    def to_node(self):
        """the JSON `node` of tree.go:85-91 (children omitempty)"""
        d = {"type": self.type}
        if self.children:
            d["children"] = [c.to_node() for c in self.children]
        d.update(self.subject.to_dict())
        return d

    def MarshalJSON(self) -> str:
        return json.dumps(self.to_node(), separators=(",", ":"))


def _subject(s: L.Subject) -> Subject:
    if s.kind == L.SUBJECT_ID:
        return SubjectID(s.id.decode("utf-8"))
    return SubjectSet(s.ns.decode("utf-8"), s.obj.decode("utf-8"), s.rel.decode("utf-8"))


def _take_ids(lib, nodes, kids, n):
    """the malloc'ed arrays of ketogpu_snapshot_expand_ids as numpy copies, freed"""
    try:
        k = int(n.value)
        if not k:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        a = np.ctypeslib.as_array(C.cast(nodes, C.POINTER(C.c_uint32)), (k,)).copy()
        b = np.ctypeslib.as_array(C.cast(kids, C.POINTER(C.c_uint32)), (k,)).copy()
        return a, b
    finally:
        if nodes.value:
            lib.ketogpu_free(nodes)
        if kids.value:
            lib.ketogpu_free(kids)


class _IdTrees:
    """trees from id arrays, shared by the engines.  Node ids are decoded once per distinct id
    (ketogpu_snapshot_node) and kept for the life of the engine's snapshot version."""

    def _names(self):
        """node id -> Subject, filled on demand; dropped when an in-place write moved the version"""
        v = self.snapshot.version()
        if getattr(self, "_names_version", None) != v:
            self._names_cache, self._names_version = {}, v
        return self._names_cache

    def tree_from_ids(self, nodes, num_children) -> Optional[Tree]:
        """the Tree of two preorder arrays (None for empty ones)"""
        if not len(nodes):
            return None
        names, describe = self._names(), self.snapshot.describe

        def subject(u):
            s = names.get(u)
            if s is None:
                s = names[u] = describe(u)
            return s

        nodes, kids = [int(x) for x in nodes], [int(x) for x in num_children]
        root = Tree(Union if kids[0] else Leaf, subject(nodes[0]))
        stack = [(root, kids[0])] if kids[0] else []
        for u, k in zip(nodes[1:], kids[1:]):
            t = Tree(Union if k else Leaf, subject(u))
            parent, left = stack[-1]
            parent.children.append(t)
            if left == 1:
                stack.pop()
            else:
                stack[-1] = (parent, left - 1)
            if k:
                stack.append((t, k))
        return root

    def json_from_ids(self, nodes, num_children) -> str:
        """the library's MarshalJSON of two preorder arrays (ketogpu_tree_from_ids, then
        ketogpu_tree_json): what a cgo caller does with a device answer"""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        kids = np.ascontiguousarray(num_children, dtype=np.uint32)
        h = C.c_void_p()
        L.check(self.L.ketogpu_tree_from_ids(self.snapshot.h, nodes.ctypes.data, kids.ctypes.data, len(nodes),
                                             C.byref(h)))
        out = C.c_void_p()
        try:
            L.check(self.L.ketogpu_tree_json(h if h.value else None, C.byref(out)))
            s = C.string_at(out.value).decode("utf-8")
            self.L.ketogpu_free(out)
            return s
        finally:
            if h.value:
                self.L.ketogpu_tree_free(h)

    def _resolve(self, subjects):
        from .lookup import resolve_subjects
        return resolve_subjects(self.snapshot, list(subjects))

    def build_trees_json_batch(self, subjects, depths, wide=False):
        """build_trees_batch as JSON strings ("null" for a nil tree; NotFound stays an object)"""
        return [t if isinstance(t, NotFound) else ("null" if t is None else t.MarshalJSON())
                for t in self.build_trees_batch(subjects, depths, wide=wide)]


class Engine(_IdTrees):
    def __init__(self, snapshot: Snapshot):
        self.L = L.lib()
        self.snapshot = snapshot

    def expand_ids(self, subject_or_node, rest_depth):
        """the host twin, ketogpu_snapshot_expand_ids -> (nodes, num_children, flags): the
        tree of a snapshot node (or of a subject that resolves to one) as two preorder uint32
        arrays, empty for the nil tree; flags & EXPAND_NEEDS_HOST: a query with an
        unknown-namespace row was visited.  NotFound where BuildTree raises it (its .flags
        holds the flags).  KetoError EINVAL for a subject that is no snapshot node."""
        node = subject_or_node
        if not isinstance(node, (int, np.integer)):
            node = int(self._resolve([node])[0])
        nodes, kids, n, flags = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        rc = self.L.ketogpu_snapshot_expand_ids(self.snapshot.h, int(node), _depth32(rest_depth), C.byref(nodes),
                                                C.byref(kids), C.byref(n), C.byref(flags))
        if rc == L.ENOTFOUND:
            e = NotFound(self.L.ketogpu_last_error().decode("utf-8", "replace"))
            e.flags = flags.value
            raise e
        L.check(rc)
        a, b = _take_ids(self.L, nodes, kids, n)
        return a, b, flags.value

    def build_trees_batch(self, subjects, depths, wide=False):
        """BuildTree per (subject, depth) -> a list of Tree | None | NotFound (returned, not
        raised), through the host twin where the subject is a snapshot node.  `wide` is the
        DeviceEngine's choice of call and means nothing here"""
        subjects = list(subjects)
        ids = self._resolve(subjects) if subjects else []
        res = []
        for s, v, d in zip(subjects, ids, depths):
            try:
                if int(v) == L.NODE_NONE:
                    res.append(self.BuildTree(s, d))
                else:
                    a, b, _ = self.expand_ids(int(v), d)
                    res.append(self.tree_from_ids(a, b))
            except NotFound as e:
                res.append(e)
        return res

    def tree_size(self, subject: Subject, rest_depth: int) -> int:
        """number of nodes of BuildTree's tree (0 for a nil tree), built and dropped in C++
        without Python objects (throughput measurements)"""
        h = C.c_void_p()
        subj = subject_struct(subject)
        rc = self.L.ketogpu_expand(self.snapshot.h, C.byref(subj), _depth(rest_depth), C.byref(h))
        if rc == L.ENOTFOUND:
            raise NotFound(self.L.ketogpu_last_error().decode("utf-8", "replace"))
        L.check(rc)
        if not h.value:
            return 0
        try:
            nodes = C.POINTER(L.TreeNode)()
            n = C.c_size_t()
            L.check(self.L.ketogpu_tree_nodes(h, C.byref(nodes), C.byref(n)))
            return int(n.value)
        finally:
            self.L.ketogpu_tree_free(h)

    def BuildTree(self, subject: Subject, rest_depth: int) -> Optional[Tree]:
        h = C.c_void_p()
        subj = subject_struct(subject)
        rc = self.L.ketogpu_expand(self.snapshot.h, C.byref(subj), _depth(rest_depth), C.byref(h))
        if rc == L.ENOTFOUND:
            raise NotFound(self.L.ketogpu_last_error().decode("utf-8", "replace"))
        L.check(rc)
        if not h.value:
            return None
        try:
            nodes = C.POINTER(L.TreeNode)()
            n = C.c_size_t()
            L.check(self.L.ketogpu_tree_nodes(h, C.byref(nodes), C.byref(n)))
            pos = 0

            def take():
                nonlocal pos
                nd = nodes[pos]
                pos += 1
                t = Tree(Leaf if nd.type == L.NODE_LEAF else Union, _subject(nd.subject))
                for _ in range(nd.num_children):
                    t.children.append(take())
                return t

            return take()
        finally:
            self.L.ketogpu_tree_free(h)

    build_tree = BuildTree

    def build_tree_json(self, subject: Subject, rest_depth: int) -> str:
        """the library's own MarshalJSON (ketogpu_tree_json)"""
        h = C.c_void_p()
        subj = subject_struct(subject)
        rc = self.L.ketogpu_expand(self.snapshot.h, C.byref(subj), _depth(rest_depth), C.byref(h))
        if rc == L.ENOTFOUND:
            raise NotFound(self.L.ketogpu_last_error().decode("utf-8", "replace"))
        L.check(rc)
        out = C.c_void_p()
        try:
            L.check(self.L.ketogpu_tree_json(h if h.value else None, C.byref(out)))
            s = C.string_at(out.value).decode("utf-8")
            self.L.ketogpu_free(out)
            return s
        finally:
            if h.value:
                self.L.ketogpu_tree_free(h)


class DeviceEngine(_IdTrees):
    """BuildTree in batches on the GPU: ketogpu_subjects_expand on a lookup.Subjects handle
    (one of its own unless `subjects` is given).  On a snapshot with shared Subject.String()
    keys the handle cannot exist and every request is the host's."""

    def __init__(self, snapshot: Snapshot, subjects=None):
        from . import lookup
        self.L = L.lib()
        self.snapshot = snapshot
        self.host = Engine(snapshot)
        self._own = subjects is None
        if subjects is None:
            try:
                subjects = lookup.Subjects(snapshot)
            except L.KetoError as e:  # shared keys (R4)
                if e.code != L.EINVAL:
                    raise
        self.subjects = subjects

    def close(self):
        if self._own and self.subjects is not None:
            self.subjects.close()
        self.subjects = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def expand_stats(self):
        """ketogpu_expand_stats of the handle ({} without one)"""
        if self.subjects is None:
            return {}
        st = L.ExpandStats()
        L.check(self.L.ketogpu_subjects_expand_stats_get(self.subjects.h, C.byref(st)))
        return st.as_dict()

    def expand_wide_stats(self):
        """ketogpu_expand_wide_stats of the handle ({} without one)"""
        if self.subjects is None:
            return {}
        st = L.ExpandWideStats()
        L.check(self.L.ketogpu_subjects_expand_wide_stats_get(self.subjects.h, C.byref(st)))
        return st.as_dict()

    def expand_ids_raw(self, roots, depths, capacity=0, wide=False, out=None):
        """one ketogpu_subjects_expand call (wide: ketogpu_subjects_expand_wide) -> (nodes,
        num_children, begin, count, status, needed): count[i] the exact size of tree i, begin[i]
        its offset in both arrays or TRUNCATED / INVALID, status[i] EXPAND_OK / _NIL / _HOST;
        capacity 0 only counts.  depths: rest depths as the C call takes them (0 nil,
        EXPAND_DEPTH_ALL no limit).  out=(nodes, num_children): two C-contiguous uint32 arrays of
        at least `capacity` words that the caller keeps; the call writes into them and returns
        views of them instead of fresh arrays (ValueError for any other pair)"""
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        n = len(roots)
        depths = np.ascontiguousarray(np.broadcast_to(np.asarray(depths, dtype=np.uint32), (n,)))
        cap = int(capacity)
        if out is not None:
            try:
                nodes, kids = out
            except (TypeError, ValueError):
                raise ValueError("out: a pair (nodes, num_children) of uint32 arrays")
            for a in (nodes, kids):
                if not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.ndim == 1
                        and a.flags.c_contiguous and a.flags.writeable and len(a) >= cap):
                    raise ValueError("out: two writable C-contiguous uint32 arrays of at least `capacity` words")
            if np.shares_memory(nodes, kids):
                raise ValueError("out: the two arrays overlap")
        else:
            nodes = np.empty(max(cap, 1), dtype=np.uint32)
            kids = np.empty(max(cap, 1), dtype=np.uint32)
        begin = np.zeros(max(n, 1), dtype=np.uint64)
        count = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.full(max(n, 1), L.EXPAND_HOST, dtype=np.uint32)
        needed = C.c_uint64()
        if self.subjects is not None:
            call = self.L.ketogpu_subjects_expand_wide if wide else self.L.ketogpu_subjects_expand
            L.check(call(
                self.subjects.h, roots.ctypes.data, depths.ctypes.data, n, nodes.ctypes.data if cap else None,
                kids.ctypes.data if cap else None, cap, begin.ctypes.data, count.ctypes.data, status.ctypes.data,
                C.byref(needed)))
        return nodes[:cap], kids[:cap], begin[:n], count[:n], status[:n], needed.value

    def expand_ids(self, roots, depths, wide=False):
        """the trees of snapshot nodes: a count-only call, then a call with exactly the room
        -> (trees, status): trees[i] = (nodes, num_children) views, empty for NIL and HOST"""
        *_, needed = self.expand_ids_raw(roots, depths, 0, wide=wide)
        nodes, kids, begin, count, status, _ = self.expand_ids_raw(roots, depths, needed, wide=wide)
        trees = []
        for b, c, st in zip(begin, count, status):
            if st != L.EXPAND_OK or not c:
                trees.append((nodes[:0], kids[:0]))
            else:
                if int(b) in (L.LOOKUP_TRUNCATED, L.LOOKUP_INVALID):
                    raise L.KetoError(L.EINVAL, "expand: a tree grew between the counting call and the writing one")
                trees.append((nodes[int(b):int(b) + int(c)], kids[int(b):int(b) + int(c)]))
        return trees, status

    def _batch(self, subjects, depths, make, wide=False):
        subjects = list(subjects)
        depths = [depths] * len(subjects) if isinstance(depths, (int, np.integer)) else list(depths)
        ids = self._resolve(subjects) if subjects else np.zeros(0, np.uint32)
        on_device = [i for i, v in enumerate(ids) if int(v) != L.NODE_NONE]
        res = [None] * len(subjects)
        host = set(range(len(subjects))) - set(on_device)
        if on_device:
            trees, status = self.expand_ids([ids[i] for i in on_device], [_depth32(depths[i]) for i in on_device],
                                            wide=wide)
            for i, (a, b), st in zip(on_device, trees, status):
                if st == L.EXPAND_HOST:
                    host.add(i)
                elif st == L.EXPAND_OK:
                    res[i] = make(a, b)
        for i in sorted(host):
            try:
                if make == self.tree_from_ids:
                    res[i] = self.host.BuildTree(subjects[i], depths[i])
                else:
                    res[i] = self.host.build_tree_json(subjects[i], depths[i])
            except NotFound as e:
                res[i] = e
        return res

    def build_trees_batch(self, subjects, depths, wide=False):
        """BuildTree per (subject, depth) -> a list of Tree | None | NotFound (returned, not
        raised): one device batch (wide: of the wide call), and the host for what the device
        does not answer"""
        return self._batch(subjects, depths, self.tree_from_ids, wide=wide)

    def build_trees_json_batch(self, subjects, depths, wide=False):
        """build_trees_batch as the library's JSON ("null" for a nil tree)"""
        return ["null" if t is None else t
                for t in self._batch(subjects, depths, self.json_from_ids, wide=wide)]  # (NIL: None)

    def BuildTree(self, subject: Subject, rest_depth: int, wide=False) -> Optional[Tree]:
        t = self.build_trees_batch([subject], [rest_depth], wide=wide)[0]
        if isinstance(t, NotFound):
            raise t
        return t

    build_tree = BuildTree
