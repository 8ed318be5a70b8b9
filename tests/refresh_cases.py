"""The snapshot and the writes of the patch-log and listing-refresh tests (test_patch_log.py,
test_list_refresh_gpu.py): about 30 groups nested three deep, 20 documents and 150 users on a
writable snapshot, and a deterministic series of 60 small writes with new subjects, a row
deleted to empty and filled again, and writes the snapshot must refuse.

Rows are the raw tuples of Snapshot.from_rows: (namespace_id, object, relation, subject_id | None,
ss_namespace_id, ss_object, ss_relation)."""
import random

from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot

NAMESPACES = [("groups", 1), ("docs", 2)]
N_GROUPS, N_DOCS, N_USERS = 30, 20, 150
EMPTIED = "g7"  # the group whose row is deleted to empty (write 10) and filled again (write 12)


def level(i):
    return i % 3  # 0: named by documents, 1: nested in level 0, 2: nested in level 1


def user_row(group, user):
    return (1, group, "member", user, None, None, None)


def nest_row(parent, child):
    return (1, parent, "member", None, 1, child, "member")


def doc_row(doc, group):
    return (2, doc, "viewer", None, 1, group, "member")


def base_rows(seed=11):
    """every group has rows (a write cannot create a group) and is named as a subject by some
    row (a write cannot make a node interior), so later writes may use any of them"""
    rng = random.Random(seed)
    rows = set()
    by_level = {l: [i for i in range(N_GROUPS) if level(i) == l] for l in range(3)}
    for i in range(N_GROUPS):
        for u in rng.sample(range(N_USERS), rng.randrange(2, 7)):
            rows.add(user_row(f"g{i}", f"u{u}"))
        if level(i) > 0:
            rows.add(nest_row(f"g{rng.choice(by_level[level(i) - 1])}", f"g{i}"))
        if level(i) > 0 and rng.random() < 0.3:
            rows.add(nest_row(f"g{rng.choice(by_level[level(i) - 1])}", f"g{i}"))
    for d in range(N_DOCS):
        for g in rng.sample(by_level[0], rng.randrange(1, 4)):
            rows.add(doc_row(f"d{d}", f"g{g}"))
        rows.add((2, f"d{d}", "owner", f"u{rng.randrange(N_USERS)}", None, None, None))
        if rng.random() < 0.4:
            rows.add((2, f"d{d}", "viewer", f"u{rng.randrange(N_USERS)}", None, None, None))
    for k, g in enumerate(by_level[0]):  # every level-0 group is named by a document
        rows.add(doc_row(f"d{k % N_DOCS}", f"g{g}"))
    return sorted(rows, key=repr)


def snapshot(rows, writable=True):
    return Snapshot.from_rows(NAMESPACES, list(rows), writable=writable)


class Writes:
    """write k of the series against the table as it stands: (inserts, deletes, refused), with
    `refused` saying the snapshot must refuse it.  `rows` mirrors the table: applied(k) folds a
    write in after the snapshot took it."""

    COUNT = 60

    def __init__(self, rows, seed=5):
        self.rows = set(rows)
        self.rng = random.Random(seed)
        self.fresh = 0

    def _insert(self):
        rng = self.rng
        for _ in range(20):
            x = rng.random()
            if x < 0.5:
                row = user_row(f"g{rng.randrange(N_GROUPS)}", f"u{rng.randrange(N_USERS)}")
            elif x < 0.7:  # a subject no row names yet: a reserved node id
                self.fresh += 1
                row = user_row(f"g{rng.randrange(N_GROUPS)}", f"new{self.fresh}")
            elif x < 0.8:
                row = (2, f"d{rng.randrange(N_DOCS)}", "viewer", f"u{rng.randrange(N_USERS)}", None, None, None)
            elif x < 0.9:
                row = nest_row(f"g{rng.randrange(N_GROUPS)}", f"g{rng.randrange(N_GROUPS)}")
            else:
                row = doc_row(f"d{rng.randrange(N_DOCS)}", f"g{rng.randrange(N_GROUPS)}")
            if row not in self.rows:
                return row
        raise AssertionError("no row left to insert")

    def write(self, k):
        rng = self.rng
        if k in (6, 33):  # a group no row defines: a new expandable node
            return [user_row(f"brand_new{k}", "u1")], [], True
        if k == 21:  # a document's viewers as a subject: an expandable node would become interior
            return [nest_row("g1", "g2"), (1, "g3", "member", None, 2, "d4", "viewer")], [], True
        if k == 10:
            return [], sorted(r for r in self.rows if r[:3] == (1, EMPTIED, "member")), False
        if k == 12:
            return [user_row(EMPTIED, f"u{u}") for u in (3, 4, 5)] + [user_row(EMPTIED, "refilled")], [], False
        ins, dele = [], []
        for _ in range(rng.randrange(1, 5)):
            if rng.random() < 0.65:
                row = self._insert()
                if row not in ins:
                    ins.append(row)
            else:
                row = rng.choice(sorted(self.rows, key=repr))
                if row[:3] != (1, EMPTIED, "member") and row not in dele:
                    dele.append(row)
        return ins, dele, False

    def applied(self, ins, dele):
        self.rows |= set(ins)
        self.rows -= set(dele)


def node_names():
    """every subject the series can name: (label, subject)"""
    names = [(f"u{u}", rt.SubjectID(f"u{u}")) for u in range(N_USERS)]
    names += [(f"new{k}", rt.SubjectID(f"new{k}")) for k in range(1, 200)] + [("refilled", rt.SubjectID("refilled"))]
    names += [(f"g{i}#member", rt.SubjectSet("groups", f"g{i}", "member")) for i in range(N_GROUPS)]
    for d in range(N_DOCS):
        names += [(f"d{d}#{r}", rt.SubjectSet("docs", f"d{d}", r)) for r in ("viewer", "owner")]
    return names


def node_of(snap, subject):
    """the node id of a subject (NODE_NONE when no row names it)"""
    return snap.resolve("groups", "g0", "member", subject)[1]
