"""The graph and the yardstick of the wide expand tests (test_expand_wide_gpu.py on the device;
test_expand_wide_host.py checks the shapes against the host on the CPU).  The yardstick is
expand_cases.twin applied to ketogpu_subjects_expand_wide, and every wide answer is also compared
with the plain call's.  Rows are raw rows as in expand_cases: a query's rows come in the order of
the subject's object name, so the names fix each row's order."""
import functools

import numpy as np

from keto_amd import _lib as L
from keto_amd import expand
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import expand_cases as EC
from tests.lookup_cases import NS1, sid, sset

ALL = EC.ALL
WINDOW = 64 * 64  # expand_wide.hpp kWindow: the entries one run step can pass
LEAF_ROWS = (4095, 4096, 4097, 8193)
OPEN_AT = (0, 63, 64, 65, 127, 128, 129, 299)
FAN = 10000
RESIDUE_ROWS, RESIDUE_LEN0 = 130, 70


def view(name):
    return rt.SubjectSet("n", name, "view")


def row_with_sets_at(k, at, prefix):
    """expand_cases.row_with_sets_at with names wide enough for rows of thousands"""
    rows = [sset(f"{prefix}r", "view", f"{prefix}x{i:05d}", "member") for i in range(k)]
    rows += [sid(f"{prefix}x{i:05d}", "member", f"{prefix}u{i}") for i in at]
    return rows


def wide_rows():
    """one graph with a part per case of the run step (names do not overlap)"""
    rows = []
    for k in LEAF_ROWS:  # leaf-only rows around the ends of the 64-word window
        rows += row_with_sets_at(k, (), f"WL{k}_")
    for p in OPEN_AT:  # one child that opens in a row of 300: the z >= 64 border, a run that ends the row
        rows += row_with_sets_at(300, (p,), f"WP{p}_")
    rows += row_with_sets_at(300, (100, 110), "WT10_")  # two opening children 10 apart
    rows += row_with_sets_at(300, (50, 250), "WT200_")  # ... and 200 apart
    # [g, 200 leaves, g, 200 leaves] as the row of the wildcard node n:wg_o# (every relation of
    # wg_o, in relation order): the second g is an attention entry that is a leaf between runs
    rows += [sset("wgdup", "view", "wg_o", ""), sid("wg_g", "member", "wg_ug")]
    rows += [sset("wg_o", "a", "wg_g", "member"), sset("wg_o", "c", "wg_g", "member")]
    rows += [sset("wg_o", "b", f"wg_b{i:03d}", "member") for i in range(200)]
    rows += [sset("wg_o", "d", f"wg_d{i:03d}", "member") for i in range(200)]
    # depth marking (expand_cases `dm`) with 200 leaves between a and b: R -> [a, 200 leaves, b],
    # a -> [b], b -> [u]
    rows += [sset("wdm", "view", "wdm_a", "member"), sset("wdm", "view", "wdm_z_b", "member"),
             sset("wdm_a", "member", "wdm_z_b", "member"), sid("wdm_z_b", "member", "wdm_u")]
    rows += [sset("wdm", "view", f"wdm_m{i:03d}", "member") for i in range(200)]
    # a fan of FAN users under a group under a root, with an opening sibling behind the group
    rows += [sset("wfan", "view", "wfan_a_g", "member"), sset("wfan", "view", "wfan_b_s", "member"),
             sid("wfan_b_s", "member", "wfan_us")]
    rows += [sid("wfan_a_g", "member", f"wfan_u{i:05d}") for i in range(FAN)]
    # a leaf whose rows are all bad (an unknown namespace, as randgraph's poison rows), in the
    # middle of a run of 400
    rows += [sset("wbad", "view", f"wbad_x{i:03d}", "member") for i in range(400)]
    rows += [sset("wbad_x200", "member", "wbad_z", "member", sns=98)]
    # RESIDUE_ROWS roots whose row lengths differ by one: packed back to back, their rows begin at
    # many residues modulo 64
    for i in range(RESIDUE_ROWS):
        rows += [sset(f"wres{i:03d}", "view", f"wres_x{j:03d}", "member") for j in range(RESIDUE_LEN0 + i)]
    return rows


@functools.lru_cache(maxsize=None)
def graph():
    return Snapshot.from_rows(NS1, wide_rows())


def root_names():
    names = [f"WL{k}_r" for k in LEAF_ROWS] + [f"WP{p}_r" for p in OPEN_AT] + ["WT10_r", "WT200_r"]
    names += ["wgdup", "wdm", "wfan", "wbad"] + [f"wres{i:03d}" for i in range(RESIDUE_ROWS)]
    return names


def roots(snap):
    return np.array([EC.node_of(snap, view(x)) for x in root_names()], dtype=np.uint32)


def row_begins(ex):
    """-> {node: (begin, length)} of every node that has a row, as a compact handle packs them:
    back to back in node order.  The length of a row is the root's child count at depth 2."""
    out, at = {}, 0
    for v in range(ex.snapshot.stats()["num_expandable"]):
        try:
            _, kids, _ = ex.expand_ids(v, 2)
        except expand.NotFound:  # every row is bad: no row on the device
            continue
        if len(kids) and kids[0]:
            out[v] = (at, int(kids[0]))
            at += int(kids[0])
    return out


def tree_of(arrays, begin, count, i):
    nodes, kids = arrays
    b, c = int(begin[i]), int(count[i])
    return nodes[b:b + c], kids[b:b + c]


def assert_device_wide(dev, ex, roots, depths):
    """expand_cases.assert_device for the wide call: one count-only call and one exact call
    against the twin, word for word in both arrays, status, count, begin and needed exact; then
    the plain call with the same room, whose every answer the wide one equals -> the statuses"""
    roots = np.asarray(roots, dtype=np.uint32)
    depths = np.broadcast_to(np.asarray(depths, dtype=np.uint32), roots.shape)
    want = [EC.twin(ex, r, d) for r, d in zip(roots, depths)]
    total = sum(len(w[1]) for w in want)
    _, _, begin0, count0, status0, needed0 = dev.expand_ids_raw(roots, depths, 0, wide=True)
    nodes, kids, begin, count, status, needed = dev.expand_ids_raw(roots, depths, total, wide=True)
    assert needed0 == needed == total
    for i, (st, wn, wk, invalid) in enumerate(want):
        where = (i, int(roots[i]), int(depths[i]))
        assert status[i] == status0[i] == st, where
        assert count[i] == count0[i] == len(wn), where
        if invalid:
            assert begin[i] == begin0[i] == L.LOOKUP_INVALID, where
        elif len(wn):
            assert begin0[i] == L.LOOKUP_TRUNCATED, where
            b = int(begin[i])
            assert b + len(wn) <= total, where
            assert (nodes[b:b + len(wn)] == wn).all() and (kids[b:b + len(wn)] == wk).all(), where
    pn, pk, pbegin, pcount, pstatus, pneeded = dev.expand_ids_raw(roots, depths, total)
    assert pneeded == needed and (pstatus == status).all() and (pcount == count).all()
    for i, (st, wn, _, invalid) in enumerate(want):
        if invalid or not len(wn):
            assert pbegin[i] == begin[i], i
        else:
            a, b = tree_of((nodes, kids), begin, count, i), tree_of((pn, pk), pbegin, pcount, i)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), i
    return status
