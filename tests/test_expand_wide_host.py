"""The graph of tests/expand_wide_cases.py has the shapes its names promise, by the host walk
alone (no GPU): test_expand_wide_gpu.py runs the wide call over them.  Also what the wide
keyword and the out= arrays owe without a device: the host engine takes and ignores `wide`, and a
bad out= pair is refused before any call is made."""
import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import expand
from tests import expand_cases as EC
from tests import expand_wide_cases as WC


def _tree(ex, name, depth=WC.ALL):
    a, b, flags = ex.expand_ids(EC.node_of(ex.snapshot, WC.view(name)), depth)
    assert flags == 0
    return a, b


def _openers(a, b):
    return [i for i, c in enumerate(EC.children_of_root(a, b)) if b[c]]


def test_shapes():
    snap = WC.graph()
    ex = expand.Engine(snap)
    for k in WC.LEAF_ROWS:
        a, b = _tree(ex, f"WL{k}_r")
        assert len(a) == k + 1 and b[0] == k and not b[1:].any()
    for p in WC.OPEN_AT:
        a, b = _tree(ex, f"WP{p}_r")
        assert _openers(a, b) == [p] and len(a) == 302
    assert _openers(*_tree(ex, "WT10_r")) == [100, 110] and _openers(*_tree(ex, "WT200_r")) == [50, 250]
    # [g, 200 leaves, g, 200 leaves] under the wildcard node: the second g is a leaf
    a, b = _tree(ex, "wgdup")
    g = EC.node_of(snap, EC.member("wg_g"))
    assert len(a) == 405 and list(b[:4]) == [1, 402, 1, 0]
    assert a[2] == a[204] == g and b[204] == 0 and int((a == g).sum()) == 2 and int((b > 0).sum()) == 3
    # depth marking across a run of 200: at depth 3 b is marked at the limit and a leaf twice
    dm_b = EC.node_of(snap, EC.member("wdm_z_b"))
    a, b = _tree(ex, "wdm", 3)
    assert [int(k) for x, k in zip(a, b) if x == dm_b] == [0, 0] and len(a) == 204 and a[203] == dm_b
    a, b = _tree(ex, "wdm", 4)
    assert [int(k) for x, k in zip(a, b) if x == dm_b] == [1, 0] and len(a) == 205 and a[204] == dm_b
    # the fan: root, group, FAN users, then the sibling that opens behind them
    a, b = _tree(ex, "wfan")
    assert len(a) == WC.FAN + 4 and list(b[:2]) == [2, WC.FAN] and not b[2:WC.FAN + 2].any()
    assert a[WC.FAN + 2] == EC.node_of(snap, EC.member("wfan_b_s")) and list(b[WC.FAN + 2:]) == [1, 0]
    assert WC.FAN > 2 * WC.WINDOW  # several steps and several chunks


def test_the_bad_leaf_needs_the_host():
    snap = WC.graph()
    ex = expand.Engine(snap)
    root = EC.node_of(snap, WC.view("wbad"))
    assert EC.twin(ex, root, 2)[0] == EC.twin(ex, root, WC.ALL)[0] == L.EXPAND_HOST
    assert EC.twin(ex, root, 1)[0] == L.EXPAND_OK  # (one leaf: the row is not read)
    # ... and nothing else of the graph does
    others = [r for r in WC.roots(snap) if r != root]
    assert all(EC.twin(ex, r, WC.ALL)[0] == L.EXPAND_OK for r in others)


def test_row_beginnings_take_the_residues_at_the_word_borders():
    snap = WC.graph()
    ex = expand.Engine(snap)
    begins = WC.row_begins(ex)
    family = [EC.node_of(snap, WC.view(f"wres{i:03d}")) for i in range(WC.RESIDUE_ROWS)]
    assert [begins[v][1] for v in family] == [WC.RESIDUE_LEN0 + i for i in range(WC.RESIDUE_ROWS)]
    # every row of the family is one run of at least 70 leaves: it crosses a mask word
    residues = {begins[v][0] % 64 for v in family}
    assert {0, 1, 62, 63} <= residues, sorted(residues)


def test_host_engine_takes_wide_and_ignores_it():
    snap = WC.graph()
    ex = expand.Engine(snap)
    subjects = [WC.view("WP64_r"), WC.view("wbad"), WC.view("no such object")]
    same = lambda a, b: (a.to_node() if a else None) == (b.to_node() if b else None)
    plain = ex.build_trees_batch(subjects, [3, 3, 3])
    for wide in (False, True):
        got = ex.build_trees_batch(subjects, [3, 3, 3], wide=wide)
        assert same(got[0], plain[0]) and got[0].children and got[2] is None
        assert isinstance(got[1], expand.NotFound) and str(got[1]) == str(plain[1])
        assert ex.build_trees_json_batch(subjects[:1], [3], wide=wide) == [plain[0].MarshalJSON()]


class _NoHandle:
    h = None


def test_out_arrays_are_validated_before_the_call():
    dev = expand.DeviceEngine(WC.graph(), subjects=_NoHandle())
    ok = lambda n=8: np.zeros(n, np.uint32)
    bad = [(ok(),), (ok(), ok(), ok()), (ok(), ok(7)), (ok(7), ok()), (ok(), np.zeros(8, np.int32)),
           (np.zeros(8, np.uint64), ok()), (ok(16)[::2], ok()), (ok(), np.zeros((2, 4), np.uint32)),
           (list(range(8)), ok()), 5]
    both = ok()
    bad.append((both, both))
    frozen = ok()
    frozen.flags.writeable = False
    bad.append((ok(), frozen))
    for wide in (False, True):
        for out in bad:
            with pytest.raises(ValueError):
                dev.expand_ids_raw([0], [2], 8, wide=wide, out=out)
