"""Which branch of plan label each request takes: the dense pass (device_engine.hip
label_full_kernel) restated over whole lists, and a census of a request batch over the first
stage's outcomes (tests/test_core_index.py first_stage, the restatement of label_unit) and
the dense pass's cases.  Tests use it to assert that an input reaches the branches they mean
to cover.  CPU only (no device calls)."""
import functools
from collections import Counter

import numpy as np

from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import randgraph
from tests.test_core_index import NONE_, first_stage, label_list

HEAD_PAIRS = [(8, 8), (32, 32), (64, 64), (8, 64), (64, 8), (0, 0)]
PREFETCHED = 64  # walked entries the dense pass fetches before its searches (16 per lane)


def full_stage(hs, hp):
    """words of the dense pass's LDS stage per request (device_engine.hip full_stage)"""
    return 256 if hs >= 64 or hp >= 64 else 128


def dense_pass(li, r, t, ni):
    """label_full_kernel's answer for one request from its two whole lists: the shorter list
    is walked (P when the lengths are equal) and each of its entries searched in the other
    (staged in LDS when it fits the stage, else searched in place), then the one-edge test
    (a non-interior root among S's raw entries).  The masks are the first stage's."""
    hs, hp = li["s_head_words"], li["p_head_words"]
    s, _ = label_list(li["S"], hs, t)
    p, _ = label_list(li["P"], hp, r)
    ns, np_ = len(s), len(p)
    walk_p = np_ <= ns
    walked, other = (p, s) if walk_p else (s, p)
    at = np.searchsorted(other, walked)
    landmark = bool((other[np.minimum(at, len(other) - 1)] == walked).any()) if len(other) else False
    edge = r >= ni and bool((s == r).any())
    return {"walk_p": walk_p, "nw": len(walked), "nl": len(other), "s_over": ns > hs - 4, "p_over": np_ > hp - 4,
            "stage": full_stage(hs, hp), "answer": landmark or edge,
            "by": "landmark" if landmark else "edge" if edge else "false"}


def inline_hit(li, r, t, ni):
    """what gives the first stage's hit (first_stage returned True), in the kernel's order:
    'mask', 'landmark-walk-S' / 'landmark-walk-P' (the shorter inline landmark prefix is the
    walked one, S when equal) or 'edge'"""
    hs, hp = li["s_head_words"], li["p_head_words"]
    S, P = li["S"], li["P"]
    if (int(S[t * hs + 2]) & int(P[r * hp + 2])) or (int(S[t * hs + 3]) & int(P[r * hp + 3])):
        return "mask"
    se = S[t * hs + 4: t * hs + hs]
    es, ep = int((se < ni).sum()), min(int(P[r * hp]), hp - 4)
    if np.isin(se[:es], P[r * hp + 4: r * hp + 4 + ep]).any():
        return "landmark-walk-S" if es <= ep else "landmark-walk-P"
    assert r >= ni and (se == r).any()
    return "edge"


def classify(li, r, t, ni):
    """one request's class: 'none' (an id missing or a head without label), 'mask',
    'landmark-walk-S', 'landmark-walk-P', 'edge' (inline hits), 'settled-false', or the dense
    pass's case ('dense', S overflows, P overflows, 'P' / 'S' walked, nw > 64, nl > stage,
    'landmark' / 'edge' / 'false')"""
    hs, hp = li["s_head_words"], li["p_head_words"]
    if r == NONE_ or t == NONE_ or int(li["S"][t * hs]) == NONE_ or int(li["P"][r * hp]) == NONE_:
        return "none"
    d = first_stage(li, r, t, ni)
    if d is True:
        return inline_hit(li, r, t, ni)
    if d is False:
        return "settled-false"
    f = dense_pass(li, r, t, ni)
    return ("dense", f["s_over"], f["p_over"], "P" if f["walk_p"] else "S", f["nw"] > PREFETCHED, f["nl"] > f["stage"],
            f["by"])


def census(snap, roots, targets, heads):
    """Counter of classify() over the requests, with the index built for `heads`"""
    li = snap.label_index(*heads)
    ni = int(snap.stats()["num_interior"])
    return Counter(classify(li, int(r), int(t), ni) for r, t in zip(roots, targets))


def dense_count(c):
    """requests of a census that go to the dense pass"""
    return sum(n for k, n in c.items() if isinstance(k, tuple))


@functools.lru_cache(maxsize=None)
def comb_case(seed=95):
    """the comb graph, built and answered once for every test that uses it (read only):
    -> dict with namespaces, rows, reqs, snap, want (the oracle's answers), roots, targets, ni"""
    namespaces, rows, reqs = randgraph.make_comb_graph(seed)
    snap = Snapshot.from_rows(namespaces, rows, sort=True)
    want = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    for a in (want, roots, targets):
        a.setflags(write=False)
    return {"namespaces": namespaces, "rows": rows, "reqs": reqs, "snap": snap, "want": want, "roots": roots,
            "targets": targets, "ni": int(snap.stats()["num_interior"])}
