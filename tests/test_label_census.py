"""The comb graph (randgraph.make_comb_graph) as an input for plan label's GPU tests
(tests/test_label_lists.py): answered from its lists exactly as the oracle answers, and
reaching every branch of the first stage and of the dense pass that those tests mean to run,
at every forced head pair.  These are conditions on the input, checked here on the host index
(Snapshot.label_index) with the restatements of tests/test_core_index.py and
tests/label_census.py.  CPU only (no device calls).

Measured (seed 95: 8290 rows, 2038 nodes, 2616 requests, 35.5% allowed; the longest S list
has 667 entries, the longest P list 330; (0, 0) chooses 32,32).  Per head pair: requests
without label / mask hits / inline landmark hits with S walked / with P walked / inline
one-edge hits / settled false / dense pass; then of the dense ones: nl > stage by outcome
(landmark, edge, false), nw > 64 with P walked and with S walked, edge hits with S staged
and with S walked, S overflowing only, P only, both:
    (8, 8)    4  16  191   21  12  172  2200 |  424  93  552   248  213   128  20   522  166  1512
    (32, 32)  4  16  303   83  44  442  1724 |  325  90  526   216  179   112   9   631  337   756
    (64, 64)  4  16  383  135  60  657  1361 |  171  56  203   194  136    96   8   559  361   441
    (8, 64)   4  16  343   21  12  230  1990 |  241  58  232   234  154   128  20  1061   97   832
    (64, 8)   4  16    4  316  64  413  1799 |  253  56  203   227  206    96   8   266  635   898
The dense pass counts are what the engine reports as full_requests on the GPU
(tests/test_label_lists.py asserts the equality per call)."""
import numpy as np
import pytest

from tests import label_census as C
from tests.test_core_index import NONE_, check_labels, first_stage

MIN_PER_CLASS = 3


def coverage(cen):
    """requests of a census (label_census.census) in each class the comb graph must reach"""
    dense = lambda f: sum(n for k, n in cen.items() if isinstance(k, tuple) and f(*k[1:]))
    return {
        "inline one-edge hit": cen["edge"],
        "inline landmark hit, S walked": cen["landmark-walk-S"],
        "inline landmark hit, P walked": cen["landmark-walk-P"],
        "settled false": cen["settled-false"],
        "dense, nl > stage, landmark": dense(lambda so, po, w, long_w, long_l, by: long_l and by == "landmark"),
        "dense, nl > stage, edge": dense(lambda so, po, w, long_w, long_l, by: long_l and by == "edge"),
        "dense, nl > stage, false": dense(lambda so, po, w, long_w, long_l, by: long_l and by == "false"),
        "dense, nw > 64, P walked": dense(lambda so, po, w, long_w, long_l, by: long_w and w == "P"),
        "dense, nw > 64, S walked": dense(lambda so, po, w, long_w, long_l, by: long_w and w == "S"),
        "dense edge hit, S staged": dense(lambda so, po, w, long_w, long_l, by: by == "edge" and w == "P"),
        "dense edge hit, S walked": dense(lambda so, po, w, long_w, long_l, by: by == "edge" and w == "S"),
        "dense, S overflows only": dense(lambda so, po, w, long_w, long_l, by: so and not po),
        "dense, P overflows only": dense(lambda so, po, w, long_w, long_l, by: po and not so),
        "dense, both overflow": dense(lambda so, po, w, long_w, long_l, by: so and po),
    }


@pytest.mark.parametrize("heads", C.HEAD_PAIRS)
def test_comb_answers_like_the_oracle(heads):
    """every request answered from the whole lists as the oracle answers it, every request
    the first stage settles settled as the oracle answers it (check_labels), and the dense
    pass's restatement equal to the oracle for every request the first stage leaves open"""
    c = C.comb_case()
    li = check_labels(c["snap"], c["reqs"], c["want"], heads)
    if heads != (0, 0):
        assert (li["s_head_words"], li["p_head_words"]) == heads
    opened = 0
    for i, (r, t) in enumerate(zip(c["roots"], c["targets"])):
        r, t = int(r), int(t)
        if r == NONE_ or t == NONE_ or first_stage(li, r, t, c["ni"]) is not None:
            continue
        f = C.dense_pass(li, r, t, c["ni"])
        assert f["answer"] == bool(c["want"][i]), (c["reqs"][i], f)
        assert f["stage"] == (256 if 64 in (li["s_head_words"], li["p_head_words"]) else 128)
        opened += 1
    assert opened + li["settled"] == int(((c["roots"] != NONE_) & (c["targets"] != NONE_)).sum())


@pytest.mark.parametrize("heads", C.HEAD_PAIRS)
def test_comb_reaches_every_branch(heads):
    """at least MIN_PER_CLASS requests in every class of coverage(), at every head pair, no
    exception: also the inline landmark hit with S walked at (64, 8), where S's inline
    landmarks must be no more than P's 4 inline entries (the users of one and two
    components, inside longer document ranges)"""
    c = C.comb_case()
    cen = C.census(c["snap"], c["roots"], c["targets"], heads)
    assert sum(cen.values()) == len(c["reqs"])
    low = {k: n for k, n in coverage(cen).items() if n < MIN_PER_CLASS}
    assert not low, (heads, low)
    assert cen["mask"] >= MIN_PER_CLASS and cen["none"] >= MIN_PER_CLASS


def test_comb_outcomes_and_lengths():
    """both outcomes occur (allowed share within 0.1 .. 0.9); both sides have lists past the
    device build's 64 entries and lists between every two boundaries of the kernels: the
    inline capacities (4, 12, 28, 60), the device build's 64 and the stages (128, 256)"""
    c = C.comb_case()
    assert 0.1 <= c["want"].mean() <= 0.9
    li = c["snap"].label_index(64, 64)
    for A, n in ((li["S"], li["s_nodes"]), (li["P"], li["p_nodes"])):
        cnt = A[: n * 64].reshape(-1, 64)[:, 0].astype(np.int64)
        bounds = (0, 4, 12, 28, 60, 64, 128, 256, 1 << 30)
        for lo, hi in zip(bounds, bounds[1:]):
            assert ((cnt > lo) & (cnt <= hi)).any(), (lo, hi)
        assert (cnt > 64).sum() >= 2
