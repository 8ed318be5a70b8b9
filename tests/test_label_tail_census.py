"""The tail phase restated (tests/label_tail.py tail_stage) on the tail graph: every head
pair reaches every case of the phase and each of its neighbours, and every request's
restated answer — the heads', the phase's or the dense pass's — is the oracle's.  CPU only."""
from collections import Counter

import numpy as np
import pytest

from tests import label_tail as T

AT_LEAST = 3  # requests per case


def cases(heads):
    """Counter of the phase's cases over the tail graph's requests at `heads`"""
    c = T.tail_case()
    li, st = T.staged(heads)
    cp = heads[1] - 4
    n = Counter()
    for s, r, t in zip(st, c["roots"], c["targets"]):
        r, t = int(r), int(t)
        np_ = int(li["P"][r * heads[1]])
        if s["kind"] in ("tail-true", "tail-false"):
            assert cp < np_ <= 2 * cp and s["tail"] == np_ - cp
            n["tail", s["tail"]] += 1
            if s["kind"] == "tail-true":
                n["hit", "first" if s["hit_at"] == 0 else "last" if s["hit_at"] == s["tail"] - 1 else "between"] += 1
                if s["tail"] == 1:  # (its only entry is the first and the last)
                    n["hit", "last"] += 1
            else:
                n["miss", 1 if s["cands"] == 1 else "5+" if s["cands"] >= 5 else "2-4"] += 1
                n["above"] += s["above"]
                n["between"] += s["between"]
        elif s["kind"] == "dense" and np_ == 2 * cp + 1:
            n["np = 2 CP + 1"] += 1
        if s["kind"] in ("dense", "heads"):
            why = T.neighbour(li, r, t, c["ni"])
            if why:
                n["neighbour", why] += 1
                assert (s["kind"] == "heads") == (why in ("es0", "inline-hit")), (why, s)
    return n


@pytest.mark.parametrize("heads", T.HEAD_PAIRS)
def test_tail_graph_reaches_every_case(heads):
    cs, cp = heads[0] - 4, heads[1] - 4
    n = cases(heads)
    want = [("tail", k) for k in T.tail_lengths(cp)] + ["np = 2 CP + 1", ("hit", "first"), ("hit", "last"),
                                                        ("hit", "between"), ("miss", 1), "above", "between"]
    want += [("neighbour", w) for w in ("s-over", "raw-open", "es0", "inline-hit")]
    # five candidates are five inline landmarks of an S that is whole in its head: an 8-word
    # head holds four entries, so that case exists from 32 words on
    if cs >= 5:
        want.append(("miss", "5+"))
    else:
        assert n["miss", "5+"] == 0
    short = {k: n[k] for k in want if n[k] < AT_LEAST}
    assert not short, (heads, short, dict(n))


@pytest.mark.parametrize("heads", T.HEAD_PAIRS)
def test_restated_answers_are_the_oracles(heads):
    c = T.tail_case()
    li, st = T.staged(heads)
    got = T.answers(li, c["roots"], c["targets"], c["ni"], st)
    bad = np.flatnonzero(got != c["want"])
    assert not len(bad), [(c["reqs"][i], st[i], bool(c["want"][i])) for i in bad[:5]]
    k = Counter(s["kind"] for s in st)
    assert min(k["tail-true"], k["tail-false"], k["dense"], k["heads"]) >= 16  # (whole units of each on the GPU)
    assert any(c["want"]) and not all(c["want"])
