"""Which requests does plan label's dense pass get on the config #2 shape, and why?  A CPU
replay of the first stage's decision (device_engine.hip label_unit; tests/test_core_index.py
first_stage) over the host build of the heads: for every request the heads do not settle it
counts whether P or S overflows and names its class.  The tail class is what the tail phase
of queued calls answers in the first stage (S whole in its head, P overflowing, the one-edge
test settled, S with landmarks above P's last inline entry): it is split by the number of
those landmarks (the phase's candidates) and by the length of P's tail, the entries past its
head — the phase reads one more head's worth of them (np <= 2 CP).

    python tools/label_dense_study.py [--tuples N] [--sample CHECKS] [--heads HS,HP]
"""
import argparse
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keto_amd.snapshot import Snapshot
from tools.bench_scale import make
from tools.label_format_study import decode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=int, default=5_000_000, help="rows of the config #2 shape (50M: full scale)")
    ap.add_argument("--sample", type=int, default=20000, help="the workload's checks")
    ap.add_argument("--heads", default="32,32")
    a = ap.parse_args()
    w = make("rbac", a.tuples, a.sample)
    snap = Snapshot.from_columns(w.namespaces, w.columns)
    roots, targets = w.resolve(snap)
    li = snap.label_index(*[int(x) for x in a.heads.split(",")])
    S, P, hs, hp = li["S"], li["P"], li["s_head_words"], li["p_head_words"]
    ni = int(snap.stats()["num_interior"])
    cs, cp = hs - 4, hp - 4
    valid = dense = p_over = s_over = both = 0
    classes, cands, tails = Counter(), Counter(), Counter()
    for r, t in zip(roots.tolist(), targets.tolist()):
        if r == 0xFFFFFFFF or t == 0xFFFFFFFF:
            continue
        pl, pm = decode(P, hp, r)
        sl, sm = decode(S, hs, t)
        if pl is None or sl is None:
            continue
        valid += 1
        if pm & sm:
            continue
        slm = sl[sl < ni]
        s_in, p_in = sl[:cs], pl[:cp]
        if np.intersect1d(s_in[s_in < ni], p_in).size:
            continue
        if r >= ni and (s_in == r).any():
            continue
        s_whole = len(sl) <= cs or s_in[-1] >= ni
        p_whole = len(pl) <= cp
        es, ep = int((s_in < ni).sum()), min(len(pl), cp)
        s_last = s_in[es - 1] if es else 0
        p_last = p_in[ep - 1] if ep else 0
        lm = es == 0 or len(pl) == 0 or (s_whole and (p_whole or s_last <= p_last)) or (p_whole and p_last <= s_last)
        rawd = r < ni or len(sl) <= cs or r <= s_in[-1]
        if lm and rawd:
            continue
        dense += 1
        p_over += not p_whole
        s_over += not s_whole
        both += (not p_whole) and (not s_whole)
        if lm:
            classes["landmarks settled, one-edge test open"] += 1
        elif not s_whole and not p_whole:
            classes["both overflow"] += 1
        elif not s_whole:
            classes["S overflows, P whole"] += 1
        elif not rawd:
            classes["S whole, P overflows, one-edge test open"] += 1
        else:  # the tail class (s_last > p_last: lm failed with S whole)
            classes["tail class"] += 1
            k = int((slm > p_last).sum())
            cands[min(k, 13)] += 1
            n = len(pl) - cp
            tails["<= CP" if n <= cp else "<= 2 CP" if n <= 2 * cp else "longer"] += 1
    n_tail = classes["tail class"]
    pct = lambda x, of: f"{100.0 * x / max(of, 1):.1f} %"
    print(f"tuples {a.tuples}, checks {len(roots)}, valid {valid}, heads {hs}/{hp}")
    print(f"dense {dense} ({pct(dense, valid)} of valid), P overflows {p_over}, S overflows {s_over}, both {both}")
    for k, v in classes.most_common():
        print(f"  {k}: {v} ({pct(v, dense)} of dense)")
    print("tail class by candidates (S landmarks above P's last inline entry; 13 = 13 or more):")
    print("  " + ", ".join(f"{k}: {v}" for k, v in sorted(cands.items())))
    print(f"tail class by tail length (entries of P past its {cp} inline ones):")
    for k in ("<= CP", "<= 2 CP", "longer"):
        print(f"  {k}: {tails[k]} ({pct(tails[k], n_tail)})")
    print(f"one read of at most {4 * cp} bytes settles {tails['<= CP']} = {pct(tails['<= CP'], dense)} of the dense requests")


if __name__ == "__main__":
    main()
