"""Plan label's tail phase (device_engine.hip label_unit, TAIL) restated over the built
index, and a graph whose lists reach every case of it.  CPU only (no device calls).

tail_stage() stands beside tests/test_core_index.py first_stage (the first stage of
synchronized calls) and tests/label_census.py classify: a request is decided by the heads,
resolved by the tail phase (true or false), or still listed for the dense pass."""
import functools
import random
from collections import Counter

import numpy as np

from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import label_census as C
from tests import randgraph
from tests.test_core_index import NONE_, first_stage

HEAD_PAIRS = [(8, 8), (32, 32), (64, 64), (8, 64), (64, 8)]


def tail_stage(li, r, t, ni):
    """a queued call's first stage with the tail phase -> dict with
    kind: 'heads' (first_stage decides), 'tail-true' / 'tail-false' (the phase settles the
          request), 'dense' (listed for the dense pass), and answer (None for 'dense');
    for the two tail kinds also tail (entries of P past its head), cands (S's inline
    landmarks above P's last inline entry), hit_at (the tail position of the meeting entry,
    or None), above (a candidate above every tail entry) and between (a candidate strictly
    between two tail entries and equal to none)"""
    d = first_stage(li, r, t, ni)
    if d is not None:
        return {"kind": "heads", "answer": d}
    hs, hp = li["s_head_words"], li["p_head_words"]
    S, P = li["S"], li["P"]
    ns, np_ = int(S[t * hs]), int(P[r * hp])
    cs, cp = hs - 4, hp - 4
    se = S[t * hs + 4: t * hs + hs].astype(np.int64)
    pe = P[r * hp + 4: r * hp + hp].astype(np.int64)
    es = int((se < ni).sum())
    if not (cp < np_ <= 2 * cp and es > 0):
        return {"kind": "dense", "answer": None}
    s_end, p_last = int(se[cs - 1]), int(pe[cp - 1])
    s_whole = ns <= cs or s_end >= ni
    raw_done = r < ni or ns <= cs or r <= s_end
    if not (s_whole and raw_done and int(se[es - 1]) > p_last):
        return {"kind": "dense", "answer": None}
    at = int(P[r * hp + 1]) * 16
    tail = P[at + cp: at + np_].astype(np.int64)  # exactly [CP, np): nothing behind the list is read
    cands = se[:es][se[:es] > p_last]
    assert len(cands) and len(tail) and np.all(np.diff(tail) > 0) and tail[0] > p_last
    where = np.flatnonzero(np.isin(tail, cands))
    hit = len(where) > 0
    return {"kind": "tail-true" if hit else "tail-false", "answer": hit, "tail": len(tail), "cands": len(cands),
            "hit_at": int(where[0]) if hit else None, "above": bool((cands > tail[-1]).any()),
            "between": bool(((cands > tail[0]) & (cands < tail[-1]) & ~np.isin(cands, tail)).any())}


def neighbour(li, r, t, ni):
    """why a request that looks like the tail class must not take the phase: 's-over' (S's
    landmarks not whole inline), 'raw-open' (the one-edge test not settled), 'es0' (S without
    inline landmark), 'inline-hit' (the heads hit), else None.  Only for P lists of the
    phase's lengths (CP < np <= 2 CP)."""
    hs, hp = li["s_head_words"], li["p_head_words"]
    S, P = li["S"], li["P"]
    ns, np_ = int(S[t * hs]), int(P[r * hp])
    cs, cp = hs - 4, hp - 4
    if ns == NONE_ or np_ == NONE_ or not cp < np_ <= 2 * cp:
        return None
    d = first_stage(li, r, t, ni)
    se = S[t * hs + 4: t * hs + hs].astype(np.int64)
    es = int((se < ni).sum())
    if d is True:
        return "inline-hit"
    if d is False:
        return "es0" if es == 0 else None
    s_end = int(se[cs - 1])
    if not (ns <= cs or s_end >= ni):
        return "s-over"
    if not (r < ni or ns <= cs or r <= s_end):
        return "raw-open"
    return None


def stages(li, roots, targets, ni):
    return [tail_stage(li, int(r), int(t), ni) for r, t in zip(roots, targets)]


def answers(li, roots, targets, ni, st):
    """every request's restated answer: the heads', the tail phase's or the dense pass's"""
    return np.array([s["answer"] if s["kind"] != "dense" else C.dense_pass(li, int(r), int(t), ni)["answer"]
                     for s, r, t in zip(st, roots, targets)], dtype=bool)


COMPS = 420
P_CAPS = (4, 28, 60)  # inline entries of a P head of 8, 32, 64 words


# the users made around every document, in order (make_tail_graph)
ROLES = ("first", "last", "inner", "walked-last", "gap", "above", "h", "three", "six", "six-last", "s29", "s61",
         "raw-low", "raw-high", "raw-only", "inline", "edge")


def tail_lengths(cp):
    return sorted({n for n in (1, 3, 4, 5, cp - 1, cp) if 1 <= n <= cp})


def make_tail_graph(seed=11):
    """randgraph.make_comb_graph's components and hub cluster (g{i} -member-> h{i}, both
    interior, of equal centrality: landmark ranks follow the names, every g before every h;
    the hub takes the mask landmarks), with lists of exact contents: a document holds the
    subject sets g{a}, g{a + 2}, ... (P(D): n landmarks with gaps between them), a user is a
    direct member of chosen g{i} (one landmark each), of h{i} (landmarks g{i} and h{i}) and
    a direct subject of leaf objects (raw entries of S(U)).  For every P head capacity CP
    there is a document with each tail length (np - CP in 1, 3, 4, 5, CP - 1, CP) and one of
    2 CP + 1 entries, and around each document users whose landmarks meet its tail at the
    first, the last or an inner entry, miss it (between two entries, above all of them; one
    candidate or many), overflow their own head, leave the one-edge test open, have no
    landmark, or hit inline.  -> (namespaces, rows, requests, docs, pairs): docs[name] =
    (first component, entries); pairs[i] = (document, user, the user's ROLES name) is request
    i, the requests after them pair the users with other documents"""
    rng = random.Random(seed)
    rows = []
    g, h = (lambda i: f"g{i:03d}"), (lambda i: f"h{i:03d}")
    for i in range(COMPS):
        rows.append((1, g(i), "member", None, 1, h(i), "member"))
        rows.append((1, h(i), "member", f"p{i:03d}", None, None, None))
    for x in range(64):  # the hub cluster: the mask landmarks
        for z in ("z0", "z1"):
            rows.append((1, f"c{x:02d}", "member", None, 1, z, "member"))
        rows.append((1, "M000", "view", None, 1, f"c{x:02d}", "member"))
    rows.append((1, "z0", "member", "pz0", None, None, None))
    rows.append((1, "z1", "member", "pz1", None, None, None))
    # every g is some document's subject set (interior: a landmark), first of all B000's: nodes
    # are numbered as the sorted rows first name them, and equal centrality ranks by number
    for i in range(COMPS):
        rows.append((1, "B000", "view", None, 1, g(i), "member"))

    docs, users, pairs = {}, [], []
    leaves = [0]

    def add_user(doc, gs=(), hs=(), raw=0, low=False, direct=False):
        u = f"U{len(users):04d}"
        users.append(u)
        for i in gs:
            rows.append((1, g(i), "member", u, None, None, None))
        for i in hs:
            rows.append((1, h(i), "member", u, None, None, None))
        for _ in range(raw):  # leaf objects that hold u directly: named below ("A") or above ("E") the documents
            rows.append((1, f"{'A' if low else 'E'}{leaves[0]:04d}", "view", u, None, None, None))
            leaves[0] += 1
        if direct:
            rows.append((1, doc, "view", u, None, None, None))
        pairs.append((doc, u, ROLES[len(pairs) % len(ROLES)]))

    for cp in P_CAPS:
        for n in [cp + k for k in tail_lengths(cp)] + [2 * cp + 1]:
            for _ in range(2 if n - cp in (1, 3) else 1):
                a = rng.randrange(8, COMPS - 2 * n - 8)
                d = f"D{len(docs):03d}"
                docs[d] = (a, n)
                for j in range(n):
                    rows.append((1, d, "view", None, 1, g(a + 2 * j), "member"))
                at = lambda j: a + 2 * j            # the list's entry j
                first, last, mid = at(cp), at(n - 1), at(cp + (n - cp) // 2)
                gap = lambda j: at(j) + 1           # between entries j and j + 1 (after the last: above it)
                add_user(d, [first])                                 # hit at the first tail entry
                add_user(d, [last])                                  # at the last
                add_user(d, [mid])                                   # in between (tail of 3 or more)
                add_user(d, [gap(1), gap(cp - 2), last])             # entries below p_last walked first, then the hit
                add_user(d, [gap(cp)])                               # one candidate: between two entries, or above a tail of 1
                add_user(d, [gap(n - 1)])                            # one candidate above every tail entry
                add_user(d, hs=[a + 1])                              # g below p_last, h above everything
                add_user(d, [gap(0), gap(cp), gap(n - 1)], raw=1)    # below, between and above, a raw entry after them
                many = [gap(j) for j in range(cp, cp + 6)]           # six candidates (S heads of 32 and 64 words;
                add_user(d, many)                                    # an 8-word head overflows: its neighbour)
                add_user(d, many[:5] + [last])                       # the sixth candidate hits
                add_user(d, [gap(j) for j in range(cp - 2, cp + 27)])  # 29 landmarks: a 32-word S head overflows
                add_user(d, [gap(j) for j in range(cp - 2, cp + 59)])  # 61: every S head does
                add_user(d, [gap(cp)], raw=70, low=True)             # raw entries past the head, below the document's id
                add_user(d, [gap(cp)], raw=70)                       # ... above it
                add_user(d, raw=2)                                   # no landmark at all
                add_user(d, [at(1), gap(cp)])                        # an inline hit beside a candidate
                add_user(d, [gap(cp)], raw=1, direct=True)           # the one-edge test hits inline
    sub = lambda u: {"subject_id": u}
    assert len(pairs) == len(docs) * len(ROLES)
    reqs = [("n", d, "view", sub(u)) for d, u, _ in pairs]
    names = sorted(docs)
    for k, (d, u, _) in enumerate(pairs):  # every user against two other documents as well
        for step in (5, 11):
            reqs.append(("n", names[(names.index(d) + step + k) % len(names)], "view", sub(u)))
    return [("n", 1)], rows, reqs, docs, pairs


@functools.lru_cache(maxsize=None)
def tail_case(seed=11):
    """the tail graph built and answered once for every test that uses it (read only)"""
    namespaces, rows, reqs, docs, pairs = make_tail_graph(seed)
    snap = Snapshot.from_rows(namespaces, rows, sort=True)
    want = np.asarray(randgraph.oracle_store(namespaces, rows).check_batch(reqs), dtype=bool)
    roots, targets = snap.resolve_many([(ns, o, r, rt.subject_from_dict(s)) for ns, o, r, s in reqs])
    assert not (roots == NONE_).any() and not (targets == NONE_).any()
    for a in (want, roots, targets):
        a.setflags(write=False)
    return {"namespaces": namespaces, "rows": rows, "reqs": reqs, "docs": docs, "pairs": pairs, "snap": snap, "want": want,
            "roots": roots, "targets": targets, "ni": int(snap.stats()["num_interior"])}


@functools.lru_cache(maxsize=None)
def staged(heads):
    """(index, tail_stage of every request) of the tail graph at `heads`, computed once"""
    c = tail_case()
    li = c["snap"].label_index(*heads)
    assert (li["s_head_words"], li["p_head_words"]) == heads
    return li, tuple(stages(li, c["roots"], c["targets"], c["ni"]))


def kinds(heads):
    return np.array([s["kind"] for s in staged(heads)[1]])


def open_count(heads, idx=None):
    """(requests a synchronized call lists for the dense pass, requests a queued call with
    the tail phase still lists) among the requests idx"""
    k = kinds(heads)
    if idx is not None:
        k = k[idx]
    c = Counter(k.tolist())
    return c["dense"] + c["tail-true"] + c["tail-false"], c["dense"]
